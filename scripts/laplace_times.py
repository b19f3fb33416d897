"""Where one iteration of inference.laplace spends its time on the headline shape (FitzHugh-Nagumo, p = 3, N = 4000, 41
observations, k = 5 parameters: log theta and x0), for C = 1 and C = 20 centres (51 and 1020 trajectories per log-posterior
call) and for `fenrir` and `dalton` as the log-likelihood.  Parts, host clock around calls that end in a synchronising copy:
  stencil   upload of the centres + fd_stencil_kernel + download of the (C S, k) points
  logpost   the user's function: constraint transform on the host (one init call per point) + the batched solver call
  solver    of which the `fenrir` / `dalton` call alone
  reduce    upload of the (C S,) values + fd_grad_hess_kernel + download of gradient, Hessian and n_bad
  step      upload of gradient, Hessian, damping + newton_step_kernel + download of delta, logdet, ok
and the three kernels alone from device events (rk_profile_enable) in five further iterations.  3 warm-up iterations, then
the median of 20.

    python scripts/laplace_times.py            (needs an MI355X)
"""
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rodeo_amd as ra
from rodeo_amd.inference import laplace as lap
from rodeo_amd.interrogate import interrogate_kramer

N, T_MAX, P, K = 4000, 40.0, 3, 5
THETA, X0 = np.array([0.2, 0.2, 3.0]), np.array([-1.0, 1.0])
W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, P)
prior = ra.ibm_init(T_MAX / N, P, np.array([0.1, 0.1]))
obs_times = np.linspace(0.0, T_MAX, 41)
Xt, _ = ra.solve_mv(None, ra.ode.fitzhugh_nagumo, W, init(X0, 0.0, theta=THETA), 0.0, T_MAX, N, interrogate_kramer, prior,
                    theta=THETA)
sd = np.sqrt(0.005)
Y = (Xt[::N // 40, :, 0] + sd * np.random.default_rng(0).standard_normal((41, 2)))[:, :, None]
OW = np.zeros((41, 2, 1, P)); OW[..., 0] = 1.0
OV = np.full((41, 2, 1, 1), sd ** 2)
solver_s = []


def make_logpost(fn):
    def logpost(u):
        th = np.exp(u[:, :3])
        X = np.stack([init(u[b, 3:5], 0.0, theta=th[b]) for b in range(len(u))])
        t0 = time.perf_counter()
        ll = fn(None, ra.ode.fitzhugh_nagumo, W, X, 0.0, T_MAX, N, interrogate_kramer, prior, Y, obs_times, OW, OV, theta=th)
        solver_s.append(time.perf_counter() - t0)
        return ll + np.sum(-0.5 * (u / 10.0) ** 2, axis=1)
    return logpost


def main():
    dev = ra.default_device()
    print(f"# scripts/laplace_times.py on one MI355X {dev.name().strip()}: FitzHugh-Nagumo, p = {P}, N = {N}, 41 observations, k = {K}; "
          f"median of 20 iterations after 3 warm-up, ms")
    for name, fn in (("fenrir", ra.inference.fenrir), ("dalton", ra.inference.dalton)):
        logpost = make_logpost(fn)
        for n_c in (1, 20):
            u = np.concatenate([np.log(THETA), X0])[None] + 0.01 * np.random.default_rng(1).standard_normal((n_c, K))
            dv = lap.DeviceSteps(n_c, K, lap.default_step(u))
            damping = np.zeros(n_c)
            rows = []
            for it in range(28):
                if it == 23:                 # kernel times from device events in five more iterations, kept out of the wall times
                    dev.profile_enable(True, keep=True)
                t = [time.perf_counter()]
                pts = dv.stencil(u); t.append(time.perf_counter())
                vals = logpost(pts); t.append(time.perf_counter())
                g, H, bad = dv.grad_hess(vals); t.append(time.perf_counter())
                delta, logdet, ok = dv.newton(g, H, damping); t.append(time.perf_counter())
                rows.append(list(np.diff(t)) + [solver_s[-1]])
            prof = dev.profile_last(4096)
            dev.profile_enable(False)
            med = np.median(np.array(rows[3:23]), axis=0) * 1e3
            kern = {k: float(np.median([ms for nm, ms in prof if nm == k])) for k in
                    ("fd_stencil_kernel", "fd_grad_hess_kernel", "newton_step_kernel")}
            total = float(np.sum(med[:4]))
            print(f"{name} C={n_c:2d} ({n_c * dv.S:4d} trajectories): stencil {med[0]:.3f}  logpost {med[1]:.3f} (solver call "
                  f"{med[4]:.3f})  reduce {med[2]:.3f}  step {med[3]:.3f}  iteration {total:.3f}  |  new kernels + their "
                  f"transfers {100 * (med[0] + med[2] + med[3]) / total:.1f} % of the iteration  |  kernels alone: "
                  + "  ".join(f"{k} {v:.4f}" for k, v in kern.items()) + f"  |  n_bad {int(bad.sum())} ok {int(ok.sum())}/{n_c}",
                  flush=True)


if __name__ == "__main__":
    main()
