"""Where one iteration of inference.laplace.laplace_grad spends its time on the headline shape of scripts/laplace_times.py
(FitzHugh-Nagumo, p = 3, N = 4000, 41 observations, k = 5 parameters: log theta and x0), for C = 1 and C = 20 centres (11 and 220
points per call, 9 directions a point) and for `fenrir_grad` and `dalton_grad` as the log-likelihood, next to one iteration of
`laplace` (51 and 1020 points) of the same build.  Parts, host clock around calls that end in a synchronising copy:
  stencil   upload of the centres + the stencil kernel + download of the points
  user      the user's function: constraint transform and chain rule on the host + the batched likelihood call
  lik       of which the `*_grad` (or `fenrir` / `dalton`) call alone
  reduce    upload of values (and gradients) + the reduction kernel + download of gradient, Hessian, n_bad (and grad_fd)
  step      upload of gradient, Hessian, damping + newton_step_kernel + download of delta, logdet, ok
2 warm-up iterations, then the median of 9.  Then the number of iterations both modes take on the fit of
examples/fitzhugh_laplace_grad.py (its data, its start, max_iter = 100), with the exact gradient at each mode.

    python scripts/laplace_grad_times.py [--out profiles/laplace_grad_times.txt]            (needs an MI355X)
"""
import argparse
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import rodeo_amd as ra
from rodeo_amd.inference import laplace as lap
from rodeo_amd.inference.fenrir import fenrir_grad
from rodeo_amd.inference.dalton import dalton_grad
from rodeo_amd.interrogate import interrogate_kramer
import fitzhugh_laplace_grad as ex

N, T_MAX, P, K = 4000, 40.0, 3, 5
THETA, X0 = np.array([0.2, 0.2, 3.0]), np.array([-1.0, 1.0])
W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, P)
prior = ra.ibm_init(T_MAX / N, P, np.array([0.1, 0.1]))
obs_times = np.linspace(0.0, T_MAX, 41)
WARM, KEEP = 2, 9
lik_s = []


def make_data():
    Xt, _ = ra.solve_mv(None, ra.ode.fitzhugh_nagumo, W, init(X0, 0.0, theta=THETA), 0.0, T_MAX, N, interrogate_kramer, prior,
                        theta=THETA)
    sd = np.sqrt(0.005)
    Y = (Xt[::N // 40, :, 0] + sd * np.random.default_rng(0).standard_normal((41, 2)))[:, :, None]
    OW = np.zeros((41, 2, 1, P)); OW[..., 0] = 1.0
    return Y, OW, np.full((41, 2, 1, 1), sd ** 2)


def make_logpost(fn, Y, OW, OV):
    def logpost(u):
        th = np.exp(u[:, :3])
        X = np.stack([init(u[b, 3:5], 0.0, theta=th[b]) for b in range(len(u))])
        t0 = time.perf_counter()
        ll = fn(None, ra.ode.fitzhugh_nagumo, W, X, 0.0, T_MAX, N, interrogate_kramer, prior, Y, obs_times, OW, OV, theta=th)
        lik_s.append(time.perf_counter() - t0)
        return ll + np.sum(-0.5 * (u / 10.0) ** 2, axis=1)
    return logpost


def make_value_and_grad(fn, Y, OW, OV):
    def value_and_grad(u):
        th, v0 = np.exp(u[:, :3]), u[:, 3:5]
        X = np.stack([init(v0[b], 0.0, theta=th[b]) for b in range(len(u))])
        J = ex.fitz_init_jac(v0, th)
        t0 = time.perf_counter()
        res = fn(None, ra.ode.fitzhugh_nagumo, W, X, 0.0, T_MAX, N, interrogate_kramer, prior, Y, obs_times, OW, OV,
                 wrt=("theta", "ode_init"), init_jac=dict(theta=J), theta=th)
        lik_s.append(time.perf_counter() - t0)
        d_theta = np.zeros((len(u), 3, K))
        d_theta[:, np.arange(3), np.arange(3)] = th
        d_x0 = np.zeros((len(u), 2, P, K))
        d_x0[..., 3:5] = ex.fitz_init_dv0(v0, th)
        return res.value + np.sum(-0.5 * (u / 10.0) ** 2, axis=1), lap.pull_back(res.grad, dict(theta=d_theta, ode_init=d_x0)) - u / 100.0
    return value_and_grad


def one_iteration(mode, dv, fun, u, damping):
    t = [time.perf_counter()]
    if mode == "laplace_grad":
        pts = dv.grad_stencil(u); t.append(time.perf_counter())
        vals, grads = fun(pts); t.append(time.perf_counter())
        g, H, bad, _ = dv.hess_from_grad(vals, grads); t.append(time.perf_counter())
    else:
        pts = dv.stencil(u); t.append(time.perf_counter())
        vals = fun(pts); t.append(time.perf_counter())
        g, H, bad = dv.grad_hess(vals); t.append(time.perf_counter())
    delta, logdet, ok = dv.newton(g, H, damping); t.append(time.perf_counter())
    return list(np.diff(t)) + [lik_s[-1]], int(bad.sum()), int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "laplace_grad_times.txt"))
    out_path = ap.parse_args().out
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = ra.default_device()
    say(f"# scripts/laplace_grad_times.py on one MI355X {dev.name().strip()}: FitzHugh-Nagumo, p = {P}, N = {N}, 41 observations, "
        f"k = {K}; median of {KEEP} iterations after {WARM} warm-up, ms")
    Y, OW, OV = make_data()
    for name, fn, fn_grad in (("fenrir", ra.inference.fenrir, fenrir_grad), ("dalton", ra.inference.dalton, dalton_grad)):
        for n_c in (1, 20):
            u = np.concatenate([np.log(THETA), X0])[None] + 0.01 * np.random.default_rng(1).standard_normal((n_c, K))
            for mode, dv, fun in (("laplace_grad", lap.DeviceGradSteps(n_c, K, lap.default_grad_step(u)), make_value_and_grad(fn_grad, Y, OW, OV)),
                                  ("laplace     ", lap.DeviceSteps(n_c, K, lap.default_step(u)), make_logpost(fn, Y, OW, OV))):
                rows = [one_iteration(mode.strip(), dv, fun, u, np.zeros(n_c)) for _ in range(WARM + KEEP)]
                med = np.median(np.array([r[0] for r in rows[WARM:]]), axis=0) * 1e3
                total = float(np.sum(med[:4]))
                say(f"{name} C={n_c:2d} {mode} ({n_c * dv.S:4d} points): stencil {med[0]:.3f}  user {med[1]:.3f} (lik call {med[4]:.3f})  "
                    f"reduce {med[2]:.3f}  step {med[3]:.3f}  iteration {total:.3f}  |  n_bad {rows[-1][1]} ok {rows[-1][2]}/{n_c}")
    say("# iterations to convergence on the fit of examples/fitzhugh_laplace_grad.py (max_iter = 100, gtol = 1e-5)")
    data = ex.make_data()
    start = np.append(np.log(ex.theta), ex.x0)
    for name, fn, fn_grad in (("fenrir", ra.inference.fenrir, fenrir_grad), ("dalton", ra.inference.dalton, dalton_grad)):
        vg = ex.value_and_grad_for(fn_grad, data)
        fits = {}
        for mode, run in (("laplace_grad", lambda: lap.laplace_grad(vg, start, max_iter=100, check_grad=name != "dalton")),
                          ("laplace     ", lambda: lap.laplace(ex.logpost_for(fn, data), start, max_iter=100))):
            t0 = time.perf_counter()
            fit = fits[mode.strip()] = run()
            wall = time.perf_counter() - t0
            g = vg(fit.mode[None])[1]
            say(f"{name} {mode}: converged {bool(fit.converged)}  n_iter {fit.n_iter}  wall {wall:.2f} s  log-posterior {fit.logpost:.9f}  "
                f"log-evidence {fit.log_evidence:.6f}  max |exact gradient| at the mode {np.max(np.abs(g)):.2e}  n_bad {int(fit.n_bad)}")
        a, b = fits["laplace_grad"], fits["laplace"]
        say(f"{name}: modes differ by {np.max(np.abs(a.mode - b.mode)):.2e}, Hessians by {np.max(np.abs(a.hessian - b.hessian)):.2e} of "
            f"{np.max(np.abs(a.hessian)):.2e}, log-evidence by {abs(a.log_evidence - b.log_evidence):.2e}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
