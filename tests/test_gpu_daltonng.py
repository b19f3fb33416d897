"""
DALTON for non-Gaussian observations on the device (rodeo_amd.inference.dalton.daltonng / solve_mv_nn,
src/rodeo/inference/dalton.py:547-1039) against the NumPy restatement tests/daltonng_oracle.py.  The device differentiates the
traced log-likelihood with second-order duals; the oracle uses hand-written derivatives.
"""
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401  (the package binds the name `dalton` to the function)
from rodeo_amd.interrogate import interrogate_kramer, interrogate_rodeo, interrogate_schober
from rodeo_amd.trace import gammaln
from oracle import odes, priors, interrogations as oi
import daltonng_oracle as ng

dmod = sys.modules["rodeo_amd.inference.dalton"]
pytestmark = pytest.mark.gpu

ITG = {"kramer": (interrogate_kramer, oi.interrogate_kramer), "rodeo": (interrogate_rodeo, oi.interrogate_rodeo),
       "schober": (interrogate_schober, oi.interrogate_schober)}
THETA = np.array([0.2, 0.2, 3.0])
# dt = 0.025 as in tests/test_gpu_dalton.py's p = 3 cases: the kramer and schober filters stay finite there for every theta used
# (at dt = 0.2 the oracle itself overflows for kramer / schober at p = 4, 5); the batch spreads theta by 1 % per element
LANE = {3: dict(N=80, t_max=2.0), 4: dict(N=80, t_max=2.0, sigma=10.0), 5: dict(N=80, t_max=2.0, sigma=10.0)}


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _fhn(p, N=40, t_max=4.0, B=None, sigma=0.1, times=None):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    thetas = THETA if B is None else THETA * (1 + 0.01 * np.arange(B))[:, None]
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    prior = priors.ibm_init(t_max / N, p, np.array([sigma, sigma]))
    if times is None:
        times = np.concatenate([np.linspace(0.37, t_max - 0.21, 6), [t_max]])          # off-grid times and t_max
    y = np.random.default_rng(0).poisson(1.5, size=(len(times), 2, 1)).astype(np.float64)
    return dict(W=W, x0=x0, N=N, t_max=t_max, prior=prior, thetas=thetas, y=y, times=np.asarray(times))


def _device(fn, c, itg, loglik=poisson_loglik, ode_fun=ra.ode.fitzhugh_nagumo):
    return fn(None, ode_fun, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][0], c["prior"], c["y"], c["times"], loglik,
              theta=c["thetas"])


def _oracle(fn, c, itg, theta, fns=None, active=((0,), (0,))):
    return fn(odes.fitzhugh_nagumo, c["W"], c["x0"], 0.0, c["t_max"], c["N"], ITG[itg][1], c["prior"], c["y"], c["times"],
              *(fns or ng.poisson()), active=active, theta=theta)


def _check_ll(val, ref, rtol=1e-7, moved=0.0):
    """tests/test_gpu_dalton.py's bar; `moved`: how far the oracle itself moves under a 1e-15 relative perturbation of the prior
    variance (the yardstick of DESIGN.md section 2) -- the division by H amplifies rounding where the filter is ill-conditioned,
    and the value is then held within 20 x that, the factor tests/test_gpu_tilen.py uses against its yardstick."""
    print(f"daltonng {val!r} oracle {ref!r} rel {abs(val - ref) / max(1.0, abs(ref)):.3e} oracle moves {moved:.3e}")
    assert abs(val - ref) <= max(rtol * max(1.0, abs(ref)), 20.0 * moved), (val, ref, moved)


ILL = {(5, "schober")}          # where 1e-7 / 1e-8 were measured to be missed; every other case holds the bar


def _moved(c, itg, theta, ref):
    if (c["W"].shape[-1], itg) not in ILL:
        return 0.0
    Q, R = c["prior"]
    return abs(_oracle(ng.daltonng, dict(c, prior=(Q, R * (1.0 + 1e-15))), itg, theta) - ref)


def _check_mv(m, v, mo, vo, tol=1e-8, moved=(0.0, 0.0)):
    """tests/test_gpu_dalton.py's solve_mv bounds; `moved`: the same yardstick as in _check_ll, for the mean and the variance."""
    em, ev = np.max(np.abs(m - mo)) / max(1.0, np.max(np.abs(mo))), np.max(np.abs(v - vo)) / max(1.0, np.max(np.abs(vo)))
    print(f"solve_mv_nn mean {em:.3e} var {ev:.3e} oracle moves {moved[0]:.3e} {moved[1]:.3e}")
    assert em <= max(tol, 20.0 * moved[0]) and ev <= max(tol, 20.0 * moved[1]), (em, ev, moved)


def _moved_mv(c, itg, theta, mo, vo):
    if (c["W"].shape[-1], itg) not in ILL:
        return 0.0, 0.0
    Q, R = c["prior"]
    m2, v2 = _oracle(ng.solve_mv_nn, dict(c, prior=(Q, R * (1.0 + 1e-15))), itg, theta)
    return np.max(np.abs(m2 - mo)) / max(1.0, np.max(np.abs(mo))), np.max(np.abs(v2 - vo)) / max(1.0, np.max(np.abs(vo)))


@pytest.mark.parametrize("itg", ["kramer", "rodeo", "schober"])
@pytest.mark.parametrize("p", [3, 4, 5])
def test_poisson_fhn_single_and_batched(p, itg):
    c = _fhn(p, **LANE[p])
    val = _device(dmod.daltonng, c, itg)
    assert isinstance(val, float)
    ref = _oracle(ng.daltonng, c, itg, THETA)
    _check_ll(val, ref, moved=_moved(c, itg, THETA, ref))
    mo, vo = _oracle(ng.solve_mv_nn, c, itg, THETA)
    _check_mv(*_device(dmod.solve_mv_nn, c, itg), mo, vo, moved=_moved_mv(c, itg, THETA, mo, vo))
    cb = _fhn(p, B=3, **LANE[p])
    vals = _device(dmod.daltonng, cb, itg)
    m, v = _device(dmod.solve_mv_nn, cb, itg)
    assert vals.shape == (3,) and m.shape == (3, cb["N"] + 1, 2, p) and v.shape == (3, cb["N"] + 1, 2, p, p)
    for b in (0, 2):
        ref = _oracle(ng.daltonng, cb, itg, cb["thetas"][b])
        _check_ll(vals[b], ref, moved=_moved(cb, itg, cb["thetas"][b], ref))
        mo, vo = _oracle(ng.solve_mv_nn, cb, itg, cb["thetas"][b])
        _check_mv(m[b], v[b], mo, vo, moved=_moved_mv(cb, itg, cb["thetas"][b], mo, vo))


@pytest.mark.parametrize("p", [3, 4, 5])
def test_poisson_with_a_traced_python_rhs(p):
    c = _fhn(p, **LANE[p])
    c["W"], _ = ra.utils.first_order_pad(_fitz, 2, p)
    _check_ll(_device(dmod.daltonng, c, "kramer", ode_fun=_fitz), _oracle(ng.daltonng, c, "kramer", THETA))
    _check_mv(*_device(dmod.solve_mv_nn, c, "kramer", ode_fun=_fitz), *_oracle(ng.solve_mv_nn, c, "kramer", THETA))
    cb = _fhn(p, B=3, **LANE[p])
    vals = _device(dmod.daltonng, cb, "rodeo", ode_fun=_fitz)
    m, v = _device(dmod.solve_mv_nn, cb, "rodeo", ode_fun=_fitz)
    assert vals.shape == (3,)
    for b in (0, 2):
        _check_ll(vals[b], _oracle(ng.daltonng, cb, "rodeo", cb["thetas"][b]))
        _check_mv(m[b], v[b], *_oracle(ng.solve_mv_nn, cb, "rodeo", cb["thetas"][b]))


S2 = 0.05


def gauss_loglik(y, X, ind, **params):
    r = y[:, 0] - X[:, 0]
    return np.sum(-0.5 * r * r / S2 - 0.5 * np.log(2 * np.pi * S2))


def test_gaussian_loglik_solve_mv_nn_equals_dalton_solve_mv_on_the_device():
    c = _fhn(3, B=3, **LANE[3])
    c["y"] = np.random.default_rng(2).standard_normal(c["y"].shape) * 0.5
    n = len(c["times"])
    D = np.zeros((n, 2, 1, 3))
    D[..., 0] = 1.0
    m, v = _device(dmod.solve_mv_nn, c, "kramer", loglik=gauss_loglik)
    mo, vo = dmod.solve_mv(None, ra.ode.fitzhugh_nagumo, c["W"], c["x0"], 0.0, c["t_max"], c["N"], interrogate_kramer, c["prior"],
                           c["y"], c["times"], D, np.full((n, 2, 1, 1), S2), theta=c["thetas"])
    _check_mv(m, v, mo, vo, tol=1e-9)


def test_gaussian_loglik_daltonng_equals_dalton_on_the_linear_ode():
    """(the prior scale of tests/test_oracle_daltonng.py's case: Bayes' identity holds between densities)"""
    N, t_max, p = 10, 1.0, 3
    W = np.array([[[0.0, 0.0, 1.0]]]); x0 = np.array([[-1.0, 0.0, 1.0]])
    prior = priors.ibm_init(t_max / N, p, np.array([5.0]))
    times = np.array([0.2, 0.5, 1.0])
    y = np.random.default_rng(0).standard_normal((3, 1, 1)) * 0.3 - 0.5
    D = np.tile(np.array([1.0, 0.0, 0.0])[None, None, None, :], (3, 1, 1, 1))
    val = dmod.daltonng(None, ra.ode.higher_order, W, x0, 0.0, t_max, N, interrogate_kramer, prior, y, times, gauss_loglik)
    ref = dmod.dalton(None, ra.ode.higher_order, W, x0, 0.0, t_max, N, interrogate_kramer, prior, y, times, D,
                      np.full((3, 1, 1, 1), S2))
    _check_ll(val, ref, 1e-7)


def coupled_loglik(y, X, ind, theta):
    """couples the blocks (gradients at the joint point, diagonal Hessian blocks kept), two active components in block 0
    (MO = 2), a parameter of **params inside."""
    r0 = y[0, 0] - X[0, 0] * X[1, 0]
    r1 = y[1, 0] - theta[0] * X[0, 1]
    return -0.5 * r0 * r0 / 0.04 - 0.5 * r1 * r1 / 0.25 - 0.5 * (X[0, 0] - 0.3 * X[0, 1]) ** 2 - 0.5 * X[1, 0] ** 2


def test_coupled_blocks_two_active_components_t_min_and_a_parameter():
    c = _fhn(3, B=2, times=np.array([0.0, 0.5, 1.13, 2.0]), **LANE[3])
    c["y"] = np.random.default_rng(4).standard_normal(c["y"].shape) * 0.3
    fns, act = ng.coupled(), ((0, 1), (0,))
    vals = _device(dmod.daltonng, c, "kramer", loglik=coupled_loglik)
    m, v = _device(dmod.solve_mv_nn, c, "kramer", loglik=coupled_loglik)
    for b in range(2):
        _check_ll(vals[b], _oracle(ng.daltonng, c, "kramer", c["thetas"][b], fns, act))
        _check_mv(m[b], v[b], *_oracle(ng.solve_mv_nn, c, "kramer", c["thetas"][b], fns, act))


def test_two_calls_return_identical_bits_and_the_plan_keeps_no_output_buffers(monkeypatch):
    from rodeo_amd.solve import _plan_cache
    c = _fhn(3, B=7, N=23, t_max=2.3)
    a = _device(dmod.daltonng, c, "kramer")
    plans = [pl for pl in _plan_cache.values() if pl.N == 23]
    assert plans and all(pl._bufs == {} and pl.mean_state is None and pl.var_state is None for pl in plans)
    assert all("_daltonng_ws" not in pl.__dict__ for pl in plans)    # the workspace lived for the call only
    b = _device(dmod.daltonng, c, "kramer")
    assert a.tobytes() == b.tobytes()
    # the same plan (batch-minor: dalton's lane route), now with outputs: dalton.solve_mv, then solve_mv_nn
    n = len(c["times"])
    D = np.zeros((n, 2, 1, 3)); D[..., 0] = 1.0
    gauss = lambda: dmod.solve_mv(None, ra.ode.fitzhugh_nagumo, c["W"], c["x0"], 0.0, c["t_max"], c["N"], interrogate_kramer,  # noqa: E731
                                  c["prior"], c["y"], c["times"], D, np.full((n, 2, 1, 1), 0.3), theta=c["thetas"])
    monkeypatch.setenv("RK_DALTON_LANES", "1")
    n_plans = len(_plan_cache)
    ml, vl = gauss()
    assert len(_plan_cache) == n_plans                               # no new plan: the one daltonng used
    monkeypatch.setenv("RK_DALTON_LANES", "0")
    _check_mv(ml, vl, *gauss(), tol=1e-9)                            # (the tile route, on a plan of its own)
    m, v = _device(dmod.solve_mv_nn, c, "kramer")
    _check_mv(m[0], v[0], *_oracle(ng.solve_mv_nn, c, "kramer", c["thetas"][0]))


def test_a_non_concave_likelihood_returns_nan_without_a_fault():
    """+x^2 / 2 has H = +1 at every point: known from the formula."""
    c = _fhn(3, B=3, **LANE[3])
    vals = _device(dmod.daltonng, c, "kramer", loglik=lambda y, X, i, **kw: 0.5 * np.sum(X[:, 0] ** 2))
    assert vals.shape == (3,) and np.all(np.isnan(vals))
    m, _ = _device(dmod.solve_mv_nn, c, "kramer", loglik=lambda y, X, i, **kw: 0.5 * np.sum(X[:, 0] ** 2))
    assert np.all(np.isnan(m[:, -1]))
    assert np.isfinite(_device(dmod.daltonng, _fhn(3, **LANE[3]), "kramer"))           # the device still answers


def test_laplace_around_daltonng_agrees_with_the_driver_on_the_cpu_oracle():
    """inference.laplace around daltonng on the example's model (FitzHugh-Nagumo, Poisson counts with rate exp(0.1 + 0.5 x),
    theta and x(0) free), held to the bounds tests/test_gpu_laplace.py holds fenrir to: with r = 1e-7 the parity of the
    log-density, h the stencil step and f the log-posterior at the mode, the Hessians agree within 4 r |f| / h^2, and the modes
    within |H^-1| sqrt(5) (2 gtol + r |f| / h), both runs stopping where their own gradient is below gtol.  The 51 stencil points
    of an iteration are one batched daltonng call, so this also checks that the batched value is smooth in theta at the scale
    of the stencil."""
    from rodeo_amd.inference import laplace as lap
    N, t_max, p, n_obs = 100, 10.0, 3, 21
    theta, x0 = THETA, np.array([-1.0, 1.0])
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    prior = ra.ibm_init(t_max / N, p, np.array([0.1, 0.1]))
    obs_times = np.linspace(0.0, t_max, n_obs)
    X, _ = ra.solve_mv(None, ra.ode.fitzhugh_nagumo, W, init(x0, 0.0, theta=theta), 0.0, t_max, N, interrogate_kramer, prior,
                       theta=theta)
    idx = np.searchsorted(np.linspace(0.0, t_max, N + 1), obs_times)
    y = np.random.default_rng(100).poisson(np.exp(0.1 + 0.5 * X[idx, :, 0])).astype(np.float64)[:, :, None]

    def constrain(u):
        th = np.exp(u[:, :3])
        return th, np.stack([init(u[b, 3:5], 0.0, theta=th[b]) for b in range(len(u))])

    def logprior(u):
        return np.sum(-0.5 * (u / 10.0) ** 2 - np.log(10.0) - 0.5 * np.log(2 * np.pi), axis=1)

    def logpost_dev(u):
        th, X0 = constrain(u)
        return dmod.daltonng(None, ra.ode.fitzhugh_nagumo, W, X0, 0.0, t_max, N, interrogate_kramer, prior, y, obs_times,
                             poisson_loglik, theta=th) + logprior(u)

    def logpost_cpu(u):
        th, X0 = constrain(u)
        return np.array([ng.daltonng(odes.fitzhugh_nagumo, W, X0[b], 0.0, t_max, N, oi.interrogate_kramer, prior, y, obs_times,
                                     *ng.poisson(), active=((0,), (0,)), theta=th[b]) for b in range(len(u))]) + logprior(u)

    start = np.concatenate([np.log(theta), x0]) + 0.05
    gtol = 1e-5
    dev = lap.laplace(logpost_dev, start, gtol=gtol)
    print(f"laplace_daltonng device: converged {bool(dev.converged)} n_iter {dev.n_iter} logpost {float(dev.logpost)!r} "
          f"eig(H) {np.linalg.eigvalsh(dev.hessian)}")
    cpu = lap.laplace(logpost_cpu, start, gtol=gtol)
    h = float(np.min(lap.default_step(start)))
    fmax = max(1.0, abs(cpu.logpost))
    tol_H, tol_g = 4 * 1e-7 * fmax / h ** 2, 1e-7 * fmax / h
    tol_mode = np.linalg.norm(np.linalg.inv(cpu.hessian), 2) * np.sqrt(5) * (2 * gtol + tol_g)
    dv = lap.DeviceSteps(1, 5, lap.default_step(start))
    g_mode, _, _ = dv.grad_hess(logpost_dev(dv.stencil(dev.mode[None])))
    e_H, e_mode = float(np.max(np.abs(dev.hessian - cpu.hessian))), float(np.max(np.abs(dev.mode - cpu.mode)))
    print(f"laplace_daltonng n_iter_dev={dev.n_iter} n_iter_cpu={cpu.n_iter} grad_at_mode={float(np.max(np.abs(g_mode))):.3e} "
          f"hess_diff={e_H:.3e} tol_hess={tol_H:.3e} hess_scale={float(np.max(np.abs(cpu.hessian))):.3e} mode_diff={e_mode:.3e} "
          f"tol_mode={float(tol_mode):.3e} logpost_diff={float(abs(dev.logpost - cpu.logpost)):.3e}")
    assert bool(dev.converged) and bool(cpu.converged)
    assert np.max(np.abs(g_mode)) < gtol
    assert np.all(np.linalg.eigvalsh(dev.hessian) < 0)
    assert e_H <= tol_H and e_mode <= tol_mode
    assert np.all(np.isfinite(dev.cov))
