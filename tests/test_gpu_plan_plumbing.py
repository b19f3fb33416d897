"""
The host-side bookkeeping that the inference callers share on one cached ``SolvePlan``: which launches bump ``generation``, what
is uploaded again when ``dalton`` and ``fenrir`` alternate, and what a path-less ``sim_logpost`` leaves allocated.
FitzHugh-Nagumo, two blocks, n_bstate 3, 20 steps, B = 3 (the MFMA-tile route of every caller).
"""
import functools
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401  (the package binds the name `dalton` to the function)
import rodeo_amd.solve as solve
from rodeo_amd.inference import basic, fenrir, sim_logpost
from rodeo_amd.inference.basic import GaussianObsLoglik
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer

dmod = sys.modules["rodeo_amd.inference.dalton"]
pytestmark = pytest.mark.gpu

N, T_MAX, P, B = 20, 2.0, 3, 3
THETAS = np.array([0.2, 0.2, 3.0]) * (1 + 0.05 * np.arange(B))[:, None]
TIMES = np.array([0.0, 0.4, 0.9, 1.5, 2.0])


def _args():
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, P)
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETAS[0])
    return ra.ode.fitzhugh_nagumo, W, x0, 0.0, T_MAX, N, interrogate_kramer, ra.ibm_init(T_MAX / N, P, np.array([0.1, 0.1]))


def _obs():
    rng = np.random.default_rng(7)
    D = np.zeros((len(TIMES), 2, 1, P))
    D[:, :, 0, 0] = 1.0
    return rng.standard_normal((len(TIMES), 2, 1)) * 0.5, D, np.full((len(TIMES), 2, 1, 1), 0.05)


def test_interleaved_calls_on_one_cached_plan():
    """dalton launches on basic's cached plan without touching its outputs: the only generation bump is the one of
    ``cached_plan``'s ``update()`` (which is why an unread Xt is stale after ANY call on the configuration, dalton included), and the
    plan still holds basic's moments, mode and layout.  dalton.solve_mv writes the outputs: update() and the launch bump."""
    y, D, Om = _obs()
    solve._plan_cache.clear()
    _, Xt = basic(None, *_args(), y[:, :, 0], TIMES, GaussianObsLoglik(0.2), theta=THETAS)
    want = np.asarray(Xt).copy()
    solve._plan_cache.clear()
    _, Xt = basic(None, *_args(), y[:, :, 0], TIMES, GaussianObsLoglik(0.2), theta=THETAS)
    (plan,) = solve._plan_cache.values()
    gen, layout = plan.generation, plan.layout
    ll = dmod.dalton(None, *_args(), y, TIMES, D, Om, theta=THETAS)
    assert ll.shape == (B,) and np.all(np.isfinite(ll))
    assert list(solve._plan_cache.values()) == [plan]               # the same plan served both
    assert plan.generation == gen + 1 and plan.last_mode == ra._lib.MODE_MV and plan.layout == layout
    np.testing.assert_array_equal(plan.state_host()[0], want)      # basic's posterior mean, bit for bit
    with pytest.raises(RuntimeError, match="earlier call"):
        np.asarray(Xt)
    dmod.solve_mv(None, *_args(), y, TIMES, D, Om, theta=THETAS)
    assert list(solve._plan_cache.values()) == [plan] and plan.generation == gen + 3
    assert np.max(np.abs(plan.state_host()[0] - want)) > 1e-6       # the data-adaptive mean now
    with pytest.raises(RuntimeError, match="earlier call"):
        np.asarray(Xt)


def test_upload_counts_of_alternating_callers(monkeypatch):
    """dalton, fenrir, dalton with unchanged observations on one cached plan: the values of three fresh calls, and 13 uploads --
    the plan's five inputs, dalton's four observation arrays, fenrir's four, and none for the second dalton (counted on the
    commit before the callers shared ``SolvePlan.staged``)."""
    y, D, Om = _obs()
    calls = [lambda: dmod.dalton(None, *_args(), y, TIMES, D, Om, theta=THETAS),
             lambda: fenrir(None, *_args(), y, TIMES, D, Om, theta=THETAS),
             lambda: dmod.dalton(None, *_args(), y, TIMES, D, Om, theta=THETAS)]
    fresh = []
    for call in calls:
        solve._plan_cache.clear()
        fresh.append(call())
    solve._plan_cache.clear()
    dev = ra.default_device()
    uploads = []
    to_device = dev.to_device
    monkeypatch.setattr(dev, "to_device", lambda host: uploads.append(np.shape(host)) or to_device(host))
    chain = [call() for call in calls]
    monkeypatch.undo()
    print("uploads:", len(uploads), uploads)
    assert len(solve._plan_cache) == 1
    for got, want in zip(chain, fresh):
        np.testing.assert_array_equal(got, want)
    assert len(uploads) == 13


def test_pathless_sim_logpost_allocates_no_path():
    """A path-less sim_logpost on a fresh plan (the fused tile route) allocates no x_state and x_host() raises; keep_path=True
    then stores the path of plan.sim with the same key."""
    ode, W, x0, t0, t1, n, _, prior = _args()
    g = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    rng = np.random.default_rng(3)
    obs, ind, upars = rng.standard_normal((5, 2)), np.array([0, 4, 9, 15, 20], dtype=np.int32), rng.standard_normal((B, 4))
    plan = ra.SolvePlan(ode, W, x0, t0, t1, n, g, prior, theta=THETAS)
    lp = sim_logpost(plan, 17, obs, ind, 0.2, upars=upars, n_prior=3).to_host()
    assert plan.x_state is None and plan.last_mode == ra._lib.MODE_SIM
    with pytest.raises(RuntimeError, match="path"):
        plan.x_host()
    kept = sim_logpost(plan, 17, obs, ind, 0.2, upars=upars, n_prior=3, keep_path=True).to_host()
    np.testing.assert_array_equal(kept, lp)
    ref = ra.SolvePlan(ode, W, x0, t0, t1, n, g, prior, theta=THETAS)
    ref.sim(17)
    np.testing.assert_array_equal(plan.x_host(), ref.x_host())
