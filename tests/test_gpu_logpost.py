"""
The device log-posterior reductions at every shape: the sampler that adds the observation terms itself
(bwd_sim_tile3_kernel<true>, rk_solve_sim_logpost / inference.sim_logpost) and the stand-alone reduction over a path or a mean
(gauss_logpost_kernel, rk_gauss_obs_logpost / inference.gauss_obs_logpost), against tests/logpost_oracle.py -- the formula in
longdouble -- evaluated on the SAME path, which a separate plan's ``sim(key); x_host()`` provides (bwd_sim_tile3_kernel<false>,
the instantiation that stores the path).  Bound of every such comparison (logpost_oracle.derived_bound):

    |dev - ref| <= 8 * n_terms * 2^-52 * sum|term|,    n_terms = n_obs * d + n_prior,   sum|term| from the reference.

Paths are tied to the oracle's solve_sim (shared Philox stream) at the project's 1e-7, means to its solve_mv through the
log-posterior at rtol = atol = 1e-7.  Each test prints the share of the bound it used (pytest -s).
"""
import functools
import numpy as np
import pytest
from oracle import scan, odes, interrogations as oi
from test_gpu_user_rhs import _oracle_ode
import logpost_oracle as lo

pytestmark = pytest.mark.gpu
SD = np.sqrt(0.005)
PRIOR_SD = 10.0
USED = {}                                             # family -> largest |dev - ref| / bound seen


@pytest.fixture(scope="module")
def ra():
    import rodeo_amd
    yield rodeo_amd
    print("\nshare of the derived bound used, per family:", {k: round(v, 4) for k, v in sorted(USED.items())})


def two_fitz(X, t, **params):
    """Two FitzHugh-Nagumo pairs with a weak linear coupling of the voltages: four blocks."""
    a, b, c, eps = params["theta"]
    V1, R1, V2, R2 = X[:, 0]
    return np.array([[c * (V1 - V1 * V1 * V1 / 3 + R1) + eps * (V2 - V1)], [-1 / c * (V1 - a + b * R1)],
                     [c * (V2 - V2 * V2 * V2 / 3 + R2) + eps * (V1 - V2)], [-1 / c * (V2 - a + b * R2)]])


@pytest.fixture(scope="module")
def systems(ra):
    """Device ODE, oracle ODE, nominal parameters, nominal initial values, step size and prior scale per n_block; the traced
    four-block function is registered (and compiled) once for the module."""
    return {
        1: dict(ode=ra.ode.higher_order, o=odes.higher_order, theta=None, x0=np.array([-1.0]), dt=0.05, sigma=0.01),
        2: dict(ode=ra.ode.fitzhugh_nagumo, o=odes.fitzhugh_nagumo, theta=np.array([0.2, 0.2, 3.0]), x0=np.array([-1.0, 1.0]),
                dt=0.05, sigma=0.1),
        3: dict(ode=ra.ode.lorenz63, o=odes.lorenz63, theta=np.array([28.0, 10.0, 8.0 / 3.0]), x0=np.array([-12.0, -5.0, 38.0]),
                dt=5e-3, sigma=5e7),
        4: dict(ode=ra.ode.from_python(two_fitz, 4, theta=4), o=_oracle_ode("two_fitz", two_fitz, 4),
                theta=np.array([0.2, 0.2, 3.0, 0.05]), x0=np.array([-1.0, 1.0, -0.8, 0.9]), dt=0.05, sigma=0.1),
    }


def _itg(ra, name):
    g, o = getattr(ra.interrogate, "interrogate_" + name), getattr(oi, "interrogate_" + name)
    if name == "chkrebtii":
        g, o = functools.partial(g, kalman_type="standard"), functools.partial(o, kalman_type="standard")
    return g, o


def _problem(ra, systems, d, B, N, p=3, seed=0, batched=True, per_draw_sigma=False, dt=None):
    """Arguments of a solve: B trajectories with their own parameters and initial values (``batched=False``: one, unbatched)."""
    s = systems[d]
    rng = np.random.default_rng(1000 * d + 10 * B + seed)
    dt = s["dt"] if dt is None else dt
    lead = (B,) if batched else ()
    params = {}
    if s["theta"] is not None:
        params["theta"] = s["theta"] * np.exp(0.05 * rng.standard_normal(lead + s["theta"].shape))
    x0v = s["x0"] + 0.05 * rng.standard_normal(lead + s["x0"].shape)
    if d == 1:                                          # x'' = sin 2t - x with W = [0, 0, 1] (docs/examples/higher_order.md)
        W = np.zeros((1, 1, p)); W[0, 0, 2] = 1.0
        x0 = np.zeros(lead + (1, p)); x0[..., 0, 0] = x0v[..., 0]; x0[..., 0, 2] = -x0v[..., 0]
    else:
        W, init = ra.utils.first_order_pad(s["ode"], d, p)
        x0 = init(x0v, 0.0, **params)
    sigma = np.full(d, s["sigma"])
    if per_draw_sigma:
        sigma = sigma * np.exp(0.1 * rng.standard_normal((B, d)))
    return dict(ode=s["ode"], o=s["o"], W=W, x0=x0, t_max=dt * N, N=N, prior=ra.ibm_init(dt, p, sigma), params=params, d=d, B=B)


def _plan(ra, pr, g, sl=None, **kw):
    x0, prior, params = pr["x0"], pr["prior"], pr["params"]
    if sl is not None:
        x0 = x0[sl]
        params = {k: v[sl] for k, v in params.items()}
        prior = tuple(a[sl] if a.ndim == 4 else a for a in prior)
    return ra.SolvePlan(pr["ode"], pr["W"], x0, 0.0, pr["t_max"], pr["N"], g, prior, **kw, **params)


def _paths(plan):
    """(B, N+1, d) zeroth derivative of the plan's sample path."""
    x = plan.x_host()
    return (x if plan.batched else x[None])[..., 0]


def _means(plan):
    m = plan.state_host()[0]
    return (m if plan.batched else m[None])[..., 0]


def _data(seed, n_obs, d, B, k=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_obs, d)), rng.standard_normal((B, k))


def _agree(family, dev, x0, obs, ind, upars=None, n_prior=None):
    """Device values against the longdouble reference on the path / mean x0 at the derived bound."""
    dev = np.asarray(dev, dtype=np.float64)
    ref, sab = lo.gauss_logpost_ref(x0, obs, ind, SD, upars, n_prior, PRIOR_SD)
    bound = lo.derived_bound(len(ind), x0.shape[2], sab, upars, n_prior)
    err = np.abs(dev - ref)
    used = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    USED[family] = max(USED.get(family, 0.0), used)
    print(f"\n[{family}] n_terms = {lo.n_terms(len(ind), x0.shape[2], upars, n_prior)}  max |dev - ref| = {err.max():.3e}  "
          f"bound = {bound.min():.3e}  share of the bound = {used:.3f}  (family so far {USED[family]:.3f})")
    assert dev.shape == ref.shape and np.all(np.isfinite(dev))
    assert np.all(err <= bound), (family, dev, ref, err, bound)
    return ref


def _fused(ra, plan, key, obs, ind, upars=None, n_prior=None, expect_fused=True, **kw):
    """sim_logpost with the checks that belong to every call: _fused_supported mirrors what happened to x_state."""
    from rodeo_amd.inference import logpost
    had_path = plan.x_state is not None
    val = logpost.sim_logpost(plan, key, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=n_prior, **kw).to_host()
    assert logpost._fused_supported(plan, len(ind)) == expect_fused
    if not had_path and not kw.get("keep_path"):
        assert (plan.x_state is None) == expect_fused             # fused: no path buffer; two kernels: one was allocated
    return val


def _ind(N, n_obs, seed):
    """Sorted indices with both ends of the grid and, when there are more than the grid has nodes, repeats."""
    rng = np.random.default_rng(seed)
    inner = rng.integers(0, N + 1, size=max(n_obs - 2, 0))
    return np.sort(np.concatenate([[0, N][:n_obs], inner])).astype(np.int32)


# ---- the fused sampler ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chkrebtii", "rodeo"])
@pytest.mark.parametrize("B", [1, 3, 5, 9])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_fused_shapes(ra, systems, d, B, name):
    """n_block 1 / 2 / 4 (each its own shuffle pattern over a trajectory's tiles) times batches whose last wave is full, half
    full or holds one tile (tile counts 1, 2, 3, 5, 6, 9, 10, 12, 18, 20, 36), N = 33: two full chunks and a step.  For B = 5 the
    path is tied to the oracle's sampler as well."""
    from rodeo_amd import _lib
    g, o = _itg(ra, name)
    N = 33
    pr = _problem(ra, systems, d, B, N)
    obs, upars = _data(10 * d + B, 7, d, B)
    ind = _ind(N, 7, d + B)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(42)
    assert ref_plan.layout == _lib.LAYOUT_TILE3            # (n_block = 4: the traced function got the tile route from hiprtc)
    x = ref_plan.x_host()
    plan = _plan(ra, pr, g)
    val = _fused(ra, plan, 42, obs, ind, upars, 5)
    assert plan.x_state is None and plan.layout == _lib.LAYOUT_TILE3
    _agree(f"fused shapes d={d}", val, x[..., 0], obs, ind, upars, 5)
    if B == 5:
        xo = scan.solve_sim(42, pr["o"], pr["W"], pr["x0"], 0.0, pr["t_max"], N, o, pr["prior"], **pr["params"])
        assert np.max(np.abs(x - xo)) < 1e-7


@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 32, 33, 49])
def test_fused_horizons_every_index_observed(ra, systems, N):
    """No full chunk, exactly full chunks, full chunks and a partial one -- with EVERY grid index 0 .. N observed once, so that
    a dropped or doubled term at a chunk boundary (each about 0.5 (delta / 0.07)^2) cannot hide."""
    g, _ = _itg(ra, "chkrebtii")
    d, B = 2, 5
    pr = _problem(ra, systems, d, B, N)
    obs, upars = _data(N, N + 1, d, B)
    ind = np.arange(N + 1, dtype=np.int32)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(7)
    plan = _plan(ra, pr, g)
    val = _fused(ra, plan, 7, obs, ind, upars, 5)
    assert plan.x_state is None
    _agree("fused horizons", val, _paths(ref_plan), obs, ind, upars, 5)


@pytest.fixture(scope="module")
def placement(ra, systems):
    """N = 49, d = 2, B = 3: the path of key 11 (a plan that stores it) and a plan for the path-less calls."""
    g, _ = _itg(ra, "chkrebtii")
    pr = _problem(ra, systems, 2, 3, 49)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(11)
    return _paths(ref_plan), _plan(ra, pr, g)


N49 = 49
PLACEMENTS = {
    "first": [0], "last": [N49], "16-17": [16, 17], "32-33": [32, 33], "1": [1], "N-16,N-15": [N49 - 16, N49 - 15],
    "five-times": [20] * 5, "five-times-at-hand-off": [33] * 5, "five-times-at-0": [0] * 5,
}


@pytest.mark.parametrize("where", list(PLACEMENTS))
def test_fused_placements(ra, placement, where):
    """Observations on the two sides of every hand-off between chunks (N = 49: steps 49 .. 34, 33 .. 18, 17 .. 2, the partial
    chunk's step 1, index 0 from the initial value), single ones at the ends, a repeated index."""
    x0, plan = placement
    ind = np.array(PLACEMENTS[where], dtype=np.int32)
    obs, upars = _data(len(where), len(ind), 2, 3)
    val = _fused(ra, plan, 11, obs, ind, upars, 5)
    _agree("fused placements", val, x0, obs, ind, upars, 5)
    val = _fused(ra, plan, 11, obs, ind)                                    # ... and without a prior
    _agree("fused placements", val, x0, obs, ind)


def test_fused_prior_only_and_prior_sizes(ra, placement):
    x0, plan = placement
    none = np.zeros((0, 2))
    ind0 = np.zeros(0, dtype=np.int32)
    obs, upars = _data(5, 4, 2, 3)
    ind = np.array([3, 17, 18, 40], dtype=np.int32)
    val = _fused(ra, plan, 11, none, ind0, upars)                           # n_obs = 0: the prior alone, all seven
    _agree("fused prior", val, x0, none, ind0, upars)
    val = _fused(ra, plan, 11, none, ind0)                                  # nothing at all: exact zeros
    assert val.shape == (3,) and np.all(val == 0.0) and not np.any(np.signbit(val))
    val = _fused(ra, plan, 11, obs, ind, upars, 0)                          # n_prior = 0
    ref0 = _agree("fused prior", val, x0, obs, ind, upars, 0)
    np.testing.assert_array_equal(ref0, lo.gauss_logpost_ref(x0, obs, ind, SD)[0])
    val3 = _fused(ra, plan, 11, obs, ind, upars, 3)                         # n_prior smaller than upars.shape[1]
    _agree("fused prior", val3, x0, obs, ind, upars, 3)
    val7 = _fused(ra, plan, 11, obs, ind, upars)
    _agree("fused prior", val7, x0, obs, ind, upars)
    assert np.all(val3 != val7) and np.all(val3 != val)


@pytest.mark.parametrize("d,n_obs,fused", [(2, 512, True), (2, 513, False), (4, 256, True), (4, 257, False)])
def test_route_limits(ra, systems, d, n_obs, fused):
    """n_obs <= 512 and n_obs * d <= 1024: at the limit the sampler reduces and no path exists, one past it the two kernels run
    and the plan allocates x_state; logpost._fused_supported says the same; both sides agree with the reference."""
    g, _ = _itg(ra, "chkrebtii")
    N, B = 600, 3
    pr = _problem(ra, systems, d, B, N, dt=0.005)
    obs, upars = _data(n_obs, n_obs, d, B)
    ind = np.sort(np.random.default_rng(n_obs).permutation(N + 1)[:n_obs]).astype(np.int32)      # distinct
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(5)
    plan = _plan(ra, pr, g)
    val = _fused(ra, plan, 5, obs, ind, upars, 5, expect_fused=fused)
    assert (plan.x_state is None) == fused
    _agree("route limits", val, _paths(ref_plan), obs, ind, upars, 5)
    if not fused:
        np.testing.assert_array_equal(plan.x_host(), ref_plan.x_host())


@pytest.mark.parametrize("d,p", [(3, 3), (2, 4)])
def test_never_fused_configurations(ra, systems, d, p):
    """Three blocks (lorenz63: a trajectory's tiles do not fill a power-of-two group of a wave) and n_bstate = 4: sampler, then
    the reduction kernel on its path, in one call."""
    g, _ = _itg(ra, "rodeo" if d == 3 else "chkrebtii")     # (lorenz63 at its prior scale 5e7: chkrebtii's forward draws leave fp64)
    N, B = 20, 5
    pr = _problem(ra, systems, d, B, N, p=p)
    obs, upars = _data(d + p, 6, d, B)
    obs = obs + systems[d]["x0"]
    ind = _ind(N, 6, 3)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(9)
    plan = _plan(ra, pr, g)
    val = _fused(ra, plan, 9, obs, ind, upars, 5, expect_fused=False)
    assert plan.x_state is not None
    _agree("two-kernel route", val, _paths(ref_plan), obs, ind, upars, 5)
    np.testing.assert_array_equal(plan.x_host(), ref_plan.x_host())


def test_fused_sharding_is_bit_exact(ra, systems):
    """Trajectories 4 .. 7 of 12 solved alone with traj_offset = 4: the full batch's values, bit for bit."""
    g, _ = _itg(ra, "chkrebtii")
    N, B = 33, 12
    pr = _problem(ra, systems, 2, B, N)
    obs, upars = _data(1, 7, 2, B)
    ind = _ind(N, 7, 1)
    full = _fused(ra, _plan(ra, pr, g), 7, obs, ind, upars, 5)
    shard = _fused(ra, _plan(ra, pr, g, sl=slice(4, 8), traj_offset=4), 7, obs, ind, upars[4:8], 5)
    np.testing.assert_array_equal(shard, full[4:8])
    other = _fused(ra, _plan(ra, pr, g, sl=slice(4, 8), traj_offset=0), 7, obs, ind, upars[4:8], 5)
    assert np.all(other != full[4:8])                                       # the offset selects the draws


def test_fused_per_draw_prior_scale(ra, systems):
    """A (B, d, p, p) prior (sigma per draw, the pseudo-marginal sampler's case) with an odd batch."""
    g, o = _itg(ra, "chkrebtii")
    N, B = 33, 5
    pr = _problem(ra, systems, 2, B, N, per_draw_sigma=True)
    assert pr["prior"][1].ndim == 4
    obs, upars = _data(2, 7, 2, B)
    ind = _ind(N, 7, 2)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(3)
    x = ref_plan.x_host()
    plan = _plan(ra, pr, g)
    val = _fused(ra, plan, 3, obs, ind, upars, 5)
    _agree("fused per-draw sigma", val, x[..., 0], obs, ind, upars, 5)
    xo = scan.solve_sim(3, pr["o"], pr["W"], pr["x0"], 0.0, pr["t_max"], N, o, pr["prior"], **pr["params"])
    assert np.max(np.abs(x - xo)) < 1e-7


def test_fused_ownership_and_determinism(ra, systems):
    """One key, identical bits; the fifth result reuses the first call's buffer and no other (the ring of the docstring);
    keep_path = True gives the path-less call's bits and plan.sim's path."""
    from rodeo_amd.inference import sim_logpost
    g, _ = _itg(ra, "chkrebtii")
    N, B = 33, 5
    pr = _problem(ra, systems, 2, B, N)
    obs, upars = _data(3, 7, 2, B)
    ind = _ind(N, 7, 3)
    plan = _plan(ra, pr, g)
    a = _fused(ra, plan, 21, obs, ind, upars, 5)
    b = _fused(ra, plan, 21, obs, ind, upars, 5)
    np.testing.assert_array_equal(a, b)
    want = [_fused(ra, _plan(ra, pr, g), 30 + k, obs, ind, upars, 5) for k in range(5)]
    plan = _plan(ra, pr, g)
    ring = [sim_logpost(plan, 30 + k, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=5) for k in range(5)]
    assert ring[4].ptr.value == ring[0].ptr.value and len({r.ptr.value for r in ring[:4]}) == 4
    for k in (1, 2, 3, 4):
        np.testing.assert_array_equal(ring[k].to_host(), want[k])
    np.testing.assert_array_equal(ring[0].to_host(), want[4])              # overwritten by the fifth call, as documented
    assert len({w.tobytes() for w in want}) == 5
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(21)
    plan = _plan(ra, pr, g)
    kept = _fused(ra, plan, 21, obs, ind, upars, 5, keep_path=True)
    np.testing.assert_array_equal(kept, a)
    np.testing.assert_array_equal(plan.x_host(), ref_plan.x_host())


# ---- the two defects ------------------------------------------------------------------------------------------------------

def test_unsorted_indices(ra, systems):
    """obs_ind in any order, as the reference's Xt[obs_ind]: the fused sampler (which walks ascending indices from the end and
    used to drop 5 and everything before it for [5, 2, 8, ...]), the same call with the path kept, and the stand-alone
    reduction on that path all give the reference's value; the first two the same bits."""
    from rodeo_amd.inference import gauss_obs_logpost
    g, _ = _itg(ra, "chkrebtii")
    N, B = 33, 5
    pr = _problem(ra, systems, 2, B, N)
    ind = np.array([5, 2, 8, 2, 33, 0], dtype=np.int32)
    obs, upars = _data(4, 6, 2, B)
    ref_plan = _plan(ra, pr, g)
    ref_plan.sim(13)
    x0 = _paths(ref_plan)
    plan = _plan(ra, pr, g)
    fused = _fused(ra, plan, 13, obs, ind, upars, 5)
    assert plan.x_state is None
    _agree("unsorted indices", fused, x0, obs, ind, upars, 5)
    kept = _fused(ra, plan, 13, obs, ind, upars, 5, keep_path=True)
    _agree("unsorted indices", kept, x0, obs, ind, upars, 5)
    np.testing.assert_array_equal(fused, kept)
    alone = gauss_obs_logpost(plan, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=5, which="x").to_host()
    _agree("unsorted indices", alone, x0, obs, ind, upars, 5)
    np.testing.assert_array_equal(obs, _data(4, 6, 2, B)[0])                # the caller's arrays are left alone
    np.testing.assert_array_equal(ind, [5, 2, 8, 2, 33, 0])


def test_pathless_call_invalidates_the_path(ra, systems):
    """plan.sim(1), then a path-less sim_logpost(plan, 2): x_state still holds key 1's path and must not be handed out."""
    from rodeo_amd.inference import gauss_obs_logpost
    g, _ = _itg(ra, "chkrebtii")
    N, B = 33, 5
    pr = _problem(ra, systems, 2, B, N)
    obs, upars = _data(5, 7, 2, B)
    ind = _ind(N, 7, 5)
    plan = _plan(ra, pr, g)
    plan.sim(1)
    x1 = plan.x_host().copy()
    gauss_obs_logpost(plan, obs, ind, SD, which="auto")
    lp2 = _fused(ra, plan, 2, obs, ind, upars, 5)
    with pytest.raises(RuntimeError, match="path"):
        plan.x_host()
    with pytest.raises(RuntimeError, match="path"):
        gauss_obs_logpost(plan, obs, ind, SD, which="x")
    with pytest.raises(RuntimeError, match="path"):
        gauss_obs_logpost(plan, obs, ind, SD, which="auto")
    kept = _fused(ra, plan, 2, obs, ind, upars, 5, keep_path=True)
    np.testing.assert_array_equal(kept, lp2)
    fresh = _plan(ra, pr, g)
    fresh.sim(2)
    x2 = fresh.x_host()
    np.testing.assert_array_equal(plan.x_host(), x2)
    assert np.max(np.abs(x2 - x1)) > 1e-6
    _agree("stale path", gauss_obs_logpost(plan, obs, ind, SD, which="auto").to_host(), x2[..., 0], obs, ind)
    _fused(ra, plan, 3, obs, ind, upars, 5)                                 # stale again ...
    with pytest.raises(RuntimeError, match="path"):
        plan.x_host()
    plan.sim(2)                                                             # ... and valid after a plain sim
    np.testing.assert_array_equal(plan.x_host(), x2)
    never = _plan(ra, pr, g)                                                # a plan that never stored a path
    _fused(ra, never, 2, obs, ind, upars, 5)
    with pytest.raises(RuntimeError, match="path"):
        never.x_host()
    with pytest.raises(RuntimeError, match="path"):
        gauss_obs_logpost(never, obs, ind, SD, which="auto")


# ---- the stand-alone reduction ----------------------------------------------------------------------------------------------

LAYOUTS = {
    # name: (n_block, n_bstate, SolvePlan keywords, batched, expected layout of mv() or None, step size)
    "tile3-d1": (1, 3, {}, True, "LAYOUT_TILE3", None),
    "tile3-d2": (2, 3, {}, True, "LAYOUT_TILE3", None),
    "tile3-d3": (3, 3, {}, True, "LAYOUT_TILE3", None),
    "tile4": (2, 4, {}, True, "LAYOUT_TILE4", None),
    "tilep-5": (2, 5, {}, True, "LAYOUT_TILEP", 0.01),
    "tilep-8": (2, 8, {}, True, "LAYOUT_TILEP", 0.01),
    "batch-minor": (2, 3, {"batch_minor": True}, True, "LAYOUT_BATCH_MINOR", None),
    "unbatched": (2, 3, {}, False, None, None),
}


@pytest.mark.parametrize("layout,B", [(k, B) for k, v in LAYOUTS.items() for B in ((1, 5) if v[3] else (1,))])
def test_standalone_reduction_layouts(ra, systems, layout, B):
    """gauss_obs_logpost over the mean of mv() in every record layout, over the path of sim() (which = "x" and "auto") and
    over the filtered mean the sampler's forward pass left (which = "mean" after a sim); 40 observations at n_block = 2: the 80
    terms take the 64 lanes' stride loop round a second time.  B = 5: the mean is tied to the oracle's solve_mv."""
    from rodeo_amd import _lib
    from rodeo_amd.inference import gauss_obs_logpost
    d, p, kw, batched, lay, dt = LAYOUTS[layout]
    g, o = _itg(ra, "rodeo")
    N, n_obs = 33, 40
    pr = _problem(ra, systems, d, B, N, p=p, batched=batched, dt=dt)
    obs, upars = _data(p + B, n_obs, d, B)
    obs = obs + systems[d]["x0"]
    ind = _ind(N, n_obs, p)
    assert ind[0] == 0 and ind[-1] == N
    plan = _plan(ra, pr, g, **kw)
    plan.mv(None)
    if lay is not None:
        assert plan.layout == getattr(_lib, lay)
    fam = "stand-alone " + layout
    m0 = _means(plan)
    val = gauss_obs_logpost(plan, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=5).to_host()
    ref = _agree(fam, val, m0, obs, ind, upars, 5)
    _agree(fam, gauss_obs_logpost(plan, obs, ind, SD, which="mean").to_host(), m0, obs, ind)
    _agree(fam, gauss_obs_logpost(plan, obs, ind, SD, upars=upars, n_prior=0).to_host(), m0, obs, ind, upars, 0)
    if B == 5 or not batched:
        mo, _ = scan.solve_mv(None, pr["o"], pr["W"], pr["x0"], 0.0, pr["t_max"], N, o, pr["prior"], **pr["params"])
        mo = (mo if batched else mo[None])[..., 0]
        np.testing.assert_allclose(val, lo.gauss_logpost_ref(mo, obs, ind, SD, upars, 5, PRIOR_SD)[0], rtol=1e-7, atol=1e-7)
    plan.sim(17)
    x0 = _paths(plan)
    for which in ("x", "auto"):
        val = gauss_obs_logpost(plan, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=5, which=which).to_host()
        refx = _agree(fam, val, x0, obs, ind, upars, 5)
    assert np.all(refx != ref)
    val = gauss_obs_logpost(plan, obs, ind, SD, upars=upars, prior_sd=PRIOR_SD, n_prior=5, which="mean").to_host()
    _agree(fam, val, _means(plan), obs, ind, upars, 5)
    for bad in (np.where(np.arange(n_obs) == 3, N + 1, ind), np.where(np.arange(n_obs) == 0, -1, ind)):
        with pytest.raises(ValueError):
            gauss_obs_logpost(plan, obs, bad, SD)
