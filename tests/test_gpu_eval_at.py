"""
GPU parity of ``rodeo_amd.solve_mv_at`` (the solver's posterior at arbitrary times; eval_at_kernel on the records of a
filter() and an mv() plan) against the NumPy restatement tests/eval_at_oracle.py, on every record layout: RK_LAYOUT_TILE3
(p = 3, and p = 2 by padding), RK_LAYOUT_TILE4 (p = 4), RK_LAYOUT_TILEP (p = 5) and batch-minor.

Queries on a node must equal ``solve_mv``'s own output bit for bit.  Queries between nodes are held to the bars of
tests/test_gpu_solver.py: |mean - oracle| <= 1e-9 absolute, var within 1e-9 of max|var|.
"""
import functools
import numpy as np
import pytest
from oracle import interrogations as oi, odes, scan
import eval_at_oracle as eo

pytestmark = pytest.mark.gpu

N = 40
# t_max, the first interval, a node, two times in one interval, t_min, the last interval, a node, 1e-3 dt from a node, a repeat
STEPS = np.array([N, 0.33, 17, 23.1, 23.7, 0, N - 0.4, 9, 25 + 1e-3, 23.1])
ON = np.array([True, False, True, False, False, True, False, True, False, False])

CASES = {
    "p3": dict(p=3),
    "p4": dict(p=4),
    "p5": dict(p=5),
    "p2-padded": dict(p=2),
    "p3-batch-minor": dict(p=3, batch_minor=True),
    "p3-B3": dict(p=3, B=3),
    "p3-B70": dict(p=3, B=70),                           # a ragged second wave
    "p4-B70": dict(p=4, B=70),
    "p3-B70-batch-minor": dict(p=3, B=70, batch_minor=True),
    "lorenz-p3": dict(p=3, ode="lorenz63"),
    "p3-batched-sigma": dict(p=3, B=5, batched_sigma=True),
}


def _problem(ra, p=3, B=None, ode="fitzhugh_nagumo", batched_sigma=False, batch_minor=False):
    rng = np.random.default_rng(11)
    if ode == "fitzhugh_nagumo":
        theta, x0v, t_max, d = np.array([0.2, 0.2, 3.0]), np.array([-1.0, 1.0]), 4.0, 2
    else:
        theta, x0v, t_max, d = np.array([28.0, 10.0, 8.0 / 3.0]), np.array([-12.0, -5.0, 38.0]), 0.4, 3
    if B is not None:
        theta = theta * np.exp(0.1 * rng.standard_normal((B, 3)))
        x0v = x0v + 0.1 * rng.standard_normal((B, d))
    dev_ode, ora_ode = getattr(ra.ode, ode), getattr(odes, ode)
    W, init = ra.utils.first_order_pad(dev_ode, d, p)
    sigma = np.full(d, 0.1)
    if batched_sigma:
        sigma = 0.05 + 0.1 * rng.random((B, d))
    return dict(ode=dev_ode, ora_ode=ora_ode, W=W, x0=init(x0v, 0.0, theta=theta), theta=theta, t_max=t_max,
                prior=ra.ibm_init(t_max / N, p, sigma), prior_at=lambda h: ra.ibm_init(h, p, sigma),
                t_eval=t_max * STEPS / N, kw=dict(batch_minor=True) if batch_minor else {})


@functools.lru_cache(maxsize=None)
def _results(name):
    """One device call, the grid values of the same route and the oracle's values, shared by the tests of a case."""
    import rodeo_amd as ra
    from rodeo_amd.interrogate import interrogate_kramer
    s = _problem(ra, **CASES[name])
    args = (s["W"], s["x0"], 0.0, s["t_max"], N)
    m, v = ra.solve_mv_at(None, s["ode"], *args, interrogate_kramer, s["prior"], s["t_eval"], s["prior_at"], theta=s["theta"],
                          **s["kw"])
    if s["kw"]:
        plan = ra.SolvePlan(s["ode"], *args, interrogate_kramer, s["prior"], theta=s["theta"], **s["kw"])
        plan.mv(None)
        gm, gv = plan.state_host()
    else:
        gm, gv = ra.solve_mv(None, s["ode"], *args, interrogate_kramer, s["prior"], theta=s["theta"])
    mo, vo = eo.solve_mv_at(None, s["ora_ode"], *args, oi.interrogate_kramer, s["prior"], s["t_eval"], s["prior_at"],
                            theta=s["theta"])
    for a in (m, v, gm, gv, mo, vo):
        a.setflags(write=False)
    return dict(m=m, v=v, gm=gm, gv=gv, mo=mo, vo=vo, batched=CASES[name].get("B") is not None)


@pytest.mark.parametrize("name", list(CASES))
def test_shapes_and_queries_on_nodes_equal_solve_mv_bit_for_bit(name):
    r = _results(name)
    c = CASES[name]
    d, p = (3 if c.get("ode") == "lorenz63" else 2), c["p"]
    lead = (c["B"],) if r["batched"] else ()
    assert r["m"].shape == lead + (len(STEPS), d, p) and r["v"].shape == lead + (len(STEPS), d, p, p)
    nodes = np.rint(STEPS[ON]).astype(int)
    assert np.array_equal(r["m"][..., ON, :, :], r["gm"][..., nodes, :, :])
    assert np.array_equal(r["v"][..., ON, :, :, :], r["gv"][..., nodes, :, :, :])
    assert np.all(np.isfinite(r["m"])) and np.all(np.isfinite(r["v"]))
    # the repeat gives the same bits as its first occurrence
    assert np.array_equal(r["m"][..., 9, :, :], r["m"][..., 3, :, :]) and np.array_equal(r["v"][..., 9, :, :, :], r["v"][..., 3, :, :, :])


@pytest.mark.parametrize("name", list(CASES))
def test_queries_between_nodes_against_the_oracle(name):
    r = _results(name)
    off = ~ON
    em = np.max(np.abs(r["m"][..., off, :, :] - r["mo"][..., off, :, :]))
    ev = np.max(np.abs(r["v"][..., off, :, :, :] - r["vo"][..., off, :, :, :])) / np.max(np.abs(r["vo"]))
    # (the on-node values are solve_mv's: the same bars, as in tests/test_gpu_solver.py)
    en = np.max(np.abs(r["m"][..., ON, :, :] - r["mo"][..., ON, :, :]))
    print(f"eval_at {name}: off-node |mean - oracle| = {em:.3e}, |var - oracle| / max|var| = {ev:.3e}; on-node mean {en:.3e}")
    assert em <= 1e-9 and ev <= 1e-9, (name, em, ev)


def test_two_calls_give_identical_bits():
    import rodeo_amd as ra
    from rodeo_amd.interrogate import interrogate_kramer
    s = _problem(ra, p=3, B=70)
    out = [ra.solve_mv_at(None, s["ode"], s["W"], s["x0"], 0.0, s["t_max"], N, interrogate_kramer, s["prior"], s["t_eval"],
                          s["prior_at"], theta=s["theta"]) for _ in range(2)]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    r = _results("p3-B70")
    assert np.array_equal(out[0][0], r["m"]) and np.array_equal(out[0][1], r["v"])


@pytest.mark.parametrize("pair", [("p3", "p3-batch-minor"), ("p3-B70", "p3-B70-batch-minor")])
def test_tile_route_and_batch_minor_route_agree(pair):
    a, b = _results(pair[0]), _results(pair[1])
    em = np.max(np.abs(a["m"] - b["m"]))
    ev = np.max(np.abs(a["v"] - b["v"])) / np.max(np.abs(a["v"]))
    print(f"eval_at {pair}: |mean tile - mean batch-minor| = {em:.3e}, var {ev:.3e} of max|var|")
    assert em <= 1e-9 and ev <= 1e-9


def test_chkrebtii_sees_the_same_draws_in_both_plans():
    """An integer key: the filter() plan and the mv() plan draw the same interrogation points (the counter RNG keys draws by
    trajectory and step), so the on-node values are solve_mv's with that key."""
    import rodeo_amd as ra
    from rodeo_amd.interrogate import interrogate_chkrebtii
    s = _problem(ra, p=3, B=3)
    itg = functools.partial(interrogate_chkrebtii, kalman_type="standard")
    args = (s["W"], s["x0"], 0.0, s["t_max"], N)
    m, v = ra.solve_mv_at(7, s["ode"], *args, itg, s["prior"], s["t_eval"], s["prior_at"], theta=s["theta"])
    gm, gv = ra.solve_mv(7, s["ode"], *args, itg, s["prior"], theta=s["theta"])
    nodes = np.rint(STEPS[ON]).astype(int)
    assert np.array_equal(m[:, ON], gm[:, nodes]) and np.array_equal(v[:, ON], gv[:, nodes])
    other = ra.solve_mv(8, s["ode"], *args, itg, s["prior"], theta=s["theta"])[0]
    # the key does enter, at every node after t_min (node 0 is ode_init whatever the key)
    assert all(not np.array_equal(other[:, n], gm[:, n]) for n in nodes if n > 0)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
