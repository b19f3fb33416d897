"""
Pins tests/fenrir_grad_oracle.py (the NumPy restatement of ``fenrir_grid_jvp``'s tangent recursion), without a GPU, by
tests/test_oracle_dalton_grad.py's scheme.

(a) Finite differences.  For every case of tests/fenrir_grad_cases.py and every direction that is not zero, the restated
    derivative is compared with Richardson-extrapolated central differences of the UNTOUCHED value restatement
    ``fenrir_grid_oracle.fenrir_grid``: D(h) = (f(+h) - f(-h)) / 2h, R(h) = (4 D(h/2) - D(h)) / 3, once from the steps (h, h/2) and
    once from (2h, h), h = 1e-4 max(1, |theta_j|) for a unit theta direction and 1e-4 for any other (a mixed direction's largest
    entry is 1).  Bar per case: 10 x the disagreement of the two Richardson estimates, relative to max |grad| of the trajectory
    -- the factor covers the difference quotient's own truncation and rounding -- and, as a condition on the case, that bar may
    not exceed 1e-6.
(b) Judgeability: no y forecast variance lies in (1e-9, 1e-7), at the case's parameters or at any perturbed point; the restated
    gradient's own move under R (1 + 1e-15) is below a tenth of the device bar (1e-7 max |grad| per trajectory).
(c) The restated value is ``fenrir_grid_oracle.fenrir_grid``'s to 1e-12 (two codes, one formula).
(d) ``init_jac``: the total derivative (theta direction + J's column as the ode_init direction) equals differences of the value
    restatement with ``ode_init`` rebuilt from theta.
"""
import functools
import numpy as np
import pytest
import rodeo_amd as ra
import dalton_grid_cases as dc
import fenrir_grid_cases as fc
import fenrir_grad_cases as fgc
import fenrir_grad_oracle as fgr
import grid_cases as gc

DEVICE_BAR = 1e-7                                                    # tests/test_gpu_fenrir_grad.py: of max |grad| per trajectory


def _step(g, k):
    """The difference step of direction k: 1e-4 max(1, |theta_j|) for a unit theta direction, 1e-4 for any other direction."""
    dth = np.zeros(1) if g["dtheta"] is None else g["dtheta"][..., k, :]
    dx = np.zeros((1, 1)) if g["dx0"] is None else g["dx0"][..., k, :, :]
    if dth.ndim == 1 and np.count_nonzero(dth) == 1 and not np.any(dx):
        return 1e-4 * max(1.0, float(np.max(np.abs(g.theta[..., int(np.flatnonzero(dth)[0])]))))
    return 1e-4


@functools.lru_cache(maxsize=None)
def _differences(g):
    """Per case, once: the two Richardson estimates (B, K) (zero directions: 0) and every y forecast variance met on the way."""
    B = 1 if g["B"] is None else g["B"]
    r1, r2, seen = np.zeros((B, g["K"])), np.zeros((B, g["K"])), []
    zeros = fgc.zero_directions(g)
    g.value_case().restate_value(forecast_vars=seen)
    for k in range(g["K"]):
        if k in zeros:
            continue
        h = _step(g, k)
        f = {e: np.atleast_1d(g.moved(k, e * h).restate_value(forecast_vars=seen)) for e in (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)}
        D = {e: (f[e] - f[-e]) / (2 * e * h) for e in (0.5, 1.0, 2.0)}
        r1[:, k] = (4 * D[0.5] - D[1.0]) / 3
        r2[:, k] = (4 * D[1.0] - D[2.0]) / 3
    return r1, r2, np.concatenate([np.ravel(w) for w in seen])


@functools.lru_cache(maxsize=None)
def _restated(g):
    return g.restate()


CASES = fgc.cases()
IDS = [g["label"] for g in CASES]


def test_the_case_list_is_the_issue_s():
    assert len(CASES) == 22
    items = {(1 if g["B"] is None else g["B"], g["K"]) for g in CASES}
    assert {(1, 1), (3, 5), (11, 3), (33, 1), (13, 5)} <= items
    assert sum(1 for g in CASES if g["case"]["nodes"] and g["case"]["nodes"][0] == 0) == 3


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_gradient_equals_richardson_differences_of_the_value_restatement(g):
    _, dval = _restated(g)
    r1, r2, _ = _differences(g)
    scale = np.max(np.abs(dval), axis=1, keepdims=True)
    disagreement = float(np.max(np.abs(r1 - r2) / scale))
    bar = 10.0 * disagreement
    err = float(np.max(np.abs(dval - r1) / scale))
    print(f"{g['label']}: max|grad| {scale.min():.3e} .. {scale.max():.3e}; Richardson estimates disagree by {disagreement:.3e}, bar {bar:.3e}; "
          f"|restated - differences| = {err:.3e} of max|grad|")
    assert bar <= 1e-6, bar
    assert err <= bar, (err, bar)
    for k in fgc.zero_directions(g):
        assert np.all(dval[:, k] == 0.0)


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_no_y_forecast_variance_near_the_threshold_at_any_evaluated_point(g):
    s = _differences(g)[2]
    inside = int(np.sum((s > 1e-9) & (s < 1e-7)))
    print(f"{g['label']}: y forecast variances {s.min():.3e} .. {s.max():.3e} over the case and its perturbed points, {inside} inside (1e-9, 1e-7)")
    assert inside == 0
    own = []
    g.restate(forecast_vars=own)                                     # the tangent restatement meets the same variances
    own = np.asarray(own)
    assert int(np.sum((own > 1e-9) & (own < 1e-7))) == 0


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_gradient_is_well_conditioned(g):
    _, a = _restated(g)
    _, b = g.restate(1.0 + 1e-15)
    move = float(np.max(np.abs(a - b) / np.max(np.abs(a), axis=1, keepdims=True)))
    print(f"{g['label']}: the restated gradient moves by {move:.3e} of max|grad| under R (1 + 1e-15) (a tenth of the device bar: {0.1 * DEVICE_BAR:.0e})")
    assert move < 0.1 * DEVICE_BAR


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_value_is_the_value_restatement_s(g):
    val, _ = _restated(g)
    ref = np.atleast_1d(g.value_case().restate_value())
    assert np.max(np.abs(val - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-12


def test_total_derivative_through_init_jac():
    """The quick start's initial state x0 = init(v0, 0, theta) depends on theta: d/dtheta_j of the value with x0 rebuilt equals the
    derivative along (e_j, d x0 / d theta_j)."""
    c = dc.make(gc.fhn(3, "kramer", "distinct"))
    theta, v0 = gc.THETA, np.array([-1.0, 1.0])
    _, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, 3)
    J = fgr.fhn_init_jac(v0, theta, 3)                               # (d, p, 3)
    g = fgc.FGCase(case=c, dtheta=np.eye(3), dx0=np.moveaxis(J, -1, 0), K=3, B=None, label="init_jac")
    _, dval = g.restate()
    _, partial = fgc.FGCase(case=c, dtheta=np.eye(3), dx0=None, K=3, B=None, label="partial").restate()

    def f(th):
        m = fc.FCase(c)
        m.update(params=dict(theta=th), x0=init(v0, 0.0, theta=th))
        return m.restate_value()
    est = np.zeros((2, 3))
    for j in range(3):
        h = 1e-4 * max(1.0, abs(theta[j]))
        e = np.eye(3)[j] * h
        D = {s: (f(theta + s * e) - f(theta - s * e)) / (2 * s * h) for s in (0.5, 1.0, 2.0)}
        est[0, j], est[1, j] = (4 * D[0.5] - D[1.0]) / 3, (4 * D[1.0] - D[2.0]) / 3
    scale = np.max(np.abs(dval))
    bar = 10.0 * np.max(np.abs(est[0] - est[1])) / scale
    err = np.max(np.abs(dval[0] - est[0])) / scale
    print(f"total derivative {dval[0]}, partial {partial[0]}, differences {est[0]}; error {err:.3e}, bar {bar:.3e}")
    assert bar <= 1e-6 and err <= bar
    assert np.max(np.abs(dval[0] - partial[0])) > 1e-3 * scale      # (the initial state's share is not negligible)
