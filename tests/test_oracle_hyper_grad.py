"""
Pins tests/hyper_grad_oracle.py (the NumPy restatement of the ``"log_sigma"`` / ``"log_obs_var"`` directions of ``dalton_grid_jvp`` and
``fenrir_grid_jvp``), without a GPU, by tests/test_oracle_dalton_grad.py's scheme.

(a) Finite differences.  For every case of tests/hyper_grad_cases.py and every direction that is not zero, the restated derivative
    is compared with Richardson-extrapolated central differences of the UNTOUCHED value restatements
    ``dalton_grid_oracle.dalton_grid`` / ``fenrir_grid_oracle.fenrir_grid``, moved by the definition: sigma_b -> sigma_b e^eps through
    ``ibm_init``'s sigma, Om[:, b] -> e^eps Om[:, b].  D(h) = (f(+h) - f(-h)) / 2h, R(h) = (4 D(h/2) - D(h)) / 3, once from (h, h/2) and
    once from (2h, h); h = 1e-3 for a direction in the two log-scales alone, 1e-4 max(1, |theta_j|) for a unit theta direction, 1e-4
    for a mixed one.  Bar per case: 10 x the disagreement of the two estimates, relative to max |dvalue| over the call's directions
    per trajectory; as a condition on the case, that bar may not exceed 1e-6.  The unit theta directions are in the call because the
    log sigma derivative alone can be 1e-6 of them, below what differences of these values resolve.
(b) The scaling identity, free of differences: with zero initial variance, scaling every R and every Omega by c leaves all means
    as they are and multiplies all variances by c, so along (log_sigma = 1/2, log_obs_var = 1) the derivative is
    2 (value(2 R, 2 Omega) - value(R, Omega)) + n ln 2 - n / 2 with n = n_obs d.  Bar: 1e-9 of max |dvalue|.
(c) Linearity (the per-block unit derivatives sum to the common direction's), a zero direction gives exactly 0.0, the restated
    value is the value restatement's to 1e-12, and judgeability: no forecast variance in (1e-9, 1e-7) at any evaluated point, and
    the restated gradient moves by less than a tenth of the device bar under R (1 + 1e-15).
"""
import functools
import numpy as np
import pytest
import dalton_grid_cases as dgc
import grid_cases as gc
import hyper_grad_cases as hc

DEVICE_BAR = 1e-7                                                    # tests/test_gpu_hyper_grad.py: of max |dvalue| per trajectory


def _step(g, k):
    hyper = k in hc.hyper_columns(g)
    dth = None if g["dtheta"] is None else g["dtheta"][..., k, :]
    dx = None if g["dx0"] is None else g["dx0"][..., k, :, :]
    plain = (dth is not None and np.any(dth)) or (dx is not None and np.any(dx))
    if hyper and not plain:
        return 1e-3
    if not hyper and dth is not None and dth.ndim == 1 and np.count_nonzero(dth) == 1 and not (dx is not None and np.any(dx)):
        return 1e-4 * max(1.0, float(np.max(np.abs(g.theta[..., int(np.flatnonzero(dth)[0])]))))
    return 1e-4


@functools.lru_cache(maxsize=None)
def _differences(g):
    """Per case, once: the two Richardson estimates (B, K) (zero directions: 0) and every forecast variance met on the way."""
    B = 1 if g["B"] is None else g["B"]
    r1, r2, seen = np.zeros((B, g["K"])), np.zeros((B, g["K"])), []
    zeros = hc.zero_directions(g)
    g.value_case().restate_value(forecast_vars=seen)
    for k in range(g["K"]):
        if k in zeros:
            continue
        h = _step(g, k)
        f = {e: g.moved_value(k, e * h, forecast_vars=seen) for e in (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)}
        D = {e: (f[e] - f[-e]) / (2 * e * h) for e in (0.5, 1.0, 2.0)}
        r1[:, k] = (4 * D[0.5] - D[1.0]) / 3
        r2[:, k] = (4 * D[1.0] - D[2.0]) / 3
    return r1, r2, np.concatenate([np.ravel(w) for w in seen])


@functools.lru_cache(maxsize=None)
def _restated(g):
    return g.restate()


CASES = hc.cases()
IDS = [g["label"] for g in CASES]


def test_the_case_list_is_the_issue_s():
    assert len(hc.dalton_cases()) == 20 and len(hc.fenrir_cases()) == 22
    for family in (hc.dalton_cases(), hc.fenrir_cases()):
        items = {(1 if g["B"] is None else g["B"]) * g["K"] for g in family}
        assert {1, 33, 65} <= items
        assert any(g["kind"] == "per_traj" and g["dls"].ndim == 3 and g["dlo"].ndim == 3 for g in family)
        assert any(np.ndim(g["case"]["sigma"]) == 2 for g in family)                     # a batched sigma: R per lane
        assert any(g["case"]["W"].shape[-3] == 3 for g in family)                       # Lorenz63: three blocks
        assert sum(1 for g in family if g["case"]["nodes"][0] == 0) == 3
        assert {len(g["case"]["t"]) - 1 for g in family} >= {1, 2, 3, 40, 42}
    for g in CASES:
        if g["kind"] in ("standard", "per_traj"):
            n, d = g.theta.shape[-1], g["case"]["W"].shape[-3]
            assert g["K"] == n + 2 * d + 2 and hc.zero_directions(g) == [g["K"] - 1]
            assert len(hc.hyper_columns(g)) == 2 * d + 1


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_derivative_equals_richardson_differences_of_the_value_restatement(g):
    _, dval = _restated(g)
    r1, r2, _ = _differences(g)
    scale = np.max(np.abs(dval), axis=1, keepdims=True)
    disagreement = float(np.max(np.abs(r1 - r2) / scale))
    bar = 10.0 * disagreement
    err = float(np.max(np.abs(dval - r1) / scale))
    hyper = hc.hyper_columns(g)
    print(f"{g['label']}: max|dvalue| {scale.min():.3e} .. {scale.max():.3e}; hyper columns {np.abs(dval[:, hyper]).min():.3e} .. "
          f"{np.abs(dval[:, hyper]).max():.3e}; Richardson estimates disagree by {disagreement:.3e}, bar {bar:.3e}; "
          f"|restated - differences| = {err:.3e} of max|dvalue|")
    assert bar <= 1e-6, bar
    assert err <= bar, (err, bar)
    for k in hc.zero_directions(g):
        assert np.all(dval[:, k] == 0.0)


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_no_forecast_variance_near_the_threshold_at_any_evaluated_point(g):
    s = _differences(g)[2]
    inside = int(np.sum((s > 1e-9) & (s < 1e-7)))
    print(f"{g['label']}: forecast variances {s.min():.3e} .. {s.max():.3e} over the case and its perturbed points, {inside} inside (1e-9, 1e-7)")
    assert inside == 0
    own = []
    g.restate(forecast_vars=own)                                     # the tangent restatement meets the same variances
    own = np.asarray(own)
    assert int(np.sum((own > 1e-9) & (own < 1e-7))) == 0


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_derivative_is_well_conditioned(g):
    _, a = _restated(g)
    _, b = g.restate(1.0 + 1e-15)
    move = float(np.max(np.abs(a - b) / np.max(np.abs(a), axis=1, keepdims=True)))
    print(f"{g['label']}: the restated derivative moves by {move:.3e} of max|dvalue| under R (1 + 1e-15) (a tenth of the device bar: "
          f"{0.1 * DEVICE_BAR:.0e})")
    assert move < 0.1 * DEVICE_BAR


@pytest.mark.parametrize("g", CASES, ids=IDS)
def test_restated_value_is_the_value_restatement_s(g):
    val, _ = _restated(g)
    ref = np.atleast_1d(g.value_case().restate_value())
    assert np.max(np.abs(val - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-12


def _with_directions(g, dls, dlo):
    """The problem of ``g`` with its unit theta directions followed by the hyper directions (dls, dlo) (k, d)."""
    n, k = g.theta.shape[-1], len(dls)
    return hc.HCase(g, dtheta=np.concatenate([np.eye(n), np.zeros((k, n))]), dx0=None, dls=np.concatenate([np.zeros((n, len(dls[0]))), dls]),
                    dlo=np.concatenate([np.zeros((n, len(dls[0]))), dlo]), K=n + k, kind="identity")


def scaling_cases():
    """FitzHugh-Nagumo kramer and rodeo at N = 40, kramer at N = 3 with node 0 observed, Lorenz63 kramer: for both likelihoods."""
    problems = [dgc.make(gc.fhn(3, "kramer", "distinct")), dgc.make(gc.fhn(3, "rodeo", "distinct")),
                dgc.make(dgc._short(3, "kramer", 3), dgc.SHORT_NODES[3]), dgc.make(gc.lorenz(3, "kramer", "distinct", t_max=0.4, B=5))]
    return [hc.hyper_case(c, family, "one") for family in ("dalton", "fenrir") for c in problems]


def scaling_identity(g, value_at):
    """(the derivative the identity gives (B,), n): ``value_at(r_scale, Om)`` is the value at (r_scale R, Om)."""
    c = g["case"]
    n = c["y"].shape[0] * c["W"].shape[-3]
    v1, v2 = np.atleast_1d(value_at(1.0, c["Om"])), np.atleast_1d(value_at(2.0, 2.0 * c["Om"]))
    return 2.0 * (v2 - v1) + n * np.log(2.0) - n / 2.0, n


@pytest.mark.parametrize("g", scaling_cases(), ids=lambda g: g["label"])
def test_scaling_identity(g):
    d = g["case"]["W"].shape[-3]
    s = _with_directions(g, np.full((1, d), 0.5), np.ones((1, d)))
    _, dval = s.restate()
    seen = {1.0: [], 2.0: []}
    want, n = scaling_identity(g, lambda r, Om: g.value_case(Om=Om).restate_value(r_scale=r, forecast_vars=seen[r]))
    kept = {r: int(np.sum(np.asarray(w) > 1e-8)) for r, w in seen.items()}
    assert kept[1.0] == kept[2.0]                                    # (the 1e-8 rule keeps the same terms at both scales)
    scale = np.max(np.abs(dval), axis=1)
    err = float(np.max(np.abs(dval[:, -1] - want) / scale))
    print(f"{g['label']}: n = {n}; derivative along (1/2, 1) {dval[:, -1]}, by the identity {want}; error {err:.3e} of max|dvalue| "
          f"{scale.max():.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("g", scaling_cases(), ids=lambda g: g["label"])
def test_linearity_in_the_blocks(g):
    d = g["case"]["W"].shape[-3]
    eye, one, zero = np.eye(d), np.ones((1, d)), np.zeros((d + 1, d))
    s = _with_directions(g, np.concatenate([eye, one, zero]), np.concatenate([zero, eye, one]))
    _, dval = s.restate()
    n = g.theta.shape[-1]
    scale = np.max(np.abs(dval), axis=1)
    for k0 in (n, n + d + 1):                                        # log_sigma's block, then log_obs_var's
        assert np.max(np.abs(dval[:, k0:k0 + d].sum(axis=1) - dval[:, k0 + d]) / scale) <= 1e-12
