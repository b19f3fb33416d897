"""
The restatement of ``solve_evidence`` (tests/evidence_oracle.py) and the host helpers ``evidence_scale`` / ``evidence_at``
(no GPU):
  (a) exact pin: for x'' = sin 2t - x under interrogate_kramer the solver's model is exactly linear Gaussian, so the
      log-evidence equals the dense joint-Gaussian log-density of Z_{1:N} at 0 under the prior (oracle/joint_gaussian.py);
  (b) the scale law behind the closed-form calibration, prior_var_b -> c_b prior_var_b with c = (9, 0.25);
  (c) recalibration: after one rescaling by ``evidence_scale`` the mean normalised squared innovation is 1 and the evidence
      is larger;
  (d) the standard and square-root restatements agree for L L^T inputs (kramer, schober).
"""
import numpy as np
import pytest
from scipy.stats import multivariate_normal
from oracle import interrogations as oi, joint_gaussian as jg, odes, priors
from rodeo_amd.evidence import Evidence, evidence_at, evidence_scale
import evidence_oracle as evo

THETA = np.array([0.2, 0.2, 3.0])
SIGMA = np.array([0.5, 0.3])
C = np.array([9.0, 0.25])
ITG = {"rodeo": oi.interrogate_rodeo, "schober": oi.interrogate_schober, "kramer": oi.interrogate_kramer}


def _fhn(p, N, t_max, sigma=SIGMA):
    W, init = priors.first_order_pad(odes.fitzhugh_nagumo, 2, p)
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    return W, x0, priors.ibm_init(t_max / N, p, sigma)


def _run(name, p, N, t_max, prior, kalman_type="standard"):
    W, x0, _ = _fhn(p, N, t_max)
    ld, quad, logdet = evo.evidence(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], prior, kalman_type, theta=THETA)
    return Evidence(ld, quad, logdet, N)


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(want)))


# ---- (a) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 4])
def test_evidence_equals_the_dense_joint_gaussian_density_for_a_linear_ode(p):
    N, t_max, sigma = 20, 2.0, 0.5
    W = np.zeros((1, 1, p)); W[0, 0, 2] = 1.0
    x0 = np.zeros((1, p)); x0[0, :3] = [-1.0, 0.0, 1.0]
    if p > 3:
        x0[0, 3] = 2.0                                  # x''' = 2 cos 2t - x'
    Q, R = priors.ibm_init(t_max / N, p, np.array([sigma]))
    ld, quad, logdet = evo.evidence(odes.higher_order, W, x0, 0.0, t_max, N, oi.interrogate_kramer, (Q, R))
    # Z_n = H X_n - sin 2 t_n with H = W - J = e_2 + e_0, whatever the linearisation point
    A, Cf, b = np.repeat(Q, N, axis=0), np.zeros((N + 1, p, p)), np.zeros((N + 1, p))
    b[0] = x0[0]
    Cf[1:] = np.linalg.cholesky(R[0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    mu, S = mu.reshape(-1), S.reshape((N + 1) * p, (N + 1) * p)
    G = np.zeros((N, (N + 1) * p))
    for n in range(1, N + 1):
        G[n - 1, n * p + 2] = G[n - 1, n * p] = 1.0
    ts = t_max * np.arange(1, N + 1) / N
    ref = multivariate_normal.logpdf(np.sin(2 * ts), G @ mu, G @ S @ G.T, allow_singular=False)
    print(f"p = {p}: restatement {ld:.10f}, dense {ref:.10f}, difference {abs(ld - ref):.3e}")
    assert abs(ld - ref) <= 1e-8 * max(1.0, abs(ref))
    assert abs(ld - (-0.5 * (quad.sum() + logdet.sum()) - N * evo.LOG_2PI / 2)) <= 1e-12 * abs(ld)


# ---- (b) -----------------------------------------------------------------------------------------------------------------
SCALE_CASES = ([(3, 17, 1.7, k) for k in ITG] + [(3, 72, 4.0, k) for k in ITG] +
               [(p, 40, 2.0, k) for p in (2, 4, 5) for k in ("rodeo", "kramer")] + [(6, 40, 2.0, "rodeo")])


@pytest.mark.parametrize("p,N,t_max,name", SCALE_CASES)
def test_scale_law(p, N, t_max, name):
    """quad_b -> quad_b / c_b, logdet_b -> logdet_b + N log c_b, and ``evidence_at`` predicts the second run's value."""
    _, _, (Q, R) = _fhn(p, N, t_max)
    one = _run(name, p, N, t_max, (Q, R))
    two = _run(name, p, N, t_max, (Q, R * C[:, None, None]))
    errs = (_rel(two.quad, one.quad / C), _rel(two.logdet, one.logdet + N * np.log(C)), _rel(two.logdens, evidence_at(one, C)))
    print(f"{name} p = {p} N = {N}: quad {errs[0]:.2e} logdet {errs[1]:.2e} logdens {errs[2]:.2e}")
    assert max(errs) <= 1e-10, errs


def test_scale_law_in_the_square_root_form():
    """The factor times sqrt(c): the same law (interrogate_rodeo's W L W^T "factor" scales with the factor)."""
    p, N, t_max = 3, 17, 1.7
    _, _, (Q, R) = _fhn(p, N, t_max)
    L = np.linalg.cholesky(R)
    for name in ITG:
        one = _run(name, p, N, t_max, (Q, L), "square-root")
        two = _run(name, p, N, t_max, (Q, L * np.sqrt(C)[:, None, None]), "square-root")
        errs = (_rel(two.quad, one.quad / C), _rel(two.logdet, one.logdet + N * np.log(C)),
                _rel(two.logdens, evidence_at(one, C)))
        print(f"square-root {name}: quad {errs[0]:.2e} logdet {errs[1]:.2e} logdens {errs[2]:.2e}")
        assert max(errs) <= 1e-10, errs


def test_the_quick_start_is_far_from_calibrated():
    """FitzHugh-Nagumo quick start (n_bstate = 3, N = 72, t_max = 4, kramer): the figures that motivate the calibration."""
    _, _, prior = _fhn(3, 72, 4.0)
    ev = _run("kramer", 3, 72, 4.0, prior)
    c = evidence_scale(ev)
    print(f"sigma = {SIGMA}: quad / N = {c}, logdens = {ev.logdens:.2f}, calibrated {evidence_at(ev, c):.2f}")
    assert 250 < c[0] < 400 and 2 < c[1] < 4
    assert -10900 < ev.logdens < -10700 and 300 < evidence_at(ev, c) < 370


# ---- (c) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,N,t_max,name", SCALE_CASES)
def test_recalibration(p, N, t_max, name):
    _, _, (Q, R) = _fhn(p, N, t_max)
    one = _run(name, p, N, t_max, (Q, R))
    c = evidence_scale(one)
    two = _run(name, p, N, t_max, (Q, R * c[:, None, None]))
    off = float(np.max(np.abs(evidence_scale(two) - 1.0)))
    print(f"{name} p = {p} N = {N}: c = {c}, |quad / N - 1| after rescaling {off:.2e}, logdens {one.logdens:.3f} -> {two.logdens:.3f}")
    assert off <= 1e-10
    assert two.logdens > one.logdens
    assert abs(two.logdens - evidence_at(one, c)) <= 1e-10 * abs(two.logdens)


# ---- (d) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kramer", "schober"])
@pytest.mark.parametrize("N,t_max", [(17, 1.7), (72, 4.0)])
def test_standard_and_square_root_forms_agree(name, N, t_max):
    """Not under interrogate_rodeo: its square-root var_meas is the reference's W L W^T, another model."""
    _, _, (Q, R) = _fhn(3, N, t_max)
    std = _run(name, 3, N, t_max, (Q, R))
    sq = _run(name, 3, N, t_max, (Q, np.linalg.cholesky(R)), "square-root")
    errs = (_rel(sq.quad, std.quad), _rel(sq.logdet, std.logdet), _rel(sq.logdens, std.logdens))
    print(f"{name} N = {N}: quad {errs[0]:.2e} logdet {errs[1]:.2e} logdens {errs[2]:.2e}")
    assert max(errs) <= 1e-8, errs
