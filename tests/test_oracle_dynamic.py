"""
The restatement of ``solve_mv_dynamic`` (tests/dynamic_oracle.py) pinned by independent routes (no GPU):
  (a) for x'' = sin 2t - x the model is linear Gaussian once the scales are given: with the scales the restatement produced,
      its filtered and smoothed moments and its log-evidence equal dense joint-Gaussian conditioning of the time-varying model
      R_n = c_n R (oracle/joint_gaussian.py);
  (b) the first step's z^2 / s is 1 per block under schober and kramer, 1/2 under rodeo;
  (c) scale invariance: sigma x 3 leaves mean and var where they were and divides every scale by 9 (FitzHugh-Nagumo; at
      n_bstate = 5 the grid stops at N = 40, t_max = 1: schober with N >= 72 on t_max = 4 diverges in the restatement itself);
  (d) with a floor above every estimate the run is the constant-scale solver under (Q, scale_min R): oracle.scan.solve_mv for
      the moments, tests/evidence_oracle.py for quad and logdet.
"""
import numpy as np
import pytest
from scipy.stats import multivariate_normal
from oracle import interrogations as oi, joint_gaussian as jg, odes, priors, scan
import dynamic_oracle as dyo
import evidence_oracle as evo

THETA = np.array([0.2, 0.2, 3.0])
SIGMA = np.array([0.5, 0.3])
ITG = {"rodeo": oi.interrogate_rodeo, "schober": oi.interrogate_schober, "kramer": oi.interrogate_kramer}
GRIDS = [(2, 40, 1.0), (3, 40, 1.0), (3, 72, 4.0), (4, 40, 1.0), (5, 40, 1.0)]


def _fhn(p, N, t_max, sigma=SIGMA):
    W, init = priors.first_order_pad(odes.fitzhugh_nagumo, 2, p)
    x0 = init(np.array([-1.0, 1.0]), 0.0, theta=THETA)
    return W, x0, priors.ibm_init(t_max / N, p, sigma)


def _higher(p, N, t_max, sigma=0.5):
    W = np.zeros((1, 1, p)); W[0, 0, 2] = 1.0
    x0 = np.zeros((1, p)); x0[0, :3] = [-1.0, 0.0, 1.0]
    if p > 3:
        x0[0, 3] = 2.0                                  # x''' = 2 cos 2t - x'
    return W, x0, priors.ibm_init(t_max / N, p, np.array([sigma]))


def _worst(got, want):
    """largest |got - want| in units of max(1, |want|), entry by entry"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- (a) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kramer", "schober"])
@pytest.mark.parametrize("p", [3, 4])
def test_moments_and_evidence_equal_dense_conditioning_given_the_scales(p, name):
    N, t_max = 20, 2.0
    W, x0, (Q, R) = _higher(p, N, t_max)
    f = dyo.dynamic_filter(odes.higher_order, W, x0, 0.0, t_max, N, ITG[name], (Q, R))
    ms, vs, scale, ld = dyo.solve_mv_dynamic(odes.higher_order, W, x0, 0.0, t_max, N, ITG[name], (Q, R))
    assert np.all(np.isfinite(scale)) and np.all(scale > 0)
    # the chain X_0 = x0, X_n = Q X_{n-1} + chol(c_{n-1} R) e_n and the measurements Z_n = H X_n + a_n, n = 1..N
    ts = t_max * np.arange(1, N + 1) / N
    A, Cf, b = np.repeat(Q, N, axis=0), np.zeros((N + 1, p, p)), np.zeros((N + 1, p))
    b[0] = x0[0]
    for n in range(N):
        Cf[n + 1] = np.linalg.cholesky(scale[n, 0] * R[0])
    mu, S = jg.gauss_markov_mv(A, b, Cf)
    nx = (N + 1) * p
    mu, S = mu.reshape(-1), S.reshape(nx, nx)
    G = np.zeros((N, nx))
    if name == "kramer":                                # H = W - J = e_2 + e_0, a_n = -sin 2 t_n whatever the linearisation point
        for n in range(1, N + 1):
            G[n - 1, n * p + 2] = G[n - 1, n * p] = 1.0
        a = -np.sin(2 * ts)
    else:                                               # H = W, a_n = -f(mu-_n): the restatement's own interrogation points
        for n in range(1, N + 1):
            G[n - 1, n * p + 2] = 1.0
        a = -(np.sin(2 * ts) - f.mean_pred[0, 1:, 0, 0])
    jm = np.concatenate([mu, G @ mu + a])
    jS = np.block([[S, S @ G.T], [G @ S, G @ S @ G.T]])
    ref_ld = multivariate_normal.logpdf(np.zeros(N), G @ mu + a, G @ S @ G.T, allow_singular=False)

    def conditioned(n_seen):
        """(mean, var) of all of X given Z_1..Z_n_seen = 0"""
        keep = np.r_[np.arange(nx), nx + np.arange(n_seen)]
        icond = np.r_[np.zeros(nx, bool), np.ones(n_seen, bool)]
        Ac, bc, V = jg.mvncond(jm[keep], jS[np.ix_(keep, keep)], icond)
        return bc.reshape(N + 1, p), V.reshape(N + 1, p, N + 1, p)

    sm, sV = conditioned(N)
    errs = {"logdens": _worst(ld, ref_ld), "smoothed mean": _worst(ms[:, 0], sm),
            "smoothed var": _worst(vs[:, 0], np.stack([sV[n, :, n, :] for n in range(N + 1)]))}
    fm, fv = 0.0, 0.0
    for n in range(1, N + 1):
        cm, cV = conditioned(n)
        fm = max(fm, _worst(f.mean_filt[0, n, 0], cm[n]))
        fv = max(fv, _worst(f.var_filt[0, n, 0], cV[n, :, n, :]))
    errs["filtered mean"], errs["filtered var"] = fm, fv
    print(f"{name} p = {p}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; scales {scale.min():.2e} .. {scale.max():.2e}")
    assert max(errs.values()) <= 1e-8, errs


# ---- (b) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("schober", 1.0), ("kramer", 1.0), ("rodeo", 0.5)])
def test_first_step_identity(name, want):
    for p in (2, 3, 4, 5):
        W, x0, prior = _fhn(p, 1, 0.025)
        f = dyo.dynamic_filter(odes.fitzhugh_nagumo, W, x0, 0.0, 0.025, 1, ITG[name], prior, theta=THETA)
        assert f.quad.shape == (1, 2)
        assert np.max(np.abs(f.quad - want)) <= 1e-12, (p, f.quad)
    W, x0, prior = _higher(3, 1, 0.1)
    f = dyo.dynamic_filter(odes.higher_order, W, x0, 0.0, 0.1, 1, ITG[name], prior)
    assert np.max(np.abs(f.quad - want)) <= 1e-12, f.quad


# ---- (c) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ITG))
@pytest.mark.parametrize("p,N,t_max", GRIDS)
def test_scale_invariance(p, N, t_max, name):
    out = []
    for k in (1.0, 3.0):
        W, x0, prior = _fhn(p, N, t_max, SIGMA * k)
        out.append(dyo.solve_mv_dynamic(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], prior, theta=THETA))
    (m1, v1, s1, l1), (m3, v3, s3, l3) = out
    assert np.all(np.isfinite(m1)) and np.all(np.isfinite(v1)) and np.all(s1 > 0)
    dm = float(np.max(np.abs(m3 - m1)) / np.max(np.abs(m1)))
    dv = float(np.max(np.abs(v3 - v1)) / np.max(np.abs(v1)))
    ds = float(np.max(np.abs(s3 / s1 * 9.0 - 1.0)))
    dl = abs(l3 - l1) / max(1.0, abs(l1))
    print(f"{name} p = {p} N = {N}: mean {dm:.2e} var {dv:.2e} of the largest entry, scale ratio off by {ds:.2e}, logdens {dl:.2e}")
    assert dm <= 1e-9 and dv <= 1e-9, (dm, dv)
    assert ds <= 1e-5, ds
    assert dl <= 1e-9, dl


# ---- (d) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,floor", [("kramer", 2.0 ** 14), ("schober", 2.0 ** 14), ("rodeo", 2.0 ** 20)])
def test_floor_above_every_estimate_is_the_constant_scale_solver(name, floor):
    p, N, t_max = 3, 40, 1.0
    W, x0, (Q, R) = _fhn(p, N, t_max)
    free = dyo.dynamic_filter(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], (Q, R), theta=THETA)
    assert free.scale.max() < floor                                 # (the floor is above every estimate of the free run)
    f = dyo.dynamic_filter(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], (Q, R), scale_min=floor, theta=THETA)
    m, v, s, ld = dyo.solve_mv_dynamic(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], (Q, R), scale_min=floor, theta=THETA)
    assert np.all(s == floor)
    mo, vo = scan.solve_mv(None, odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], (Q, floor * R), theta=THETA)
    eld, equad, elogdet = evo.evidence(odes.fitzhugh_nagumo, W, x0, 0.0, t_max, N, ITG[name], (Q, floor * R), theta=THETA)
    errs = (float(np.max(np.abs(m - mo)) / np.max(np.abs(mo))), float(np.max(np.abs(v - vo)) / np.max(np.abs(vo))),
            float(np.max(np.abs(f.quad[0] - equad) / np.abs(equad))), float(np.max(np.abs(f.logdet[0] - elogdet) / np.abs(elogdet))),
            abs(ld - eld) / abs(eld))
    print(f"{name} floor 2^{int(np.log2(floor))}: mean {errs[0]:.2e} var {errs[1]:.2e} quad {errs[2]:.2e} logdet {errs[3]:.2e} "
          f"logdens {errs[4]:.2e}")
    assert max(errs) <= 1e-12, errs
