"""
MAGI on the device (rodeo_amd.inference.magi, src/rodeo/inference/magi.py:6-99) against the NumPy restatement
tests/magi_oracle.py, pinned in turn by the dense joint-Gaussian answer (tests/test_oracle_magi.py).
"""
import numpy as np
import pytest
import rodeo_amd as ra
from oracle import priors
import magi_oracle as mo

pytestmark = pytest.mark.gpu

PMAX = {"standard": 6, "square-root": 7}


def _pars(Q, R, kalman_type):
    return (Q, R) if kalman_type == "standard" else (Q, np.linalg.cholesky(R))


def _path(rng, Q, R, N):
    """A path of the prior X_n = Q X_{n-1} + N(0, R) (one per block), so that every forecast density is moderate."""
    d, p = Q.shape[:2]
    x = np.zeros((N + 1, d, p))
    x[0] = rng.standard_normal((d, p))
    for n in range(1, N + 1):
        for k in range(d):
            x[n, k] = Q[k] @ x[n - 1, k] + np.linalg.cholesky(R[k]) @ rng.standard_normal(p)
    return x


def _expand(data, scale=1.0):
    """The user's ode_expand: the data hold the first p - 1 components, the last one is scale times the one before it."""
    data = np.asarray(data)
    return np.concatenate([data, scale * data[..., -1:]], axis=-1)


def _problem(p, d, N, seed=0):
    rng = np.random.default_rng(seed)
    Q, R = (mo.random_prior if N <= 20 else mo.stable_prior)(rng, d, p)      # (long series: magi_oracle.stable_prior)
    return _path(rng, Q, R, N)[..., :p - 1], Q, R


def _check(kalman_type, p, na, d, N, seed=0, rel=1e-9):
    data, Q, R = _problem(p, d, N, seed)
    pars = _pars(Q, R, kalman_type)
    got = ra.inference.magi_logdens(data, _expand, na, pars, kalman_type)
    want = mo.magi_logdens(data, _expand, na, pars, kalman_type)
    assert isinstance(got, float)
    assert got == pytest.approx(want, rel=rel, abs=1e-12)


@pytest.mark.parametrize("kalman_type,p", [(k, p) for k in ("standard", "square-root") for p in (2, 3, 4, PMAX[k])])
def test_n_active_one_and_p(kalman_type, p):
    for na in sorted({1, p}):
        _check(kalman_type, p, na, d=2, N=17, seed=p)


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
@pytest.mark.parametrize("d", [1, 2, 3, 40])
def test_blocks(kalman_type, d):
    _check(kalman_type, 3, 2, d=d, N=17, seed=d)


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
@pytest.mark.parametrize("N", [0, 1, 2, 17, 200])
def test_steps(kalman_type, N):
    _check(kalman_type, 4, 2, d=2, N=N, seed=N)


def test_no_steps_is_zero():
    data, Q, R = _problem(3, 2, 0)
    assert ra.inference.magi_logdens(data, _expand, 2, (Q, R), "standard") == 0.0


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
def test_batched_data_and_params(kalman_type):
    B, p, d, N = 6, 3, 3, 30
    rng = np.random.default_rng(7)
    Q, R = mo.stable_prior(rng, d, p)
    data = np.stack([_path(rng, Q, R, N)[..., :p - 1] for _ in range(B)])
    scale = np.linspace(0.5, 1.5, B)[:, None]                                    # (B, 1): batched params
    pars = _pars(Q, R, kalman_type)
    got = ra.inference.magi_logdens(data, _expand, 2, pars, kalman_type, scale=scale)
    assert got.shape == (B,)
    want = [mo.magi_logdens(data[b], _expand, 2, pars, kalman_type, scale=scale[b]) for b in range(B)]
    np.testing.assert_allclose(got, want, rtol=1e-9)
    # batched params over shared data
    got = ra.inference.magi_logdens(data[0], _expand, 3, pars, kalman_type, scale=scale)
    want = [mo.magi_logdens(data[0], _expand, 3, pars, kalman_type, scale=scale[b]) for b in range(B)]
    np.testing.assert_allclose(got, want, rtol=1e-9)


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
def test_batched_prior_with_a_shared_state(kalman_type):
    B, p, d, N = 70, 3, 2, 25                                  # (more than one wave of trajectories)
    rng = np.random.default_rng(3)
    data, Q0, R0 = _problem(p, d, N, seed=3)
    Qs, Rs = [], []
    for b in range(B):
        Q, R = mo.stable_prior(rng, d, p)
        Qs.append(0.5 * (Q + Q0))
        Rs.append(R)
    Qs, Rs = np.stack(Qs), np.stack(Rs)
    pars = (Qs, Rs) if kalman_type == "standard" else (Qs, np.linalg.cholesky(Rs))
    got = ra.inference.magi_logdens(data, _expand, 2, pars, kalman_type)
    assert got.shape == (B,)
    for b in (0, 1, 33, 63, 64, 69):
        want = mo.magi_logdens(data, _expand, 2, (pars[0][b], pars[1][b]), kalman_type)
        assert got[b] == pytest.approx(want, rel=1e-9)


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
@pytest.mark.parametrize("p,na", [(2, 1), (3, 2), (5, 5)])
def test_linear_gaussian_exact_answer(kalman_type, p, na):
    rng = np.random.default_rng(11 * p + na)
    Q, R = priors.ibm_init(2.0, p, np.array([0.7, 1.3]))
    x = _path(rng, Q, R, 6)
    got = ra.inference.magi_logdens(x, lambda s: s, na, _pars(Q, R, kalman_type), kalman_type)
    rel = 1e-6 if p == 5 else 1e-9                             # (the dense IBM covariance at p = 5: tests/test_oracle_magi.py)
    assert got == pytest.approx(mo.exact_logdens(x, na, Q, R), rel=rel)


def test_standard_and_square_root_agree():
    # (n_active = 2 of 4: with 3 of 4 the standard form's covariance drifts from symmetry over these 100 steps, in the
    # oracle as on the device -- magi_oracle.stable_prior)
    data, Q, R = _problem(4, 3, 100, seed=5)
    a = ra.inference.magi_logdens(data, _expand, 2, (Q, R), "standard")
    b = ra.inference.magi_logdens(data, _expand, 2, (Q, np.linalg.cholesky(R)), "square-root")
    assert a == pytest.approx(b, rel=1e-8)


@pytest.mark.parametrize("kalman_type", ["standard", "square-root"])
def test_repeated_calls_give_identical_bits(kalman_type):
    B, p, d, N = 200, 3, 7, 50                                 # seven blocks: four waves per workgroup, reduced in LDS
    rng = np.random.default_rng(9)
    Q, R = mo.stable_prior(rng, d, p)
    data = np.stack([_path(rng, Q, R, N)[..., :p - 1] for _ in range(B)])
    pars = _pars(Q, R, kalman_type)
    a = ra.inference.magi_logdens(data, _expand, 2, pars, kalman_type)
    b = ra.inference.magi_logdens(data, _expand, 2, pars, kalman_type)
    assert a.tobytes() == b.tobytes()


def test_headline_shape():
    data, expand, omega, prior = mo.headline()
    got = ra.inference.magi_logdens(data, expand, 2, prior, "standard", omega=omega)
    assert got.shape == (1024,) and np.all(np.isfinite(got))
    for b in np.linspace(0, 1023, 8).astype(int):
        want = mo.magi_logdens(data, expand, 2, prior, "standard", omega=omega[b])
        assert got[b] == pytest.approx(want, rel=1e-8), b
