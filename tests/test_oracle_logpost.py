"""
Pins tests/logpost_oracle.py (the extended-precision Gaussian observation log-posterior, the yardstick of the device
reductions) against sums of ``scipy.stats.norm.logpdf`` on random inputs, and its invariance under a permutation of the
observation rows.  No GPU.
"""
import numpy as np
import pytest
from scipy.stats import norm
import logpost_oracle as lo

RTOL = 1e-13


def _random_case(seed, B=4, N=37, d=3, n_obs=29, k=7):
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((B, N + 1, d))
    obs = rng.standard_normal((n_obs, d))
    ind = rng.integers(0, N + 1, size=n_obs)
    upars = rng.standard_normal((B, k))
    return x0, obs, ind, upars


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_reference_equals_scipy_sums(seed, d):
    x0, obs, ind, upars = _random_case(seed, d=d)
    sd, psd = np.sqrt(0.005), 10.0
    for up, n_prior, k in ((None, None, 0), (upars, None, 7), (upars, 5, 5), (upars, 0, 0)):
        val, sab = lo.gauss_logpost_ref(x0, obs, ind, sd, up, n_prior, psd)
        assert val.shape == sab.shape == (x0.shape[0],) and val.dtype == np.float64
        for b in range(x0.shape[0]):
            t = norm.logpdf(obs, loc=x0[b][ind], scale=sd).ravel()
            if up is not None:
                t = np.concatenate([t, norm.logpdf(up[b, :k], 0.0, psd)])
            assert abs(val[b] - np.sum(t)) <= RTOL * abs(np.sum(t)), (b, val[b], np.sum(t))
            assert abs(sab[b] - np.sum(np.abs(t))) <= RTOL * np.sum(np.abs(t))
            assert sab[b] >= abs(val[b])


def test_indices_are_clamped_to_the_grid():
    x0, obs, ind, _ = _random_case(3, N=20, n_obs=6)
    ind = np.array([-5, 0, 7, 20, 21, 1000])
    val, _ = lo.gauss_logpost_ref(x0, obs, ind, 0.3)
    val_c, _ = lo.gauss_logpost_ref(x0, obs, np.clip(ind, 0, 20), 0.3)
    np.testing.assert_array_equal(val, val_c)


def test_no_terms_is_exactly_zero():
    x0 = np.random.default_rng(4).standard_normal((3, 8, 2))
    val, sab = lo.gauss_logpost_ref(x0, np.zeros((0, 2)), np.zeros(0, dtype=int), 0.1)
    assert np.all(val == 0.0) and np.all(sab == 0.0)
    assert np.all(lo.derived_bound(0, 2, sab) == 0.0)


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_invariant_under_a_permutation_of_the_observation_rows(seed):
    """Longdouble addition is not associative, so a reordered sum may differ in its last bits: the permuted value agrees with
    the unpermuted one to 1e-13 relative, compared in longdouble BEFORE the rounding to double."""
    x0, obs, ind, upars = _random_case(seed, n_obs=61, d=2)
    perm = np.random.default_rng(seed + 100).permutation(len(ind))
    v, s = lo.gauss_logpost_ref_ld(x0, obs, ind, 0.07, upars, 5)
    vp, sp = lo.gauss_logpost_ref_ld(x0, obs[perm], ind[perm], 0.07, upars, 5)
    assert v.dtype == np.longdouble and vp.dtype == np.longdouble
    assert np.all(np.abs(vp - v) <= np.longdouble(RTOL) * np.abs(v))
    assert np.all(np.abs(sp - s) <= np.longdouble(RTOL) * np.abs(s))
    # ... and a row moved WITHOUT its index changes the value: the invariance is not vacuous
    swapped = obs.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    vw, _ = lo.gauss_logpost_ref_ld(x0, swapped, ind, 0.07, upars, 5)
    assert np.all(np.abs(vw - v) > 1e-6 * np.abs(v))


def test_derived_bound_is_the_stated_formula():
    sab = np.array([3.0, 5.0])
    up = np.zeros((2, 7))
    np.testing.assert_array_equal(lo.derived_bound(40, 2, sab, up, 5), 8.0 * 85 * 2.0 ** -52 * sab)
    np.testing.assert_array_equal(lo.derived_bound(40, 2, sab, up), 8.0 * 87 * 2.0 ** -52 * sab)
    np.testing.assert_array_equal(lo.derived_bound(40, 2, sab), 8.0 * 80 * 2.0 ** -52 * sab)
