"""
Test helper (not collected): the Gaussian observation log-posterior of docs/examples/parameter.md:188-210 from its formula, in
extended precision -- the yardstick of the device reductions (gauss_logpost_kernel, bwd_sim_tile3_kernel<true>).

    sum_k sum_j norm.logpdf(obs[k, j], loc = x0[b, ind[k], j], scale = noise_sd) + sum_{i < n_prior} norm.logpdf(upars[b, i], 0, prior_sd)

Every term is evaluated in ``np.longdouble`` as  -z^2 / 2 - log(sd) - log(2 pi) / 2  and the terms of a trajectory are added with
``np.sum`` over longdoubles (pairwise): neither scipy nor the kernels' lane assignment, xor tree or walk from the end.
"""
import numpy as np

LD = np.longdouble


def _half_log_2pi():
    """log(2 pi) / 2 in longdouble: pi = 4 atan(1) evaluated in longdouble, not the rounded double constant."""
    return LD(0.5) * np.log(LD(8.0) * np.arctan(LD(1.0)))


def _logpdf_terms(x, loc, sd):
    z = (np.asarray(x, dtype=LD) - np.asarray(loc, dtype=LD)) / LD(sd)
    return -LD(0.5) * z * z - np.log(LD(sd)) - _half_log_2pi()


def gauss_logpost_ref_ld(x0, obs, ind, noise_sd, upars=None, n_prior=None, prior_sd=10.0):
    """``(values, sum_abs)`` as longdouble arrays (B,): see ``gauss_logpost_ref``."""
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 3:
        raise ValueError("x0 must be (B, N+1, d)")
    B, N1, d = x0.shape
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, d)
    ind = np.clip(np.asarray(ind, dtype=np.int64).reshape(-1), 0, N1 - 1)       # both kernels clamp to [0, N]
    if obs.shape[0] != ind.shape[0]:
        raise ValueError("obs and ind disagree on n_obs")
    terms = _logpdf_terms(obs[None], x0[:, ind, :], noise_sd).reshape(B, -1)     # (B, n_obs * d)
    if upars is not None:
        up = np.asarray(upars, dtype=np.float64)
        k = up.shape[1] if n_prior is None else int(n_prior)
        terms = np.concatenate([terms, _logpdf_terms(up[:, :k], 0.0, prior_sd).reshape(B, -1)], axis=1)
    return np.sum(terms, axis=1, dtype=LD), np.sum(np.abs(terms), axis=1, dtype=LD)


def gauss_logpost_ref(x0, obs, ind, noise_sd, upars=None, n_prior=None, prior_sd=10.0):
    """
    ``x0`` (B, N+1, d): the zeroth derivative of a path or of a mean; ``obs`` (n_obs, d); ``ind`` (n_obs,) grid indices in any
    order, clamped to [0, N]; ``upars`` (B, k) optional, its first ``n_prior`` (default: all) entries get the N(0, prior_sd^2)
    prior.  Returns ``(values (B,), sum_abs (B,))`` as doubles: the log-posterior per trajectory and the sum of the absolute
    values of its terms, both accumulated in longdouble and rounded once.
    """
    val, sab = gauss_logpost_ref_ld(x0, obs, ind, noise_sd, upars, n_prior, prior_sd)
    return val.astype(np.float64), sab.astype(np.float64)


def n_terms(n_obs, d, upars=None, n_prior=None):
    if upars is None:
        return n_obs * d
    return n_obs * d + (np.shape(upars)[1] if n_prior is None else int(n_prior))


def derived_bound(n_obs, d, sum_abs, upars=None, n_prior=None):
    """
    The bound of every "device reduction against this reference ON THE SAME PATH" comparison:

        |dev - ref| <= 8 * n_terms * 2^-52 * sum|term|,      n_terms = n_obs * d + n_prior.

    Where it comes from (u = 2^-53): the device adds n_terms doubles in some order, and a sum of n numbers in any order is off
    by at most (n - 1) u sum|term| to first order.  Each term is -z^2/2 - log(sd) - log(2 pi)/2 from a handful of rounded
    operations (a subtraction, a division, two multiplications, two subtractions, a rounded constant, a libm log): a few u
    relative to its partial results, which are of the size of the term where z^2/2 dominates (observations of order 1 with
    noise_sd = 0.07: z^2/2 ~ 100 against |log sd| + 0.92 < 3.6) and where all three pieces have one sign (the prior terms).
    Together below (n_terms + 7) u sum|term| <= 8 n_terms u sum|term|; the bound keeps a further factor 2.  sum|term| is this
    reference's, never the device's.  With no term at all the bound is 0: exact zeros.
    """
    return 8.0 * n_terms(n_obs, d, upars, n_prior) * 2.0 ** -52 * np.asarray(sum_abs, dtype=np.float64)
