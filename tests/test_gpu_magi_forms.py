"""
MAGI on the device, beyond tests/test_gpu_magi.py: the square-root form against the closed-form density at full
measurement with a coupled Q over a long series (where the standard form is not to be trusted, tests/test_oracle_magi_forms.py),
and the block-sum pass through the handle's scratch as it grows and is reused between calls of different sizes.
"""
import numpy as np
import pytest
import rodeo_amd as ra
import magi_oracle as mo
from test_oracle_magi_forms import _coupled, _closed_form

pytestmark = pytest.mark.gpu


def test_square_root_form_is_exact_at_full_measurement_with_a_coupled_q():
    x, Q, R = _coupled(N=400)
    got = ra.inference.magi_logdens(x, lambda s: s, 4, (Q, np.linalg.cholesky(R)), "square-root")
    assert got == pytest.approx(_closed_form(x, Q, R), rel=1e-9)


def test_block_sums_through_a_growing_scratch():
    rng = np.random.default_rng(4)
    for B, d in ((3, 2), (130, 45), (1, 64), (70, 2)):            # grows, then smaller calls reuse it
        Q, R = mo.stable_prior(rng, d, 3)
        data = np.stack([mo.headline(B=1, N=12, d=d, seed=b)[0] for b in range(B)])
        got = ra.inference.magi_logdens(data, lambda u: np.concatenate([u, u[..., -1:]], axis=-1), 2, (Q, R), "standard")
        assert got.shape == (B,)
        for b in sorted({0, B // 2, B - 1}):
            want = mo.magi_logdens(data[b], lambda u: np.concatenate([u, u[..., -1:]], axis=-1), 2, (Q, R), "standard")
            assert got[b] == pytest.approx(want, rel=1e-9), (B, d, b)
