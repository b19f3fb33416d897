"""
The staging helpers of ``SolvePlan`` that the inference callers share (no GPU): ``staged`` (upload again only when shape or
bytes change, per slot), ``result_ring`` (four (B,) buffers in turn) and ``per_traj`` (float or array).  The plan is put
together by hand around a device stub that counts ``to_device`` / ``empty``.
"""
import numpy as np
import pytest
from rodeo_amd.solve import SolvePlan


class StubArray:
    def __init__(self, host=None, shape=None):
        self.host = None if host is None else np.array(host)
        self.shape = tuple(shape if host is None else self.host.shape)

    def to_host(self):
        return self.host


class StubDevice:
    def __init__(self):
        self.uploads, self.allocations = [], []

    def to_device(self, host):
        assert host.flags.c_contiguous
        self.uploads.append(host.shape)
        return StubArray(host)

    def empty(self, shape):
        self.allocations.append(tuple(shape))
        return StubArray(shape=shape)


@pytest.fixture
def plan():
    p = SolvePlan.__new__(SolvePlan)
    p.dev, p.B, p.batched = StubDevice(), 3, True
    p._staged, p._ring, p._ring_calls = {}, [], 0
    return p


def test_staged_uploads_only_what_changed(plan):
    obs, ind = np.arange(6.0).reshape(3, 2), np.array([0, 4, 9], dtype=np.int32)
    d_obs, d_ind = plan.staged("a", obs, ind)
    np.testing.assert_array_equal(d_obs.host, obs)
    np.testing.assert_array_equal(d_ind.host, ind)
    assert plan.dev.uploads == [(3, 2), (3,)]
    again = plan.staged("a", obs.copy(), ind.copy())                  # same bytes: the same device copies, no upload
    assert again[0] is d_obs and again[1] is d_ind and len(plan.dev.uploads) == 2
    other = plan.staged("b", ind)                                      # another slot: its own upload ...
    assert plan.dev.uploads[2:] == [(3,)]
    changed = obs.copy()
    changed[1, 1] += 1.0
    new = plan.staged("a", changed, ind)                               # one changed element: slot "a" again, and only it
    assert plan.dev.uploads[3:] == [(3, 2), (3,)] and new[0] is not d_obs
    np.testing.assert_array_equal(new[0].host, changed)
    assert plan.staged("b", ind)[0] is other[0] and len(plan.dev.uploads) == 5
    plan.staged("a", changed.reshape(2, 3), ind)                       # same bytes with another shape: uploaded again
    assert plan.dev.uploads[5:] == [(2, 3), (3,)]


def test_staged_slots_alternate_without_uploads(plan):
    y, z = np.ones((4, 2)), np.zeros((4, 2))
    first = {"dalton": plan.staged("dalton", y), "fenrir": plan.staged("fenrir", z)}
    assert len(plan.dev.uploads) == 2
    for _ in range(3):
        assert plan.staged("dalton", y)[0] is first["dalton"][0]
        assert plan.staged("fenrir", z)[0] is first["fenrir"][0]
    assert len(plan.dev.uploads) == 2


def test_staged_takes_non_contiguous_arrays(plan):
    table = np.arange(12, dtype=np.int32).reshape(3, 4)
    (col,) = plan.staged("a", table[:, 0])
    np.testing.assert_array_equal(col.host, [0, 4, 8])
    assert plan.staged("a", np.array([0, 4, 8], dtype=np.int32))[0] is col


def test_result_ring_turns_over_four_buffers(plan):
    ring = [plan.result_ring() for _ in range(6)]
    assert all(r.shape == (3,) for r in ring) and plan.dev.allocations == [(3,)] * 4
    assert len({id(r) for r in ring[:4]}) == 4
    assert ring[4] is ring[0] and ring[5] is ring[1]                   # the fifth call returns the first call's buffer


def test_result_ring_resets_when_the_batch_size_changes(plan):
    old = [plan.result_ring() for _ in range(2)]
    plan.B = 5
    new = [plan.result_ring() for _ in range(5)]
    assert all(r.shape == (5,) for r in new) and not any(r is o for r in new for o in old)
    assert len({id(r) for r in new[:4]}) == 4 and new[4] is new[0]     # counted from the reset


def test_per_traj_returns_an_array_or_a_float(plan):
    out = StubArray(np.array([1.5, 2.5, 3.5]))
    np.testing.assert_array_equal(plan.per_traj(out), [1.5, 2.5, 3.5])
    plan.batched = False
    val = plan.per_traj(StubArray(np.array([1.5])))
    assert isinstance(val, float) and val == 1.5
