"""CPU tests of the in-place index update's host side (K9): the slab plan
BucketLayout.inplace_slabs, replayed on a numpy array of row numbers against
the layout BucketLayout.updated gives, and the argument checks of
lmi_index_move_rows_inplace, which fail before any device call."""
import numpy as np
import pytest

from li import _lib
from li.index import BucketLayout

N, C = 5000, 16
SLAB_ROWS = (1, 33, 256, 10 ** 6)
DIRECT_ROWS = (1, 64, 10 ** 9)


def _dest(layout, new_layout, drop):
    """Where every old position goes (-1: dropped), from the tables alone:
    new_off[c] + (i - old_off[c]) - #{drops of bucket c before i}."""
    n = int(layout.bucket_off[-1])
    i = np.arange(n, dtype=np.int64)
    c = np.searchsorted(layout.bucket_off, i, side="right") - 1
    before = np.searchsorted(drop, i, side="left") - np.searchsorted(drop, layout.bucket_off, side="left")[c]
    dest = new_layout.bucket_off[c] + (i - layout.bucket_off[c]) - before
    dest[drop] = -1
    return dest


def _replay(layout, drop, new_labels, slab_rows, direct_rows):
    """One in-place update replayed on an array of row numbers: every slab's
    conditions, the final array against updated()'s layout.  Returns the new
    layout and the plan."""
    drop = np.sort(np.asarray(drop, np.int64))
    new_labels = np.asarray(new_labels, np.int64)
    assert drop.size == 0 or new_labels.size == 0    # an add or a remove, as the kernel's directions
    new_layout, new_dst, _, _ = layout.updated(drop, new_labels)
    n, n_new = int(layout.bucket_off[-1]), int(new_layout.bucket_off[-1])
    plan = layout.inplace_slabs(new_layout.bucket_off, drop, slab_rows, direct_rows)
    assert plan.dtype == np.int64 and plan.ndim == 2 and plan.shape[1] == 3
    dest = _dest(layout, new_layout, drop)
    # the store: old position p holds row number layout.order[p]; room for n_new rows
    store = np.full(max(n, n_new), -7, np.int64)
    store[:n] = layout.order
    pending = np.zeros(max(n, n_new), bool)          # rows a later slab still reads
    for a, b, _ in plan:
        assert 0 <= a < b <= n
        assert not pending[a:b].any(), "slabs overlap"
        pending[a:b] = True
    in_slab = pending[:n].copy()
    # rows outside every slab keep their place (or are dropped)
    out = np.flatnonzero(~in_slab)
    assert np.all((dest[out] == out) | (dest[out] == -1))
    prev = None
    for a, b, staged in plan:
        assert staged in (0, 1)
        if prev is not None:                         # an add backwards, a remove forwards
            assert (b <= prev[0]) if drop.size == 0 else (a >= prev[1])
        prev = (a, b)
        to = dest[a:b]
        live = to >= 0
        to = to[live]
        rows = store[a:b][live].copy()               # (a staged slab: the copy in the staging buffer)
        if staged:
            assert b - a <= slab_rows
        else:
            assert b - a >= direct_rows
            assert not ((to >= a) & (to < b)).any(), "a direct slab writes into its own source range"
        pending[a:b] = False
        assert not pending[to].any(), "a slab writes a row a later slab still reads"
        # every row of a slab moves, in the update's direction (rows that stay are in no slab)
        assert np.all(to > np.arange(a, b)[live]) if drop.size == 0 else np.all(to < np.arange(a, b)[live])
        store[to] = rows
    # the batch, behind the moved rows
    n_surv = n - drop.size
    keep_row = np.ones(n, bool)
    keep_row[layout.order[drop]] = False
    renum = np.cumsum(keep_row) - 1
    got = store[:n_new].copy()
    got[new_dst] = -1
    old = got >= 0
    assert old.sum() == n_surv
    got[old] = renum[got[old]]
    got[new_dst] = n_surv + np.arange(new_labels.size)
    assert np.array_equal(got, new_layout.order)
    return new_layout, plan


def _labels(rng, n, live):
    return rng.choice(np.asarray(live), n).astype(np.int64)


@pytest.mark.parametrize("direct_rows", DIRECT_ROWS)
@pytest.mark.parametrize("slab_rows", SLAB_ROWS)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plans_of_random_chains_replay_to_the_updated_layout(seed, slab_rows, direct_rows):
    rng = np.random.Generator(np.random.PCG64(seed))
    live = rng.choice(C, C - 4, replace=False)       # four buckets start empty
    layout = BucketLayout.from_labels(_labels(rng, N, live), C)
    assert (layout.bucket_size == 0).sum() >= 4
    for step in range(3):
        n = int(layout.bucket_off[-1])
        layout, _ = _replay(layout, [], rng.integers(0, C, int(rng.integers(1, 400))), slab_rows,
                            direct_rows)
        n = int(layout.bucket_off[-1])
        layout, _ = _replay(layout, rng.choice(n, int(rng.integers(1, 400)), replace=False), [],
                            slab_rows, direct_rows)
    # a run of neighbouring drops, and the first and the last row
    n = int(layout.bucket_off[-1])
    layout, _ = _replay(layout, np.r_[0, np.arange(700, 1100), n - 1], [], slab_rows, direct_rows)


@pytest.mark.parametrize("slab_rows,direct_rows", [(33, 1), (33, 64), (256, 10 ** 9), (1, 10 ** 9)])
def test_plan_corner_cases(slab_rows, direct_rows):
    rng = np.random.Generator(np.random.PCG64(7))
    live = np.array([1, 2, 3, 5, 6, 7, 8, 9, 10, 12])           # 0, 4, 11, 13, 14, 15 never held a row
    layout = BucketLayout.from_labels(_labels(rng, N, live), C)
    # m = 0 and r = 0: no slab at all
    _, plan = _replay(layout, [], [], slab_rows, direct_rows)
    assert plan.shape == (0, 3)
    # adds only to the last non-empty bucket, and behind it: nothing moves
    _, plan = _replay(layout, [], np.full(9, 12), slab_rows, direct_rows)
    assert plan.shape == (0, 3)
    _, plan = _replay(layout, [], np.full(9, 15), slab_rows, direct_rows)
    assert plan.shape == (0, 3)
    # adds only to bucket 0 (which never held a row): every row moves, by 2 (a small shift)
    _, plan = _replay(layout, [], np.full(2, 0), slab_rows, direct_rows)
    assert (plan[:, 1] - plan[:, 0]).sum() == N
    if direct_rows <= 2:
        assert not plan[:, 2].any() and np.all(plan[:, 1] - plan[:, 0] <= 2)
    # adds only to the first bucket that holds rows: its own rows stay
    _, plan = _replay(layout, [], np.full(40, 1), slab_rows, direct_rows)
    assert plan[:, 0].min() == layout.bucket_off[2]
    # an add into a bucket in the middle that never held a row
    _, plan = _replay(layout, [], np.full(300, 4), slab_rows, direct_rows)
    assert plan[:, 0].min() == layout.bucket_off[5]
    # all rows removed; one row removed (the last: nothing moves; the first: all move by one)
    _, plan = _replay(layout, np.arange(N), [], slab_rows, direct_rows)
    assert plan.shape == (0, 3)
    _, plan = _replay(layout, [N - 1], [], slab_rows, direct_rows)
    assert plan.shape == (0, 3)
    _, plan = _replay(layout, [0], [], slab_rows, direct_rows)
    assert plan[0, 0] == 1 and plan[-1, 1] == N
    # the empty layout takes any batch without a slab
    _, plan = _replay(BucketLayout.from_labels(np.zeros(0, np.int64), C), [], rng.integers(0, C, 50),
                      slab_rows, direct_rows)
    assert plan.shape == (0, 3)


def test_plan_refuses_bad_arguments():
    layout = BucketLayout.from_labels(np.array([0, 2, 2, 1]), 3)
    new, _, _, _ = layout.updated([], [1])
    with pytest.raises(ValueError):
        layout.inplace_slabs(new.bucket_off, [], 0, 1)
    with pytest.raises(ValueError):
        layout.inplace_slabs(new.bucket_off, [], 1, 0)
    with pytest.raises(ValueError):
        layout.inplace_slabs(new.bucket_off[:-1], [], 8, 8)
    with pytest.raises(ValueError):
        layout.inplace_slabs(new.bucket_off, [1], 8, 8)       # a drop and a new row at once
    with pytest.raises(ValueError):
        layout.inplace_slabs(layout.bucket_off - np.array([0, 0, 1, 1]), [], 8, 8)   # a left shift without drops
    with pytest.raises(ValueError):
        layout.inplace_slabs(layout.updated([1, 2], [])[0].bucket_off, [2, 1], 8, 8)


def test_inplace_entry_point_checks_arguments_without_a_device():
    """Bad arguments are LMI_E_INVALID before any device call (the pointers
    here are host memory that is never read as device memory)."""
    lib = _lib.load()
    assert "lmi_index_move_rows_inplace" in _lib.EXPORTS
    buf = np.zeros(64, np.int64)
    other = np.zeros(64, np.int64)
    p, o = buf.ctypes.data, other.ctypes.data

    def slabs(*rows):
        return np.ascontiguousarray(np.array(rows, np.int64).reshape(-1, 3))

    def move(plan, **kw):
        a = dict(corpus=p, inv=p, n_old=100, n_new=110, capacity=128, d_pad=32, old_off=p, new_off=p,
                 C=2, dropped=None, r=0, before=None, direction=_lib.LMI_INPLACE_ADD, stage=o,
                 stage_inv=o, stage_rows=16, flags=0, status=p)
        a.update(kw)
        return lib.lmi_index_move_rows_inplace(
            a["corpus"], a["inv"], a["n_old"], a["n_new"], a["capacity"], a["d_pad"], a["old_off"],
            a["new_off"], a["C"], a["dropped"], a["r"], a["before"], a["direction"],
            plan.ctypes.data if plan is not None else None, 0 if plan is None else plan.shape[0],
            a["stage"], a["stage_inv"], a["stage_rows"], a["flags"], a["status"], None)

    good = slabs((60, 100, 0), (44, 60, 1), (40, 44, 1))
    rem = dict(direction=_lib.LMI_INPLACE_REMOVE, n_new=90, r=10, dropped=p, before=p)
    good_rem = slabs((5, 20, 1), (20, 100, 0))
    bad = [
        (good, dict(n_new=129)),                                  # n_new > capacity
        (good, dict(capacity=99)),                                # n_old > capacity
        (good, dict(n_new=99)),                                   # an add that shrinks
        (good, dict(r=1, dropped=p, before=p)),                   # an add that drops
        (good, dict(direction=0)), (good, dict(flags=2)),
        (good, dict(d_pad=24)), (good, dict(C=0)), (good, dict(n_old=-1)),
        (slabs((60, 100, 0), (44, 61, 1)), {}),                   # overlapping
        (slabs((44, 60, 1), (60, 100, 0)), {}),                   # an add's slabs front to back
        (slabs((60, 101, 0)), {}), (slabs((-1, 10, 1)), {}), (slabs((10, 10, 1)), {}),
        (slabs((60, 100, 2)), {}),
        (slabs((60, 100, 0), (43, 60, 1)), {}),                   # 17 staged rows, 16 in the buffer
        (good, dict(stage_rows=15)),
        (good, dict(corpus=None)), (good, dict(inv=None)), (good, dict(old_off=None)),
        (good, dict(new_off=None)), (good, dict(status=None)), (good, dict(stage=None)),
        (good, dict(stage_inv=None)), (good, dict(corpus=p + 2)), (good, dict(stage=o + 2)),
        (good, dict(stage=p)),                                    # staging is the store itself
        (good_rem, dict(rem, n_new=91)),                          # a remove that leaves another count
        (good_rem, dict(rem, dropped=None)), (good_rem, dict(rem, before=None)),
        (slabs((20, 100, 0), (5, 20, 1)), rem),                   # a remove's slabs back to front
        (slabs((5, 21, 1), (20, 100, 0)), dict(rem, stage_rows=32)),   # overlapping
    ]
    for plan, kw in bad:
        assert move(plan, **kw) == _lib.LMI_E_INVALID, (plan.tolist(), kw)
        assert lib.lmi_last_error()
    # no slab: valid, and no device call (an update in which no row moves)
    assert move(None) == _lib.LMI_OK
    assert move(None, corpus=None, inv=None, n_old=0, n_new=0, capacity=0) == _lib.LMI_OK
    assert move(None, **rem) == _lib.LMI_OK
