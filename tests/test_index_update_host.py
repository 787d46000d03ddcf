"""CPU tests of the index update's host side: BucketLayout.updated (the layout
after removing positions and appending labelled rows, by index arithmetic)
against BucketLayout.from_labels over the updated label sequence, and the
argument checks of lmi_index_move_rows / lmi_index_ingest_rows, which fail
before any device call."""
import numpy as np
import pytest

from li import _lib
from li.index import BucketLayout

N, C = 5000, 16


def _labels(rng, n, live):
    """n labels over the buckets `live` only (the others stay empty)."""
    return rng.choice(np.asarray(live), n).astype(np.int64)


def _check_step(layout, seq, drop, new_labels):
    """One updated() call against from_labels over the updated sequence `seq`
    (the labels in row order); returns the new (layout, seq)."""
    drop = np.asarray(drop, np.int64)
    new_labels = np.asarray(new_labels, np.int64)
    got, new_dst, surv_off, drop_before = layout.updated(drop, new_labels)
    # the new position of every surviving old position, in ascending old position
    n_surv = seq.size - drop.size
    assert surv_off.shape == (layout.n_buckets + 1,) and surv_off[0] == 0 and surv_off[-1] == n_surv
    at = np.full(n_surv + new_labels.size, -1, np.int64)
    BucketLayout.place_survivors(np.arange(n_surv, dtype=np.int64), surv_off, got.bucket_off, at)
    surv_dst = np.flatnonzero(at >= 0)
    assert np.array_equal(at[surv_dst], np.arange(n_surv))     # survivors keep their order
    keep_row = np.ones(seq.size, bool)
    keep_row[layout.order[drop]] = False
    seq2 = np.concatenate([seq[keep_row], new_labels])
    want = BucketLayout.from_labels(seq2, layout.n_buckets)
    assert got.n_buckets == want.n_buckets
    assert got.order.dtype == want.order.dtype and np.array_equal(got.order, want.order)
    assert got.bucket_off.dtype == want.bucket_off.dtype and np.array_equal(got.bucket_off, want.bucket_off)
    # new_dst: a bijection onto the positions the survivors do not occupy
    n2 = seq2.size
    assert new_dst.shape == (new_labels.size,) and surv_dst.shape == (seq.size - drop.size,)
    assert np.unique(new_dst).size == new_dst.size
    free = np.setdiff1d(np.arange(n2), surv_dst)
    assert np.array_equal(np.sort(new_dst), free)
    assert np.array_equal(np.sort(np.concatenate([surv_dst, new_dst])), np.arange(n2))
    # every new row lands in its bucket, behind the survivors, in batch order
    for c in np.unique(new_labels):
        at = new_dst[new_labels == c]
        assert np.all(np.diff(at) == 1) and at[-1] == want.bucket_off[c + 1] - 1
    # survivors keep their order; drop_before counts the drops per old bucket
    assert np.all(np.diff(surv_dst) > 0)
    assert np.array_equal(drop_before, [(np.sort(drop) < o).sum() for o in layout.bucket_off])
    return got, seq2


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_updated_equals_from_labels_over_random_chains(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    live = rng.choice(C, C - 4, replace=False)          # four buckets start empty
    empty = np.setdiff1d(np.arange(C), live)
    seq = _labels(rng, N, live)
    layout = BucketLayout.from_labels(seq, C)
    assert (layout.bucket_size == 0).sum() >= 4
    # adds that fill an empty bucket
    layout, seq = _check_step(layout, seq, [], np.concatenate([_labels(rng, 40, live),
                                                               np.full(3, empty[0])]))
    # a removal that empties a bucket (all of bucket live[0]) plus an add elsewhere
    c = int(live[0])
    whole = np.arange(layout.bucket_off[c], layout.bucket_off[c + 1])
    layout, seq = _check_step(layout, seq, whole, _labels(rng, 7, live[1:]))
    assert layout.bucket_size[c] == 0
    # the first and the last position
    layout, seq = _check_step(layout, seq, [0, seq.size - 1], [])
    # m = 0 and r = 0 together, r = 0 alone, m = 0 alone
    layout, seq = _check_step(layout, seq, [], [])
    layout, seq = _check_step(layout, seq, [], _labels(rng, 1, live))
    layout, seq = _check_step(layout, seq, rng.choice(seq.size, 1), [])
    # random chain of removes and adds, all buckets allowed
    for _ in range(6):
        r = int(rng.integers(0, 400))
        m = int(rng.integers(0, 400))
        drop = rng.choice(seq.size, r, replace=False)
        layout, seq = _check_step(layout, seq, drop, rng.integers(0, C, m))
    # everything removed, then refilled from nothing
    layout, seq = _check_step(layout, seq, np.arange(seq.size), [])
    assert seq.size == 0 and layout.bucket_off[-1] == 0
    layout, seq = _check_step(layout, seq, [], rng.integers(0, C, 300))


def test_updated_refuses_bad_arguments():
    layout = BucketLayout.from_labels(np.array([0, 2, 2, 1]), 3)
    with pytest.raises(ValueError):
        layout.updated([4], [])
    with pytest.raises(ValueError):
        layout.updated([-1], [])
    with pytest.raises(ValueError):
        layout.updated([1, 1], [])
    with pytest.raises(ValueError):
        layout.updated([], [3])


def test_update_entry_points_check_arguments_without_a_device():
    """Bad arguments are LMI_E_INVALID before any device call (the pointers
    here are host memory that is never read)."""
    lib = _lib.load()
    assert {"lmi_index_move_rows", "lmi_index_ingest_rows"} <= set(_lib.EXPORTS)
    buf = np.zeros(64, np.int64)
    other = np.zeros(64, np.int64)
    p, o = buf.ctypes.data, other.ctypes.data

    def move(**kw):
        a = dict(src=p, src_inv=p, n_old=4, d_pad=32, old_off=p, new_off=p, C=2, dropped=None, r=0,
                 before=None, dst=o, dst_inv=o, n_new=4, status=p)
        a.update(kw)
        return lib.lmi_index_move_rows(a["src"], a["src_inv"], a["n_old"], a["d_pad"], a["old_off"],
                                       a["new_off"], a["C"], a["dropped"], a["r"], a["before"],
                                       a["dst"], a["dst_inv"], a["n_new"], a["status"], None)

    for bad in (dict(d_pad=24), dict(d_pad=0), dict(n_old=-1), dict(C=0), dict(r=5), dict(n_new=3),
                dict(src=None), dict(status=None), dict(dst=p), dict(dst_inv=p),
                dict(r=1, n_new=3), dict(src=p + 2)):
        assert move(**bad) == _lib.LMI_E_INVALID, bad
        assert lib.lmi_last_error()
    # nothing survives: valid, and no device call
    assert move(n_old=0, n_new=0, src=None, dst=None) == _lib.LMI_OK
    assert move(n_old=3, r=3, n_new=0, dropped=p, before=p) == _lib.LMI_OK

    def ingest(**kw):
        a = dict(rows=p, dtype=_lib.LMI_F16, m=2, ld=8, d=8, d_pad=32, new_dst=p, dst=o, dst_inv=o,
                 n_new=2, status=p)
        a.update(kw)
        return lib.lmi_index_ingest_rows(a["rows"], a["dtype"], a["m"], a["ld"], a["d"], a["d_pad"],
                                         a["new_dst"], a["dst"], a["dst_inv"], a["n_new"], a["status"],
                                         None)

    for bad in (dict(dtype=7), dict(m=-1), dict(n_new=1), dict(d=0), dict(d_pad=64), dict(d_pad=8),
                dict(ld=7), dict(rows=None), dict(new_dst=None), dict(dst=None), dict(status=None)):
        assert ingest(**bad) == _lib.LMI_E_INVALID, bad
    assert ingest(m=0, rows=None, new_dst=None) == _lib.LMI_OK
