"""Filtered search, the parts that need no device: the two C symbols, every
refusal of lmi_bucket_topk_tagged (before any launch, with a message), the
tagged workspace size against the untagged one, the tag bookkeeping of
BucketLayout updates and relabels (numpy only) and the eligible-count helper."""
import ctypes as C

import numpy as np
import pytest

from li import _lib
from li.index import BucketLayout, check_tags, eligible_counts


def _desc(dtype=None, d_pad=768, **kw):
    d = _lib.IndexDesc()
    d.dtype = _lib.LMI_F16 if dtype is None else dtype
    d.d, d.d_pad, d.n_rows, d.n_buckets = d_pad, d_pad, 10**6, 122
    d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
    for name, v in kw.items():          # (dummy addresses: never dereferenced)
        setattr(d, name, v)
    return d


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("lmi_scan_tagged_workspace_bytes", "lmi_bucket_topk_tagged"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.lmi_abi_version() == 13


def _call(lib, d, *, tags=4096, want=4096, k=10, qmode=0):
    return lib.lmi_bucket_topk_tagged(C.byref(d), tags, want, 4096, 8, d.d, 4096, 2, k, qmode,
                                      4096, 4096, 4096, 4096, 1 << 40, None)


@pytest.mark.parametrize("what,desc_kw,call_kw", [
    ("null tags", {}, dict(tags=None)),
    ("null want", {}, dict(want=None)),
    ("k > LMI_MAX_K", {}, dict(k=_lib.LMI_MAX_K + 1)),
    ("corpus32", dict(corpus32=4096), {}),
    ("corpus64", dict(corpus64=4096), {}),
    ("chunk_centroid", dict(chunk_centroid=4096), {}),
    ("plan phase", {}, dict(qmode=_lib.LMI_Q_PHASE_PLAN)),
    ("scan phase", {}, dict(qmode=_lib.LMI_Q_PHASE_SCAN)),
    ("merge phase", {}, dict(qmode=_lib.LMI_Q_PHASE_MERGE)),
    ("refine phase", {}, dict(qmode=_lib.LMI_Q_PHASE_REFINE)),
    ("join", {}, dict(qmode=_lib.LMI_Q_PHASE_SCAN_JOIN)),
    ("seed", {}, dict(qmode=_lib.LMI_Q_SEED_ROUND0)),
    ("all phases + f32", {}, dict(qmode=_lib.LMI_Q_F32 | _lib.LMI_Q_PHASE_PLAN | _lib.LMI_Q_PHASE_SCAN
                                  | _lib.LMI_Q_PHASE_MERGE)),
])
def test_refusals_without_a_device(what, desc_kw, call_kw):
    lib = _lib.load()
    rc = _call(lib, _desc(**desc_kw), **call_kw)
    assert rc == _lib.LMI_E_INVALID, what
    msg = lib.lmi_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert "lmi_bucket_topk_tagged" in msg, (what, msg)


def test_workspace_equals_the_untagged_one_where_the_families_agree():
    """Untagged: the 8-wave ring for (fp16 corpus, fp16-exact queries, d_pad
    768) up to k = 15, the 4-wave ring there at k = 16, the general kernel
    elsewhere.  Tagged: the 8-wave ring there up to k = 10, the general kernel
    for everything else.  So the families agree off the ring shape and, on it,
    up to k = 10."""
    lib = _lib.load()
    same = other = 0
    for dtype in (_lib.LMI_F16, _lib.LMI_F32):
        for d_pad in (96, 768):
            for qmode in (_lib.LMI_Q_F16, _lib.LMI_Q_F32):
                for k in (1, 10, 11, 15, 16):
                    for nq, R in ((1, 1), (1000, 4), (10000, 7)):
                        d = _desc(dtype, d_pad)
                        t = lib.lmi_scan_tagged_workspace_bytes(C.byref(d), nq, R, k, qmode)
                        u = lib.lmi_scan_workspace_bytes(C.byref(d), nq, R, k, qmode)
                        assert t > 0
                        ring = dtype == _lib.LMI_F16 and d_pad == 768 and qmode == _lib.LMI_Q_F16
                        if not ring or k <= 10:
                            assert t == u, (dtype, d_pad, qmode, k, nq, R)
                            same += 1
                        else:
                            other += 1
    assert same and other
    # what the tagged call refuses has no size
    d = _desc()
    assert lib.lmi_scan_tagged_workspace_bytes(C.byref(d), 10, 2, _lib.LMI_MAX_K + 1, 0) == 0
    assert lib.lmi_scan_tagged_workspace_bytes(C.byref(_desc(corpus32=4096)), 10, 2, 10, 0) == 0
    assert lib.lmi_scan_tagged_workspace_bytes(C.byref(_desc(chunk_centroid=4096)), 10, 2, 10, 0) == 0
    assert lib.lmi_scan_tagged_workspace_bytes(C.byref(d), 10, 2, 10, _lib.LMI_Q_PHASE_SCAN) == 0


def _by_pos(labels, tags, n_buckets):
    return np.asarray(tags)[BucketLayout.from_labels(labels, n_buckets).order]


def test_tags_follow_updates_and_relabels():
    rng = np.random.default_rng(3)
    n, m, r, C_ = 500, 40, 60, 7
    lab = rng.integers(0, C_, n)
    tags = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    lay = BucketLayout.from_labels(lab, C_)
    t_pos = tags[lay.order]
    # remove r positions and add m rows in one update, then each alone
    for drop_n, add_n in ((r, m), (r, 0), (0, m), (0, 0)):
        drop = np.sort(rng.choice(n, drop_n, replace=False))
        new_lab = rng.integers(0, C_, add_n)
        new_tags = rng.integers(0, 1 << 32, add_n, dtype=np.uint64).astype(np.uint32)
        lay2, new_dst, surv_off, _ = lay.updated(drop, new_lab)
        got = BucketLayout.updated_table(t_pos, drop, surv_off, lay2.bucket_off, new_dst, new_tags)
        keep = np.ones(n, bool)
        keep[lay.order[drop]] = False
        want = _by_pos(np.concatenate([lab[keep], new_lab]), np.concatenate([tags[keep], new_tags]), C_)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (drop_n, add_n)
        assert np.array_equal(lay2.order, BucketLayout.from_labels(np.concatenate([lab[keep], new_lab]), C_).order)
    # a relabel permutation, to another number of buckets
    lab2 = rng.integers(0, C_ + 3, n)
    lay3 = BucketLayout.from_labels(lab2, C_ + 3)
    src = BucketLayout.relabel_source(lay.order, lay3.order)
    assert np.array_equal(np.sort(src), np.arange(n))
    assert np.array_equal(t_pos[src], _by_pos(lab2, tags, C_ + 3))


def test_eligible_counts_equal_a_numpy_loop():
    rng = np.random.default_rng(4)
    sizes = np.array([0, 300, 1, 0, 77, 5, 0])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tags = rng.integers(0, 16, off[-1]).astype(np.uint32)
    tags[::7] |= np.uint32(1 << 31)
    for w in (0, 1, 6, 15, 1 << 31, (1 << 31) | 3, 1 << 20):
        want = [int(sum(1 for t in tags[off[c]:off[c + 1]] if (int(t) & w) == w)) for c in range(sizes.size)]
        got = eligible_counts(tags, off, w)
        assert got.dtype == np.int64 and got.tolist() == want, w
    assert eligible_counts(np.zeros(0, np.uint32), np.zeros(3, np.int64), 1).tolist() == [0, 0]


def test_check_tags():
    assert check_tags([0, 1, (1 << 32) - 1], 3).dtype == np.uint32
    assert check_tags(np.array([5], np.int8), 1).tolist() == [5]
    for bad, n in (([-1], 1), ([1 << 32], 1), ([1.0], 1), ([1, 2], 3), ([[1, 2]], 3)):
        with pytest.raises(ValueError):
            check_tags(np.asarray(bad), n)
