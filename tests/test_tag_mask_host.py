"""All-of / none-of filtered search and tag edits, the parts that need no
device: the eligible counts with `avoid` against a numpy loop, ids_with, the
want / avoid -> (value, mask) conversion and its refusals, the three new C
entries' declarations against the header, and their refusals before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from li import _lib
from li.index import DeviceIndex, Searcher, eligible_counts, value_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lmi_bucket_topk_masked", "lmi_bucket_range_masked", "lmi_index_edit_tags")


def _desc(dtype=None, d_pad=768, **kw):
    d = _lib.IndexDesc()
    d.dtype = _lib.LMI_F16 if dtype is None else dtype
    d.d, d.d_pad, d.n_rows, d.n_buckets = d_pad, d_pad, 10**6, 122
    d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
    for name, v in kw.items():          # (dummy addresses: never dereferenced)
        setattr(d, name, v)
    return d


def _message(lib):
    msg = lib.lmi_last_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


# ---- eligible counts, ids_with -----------------------------------------------------------
def test_eligible_counts_with_avoid_against_a_loop():
    rng = np.random.default_rng(31)
    sizes = np.array([0, 5, 1, 0, 40, 17, 0])
    off = np.concatenate([[0], np.cumsum(sizes)])
    tags = rng.integers(0, 16, int(sizes.sum())).astype(np.uint32)
    tags[::7] |= np.uint32(1 << 31)
    for w, a in ((0, 0), (1, 0), (0, 1), (1, 2), (0, 7), (5, 10), (1 << 31, 1), (0, 1 << 31), (15, 0), (0, 15)):
        want = [sum(1 for t in tags[off[c]:off[c + 1]] if (int(t) & w) == w and (int(t) & a) == 0)
                for c in range(sizes.size)]
        got = eligible_counts(tags, off, w, a)
        assert got.dtype == np.int64 and got.tolist() == want, (w, a)
    assert np.array_equal(eligible_counts(tags, off, 3), eligible_counts(tags, off, 3, 0))


class _HostIndex:
    """The host tables ids_with and eligible_bucket_size read, without a device."""
    ids_with = DeviceIndex.ids_with
    tags_version = 0

    def __init__(self, tags, ids, off):
        self.tags_by_pos, self.pos_to_id = tags, ids
        self.layout = type("L", (), dict(bucket_off=off))()


def test_ids_with_reads_the_host_table_in_position_order():
    rng = np.random.default_rng(32)
    n = 500
    tags = rng.integers(0, 8, n).astype(np.uint32)
    ids = (rng.permutation(n) + 10).astype(np.int64)
    ix = _HostIndex(tags, ids, np.array([0, n]))
    for w, a in ((0, 0), (1, 0), (0, 1), (2, 5), (7, 0), (0, 7), (1 << 29, 0)):
        exp = [int(i) for i, t in zip(ids, tags) if (int(t) & w) == w and (int(t) & a) == 0]
        got = ix.ids_with(want=w, avoid=a)
        assert got.dtype == np.int64 and got.tolist() == exp, (w, a)
    assert ix.ids_with().tolist() == ids.tolist()
    for bad in (dict(want=1, avoid=1), dict(want=-1), dict(avoid=1 << 32), dict(want=1.0), dict(want=True)):
        with pytest.raises(ValueError):
            ix.ids_with(**bad)
    ix.tags_by_pos = None
    with pytest.raises(ValueError):
        ix.ids_with(want=1)


def test_the_searchers_count_cache_is_per_pair_and_follows_tags_version():
    rng = np.random.default_rng(33)
    off = np.array([0, 30, 30, 100])
    tags = rng.integers(0, 8, 100).astype(np.uint32)
    ix = _HostIndex(tags.copy(), np.arange(100), off)
    s = object.__new__(Searcher)
    s.index = ix
    first = s.eligible_bucket_size(1, 2)
    assert first.tolist() == eligible_counts(tags, off, 1, 2).tolist()
    assert s.eligible_bucket_size(1, 2) is first                      # cached per pair
    assert s.eligible_bucket_size(1).tolist() == eligible_counts(tags, off, 1).tolist()
    assert s.eligible_bucket_size(0, 1).tolist() == eligible_counts(tags, off, 0, 1).tolist()
    ix.tags_by_pos = tags | np.uint32(2)                              # an edit: every row now has bit 1
    ix.tags_version += 1
    assert s.eligible_bucket_size(1, 2).tolist() == [0, 0, 0]


# ---- want / avoid -> (value, mask) -----------------------------------------------------------
def test_value_mask_conversion_and_its_refusals():
    v, m = value_mask(5, 2)
    assert (int(v), int(m)) == (5, 7)
    v, m = value_mask(0, 1 << 31)
    assert (int(v), int(m)) == (0, 1 << 31)
    w = np.array([0, 1, 4, 1 << 31, 0], np.uint32)
    a = np.array([0, 2, 3, 1, 0xFFFFFFFF], np.uint32)
    v, m = value_mask(w, a)
    assert v.dtype == m.dtype == np.uint32
    assert v.tolist() == w.tolist() and m.tolist() == [0, 3, 7, (1 << 31) | 1, 0xFFFFFFFF]
    # the kernels' one test is the two-part predicate, on every tag word of a byte
    t = np.arange(256, dtype=np.uint32)
    for wi, ai in ((0, 0), (1, 2), (4, 3), (0, 7), (5, 0)):
        vi, mi = value_mask(wi, ai)
        assert np.array_equal((t & mi) == vi, ((t & wi) == wi) & ((t & ai) == 0))
    with pytest.raises(ValueError, match="both wanted and avoided"):
        value_mask(5, 4)
    with pytest.raises(ValueError, match="query 2"):
        value_mask(np.array([0, 1, 6, 0], np.uint32), np.array([7, 2, 2, 0], np.uint32))


# ---- the C entries ---------------------------------------------------------------------------
def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    m = re.search(r"^(\w[\w\s\*]*?)\b" + name + r"\(([^)]*)\);", hdr, flags=re.M)
    assert m, name
    return m.group(1).strip(), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype(decl):
    if "*" in decl:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}[
        decl.replace("const ", "").split()[0]]


@pytest.mark.parametrize("name", NEW)
def test_lib_declares_the_new_entries_as_the_header_does(name):
    lib = _lib.load()
    assert name in _lib.EXPORTS
    ret, args = _header_args(name)
    res, argtypes = _lib._SIGNATURES[name]
    assert res is _ctype(ret)
    assert len(argtypes) == len(args), (name, args)
    for got, decl in zip(argtypes, args):
        exp = _ctype(decl)
        assert got is exp or (exp is C.c_void_p and got == C.POINTER(_lib.IndexDesc)), (name, decl)
    assert getattr(lib, name).argtypes == list(argtypes)
    assert lib.lmi_abi_version() == 13                                # additions only
    # the masked entries take their `want` sibling's arguments plus mask and the two host copies
    if name != "lmi_index_edit_tags":
        sib = _header_args({"lmi_bucket_topk_masked": "lmi_bucket_topk_tagged",
                            "lmi_bucket_range_masked": "lmi_bucket_range"}[name])[1]
        assert [a.split()[-1].lstrip("*") for a in args] == \
            ["idx", "tags", "value", "mask", "host_value", "host_mask"] + [a.split()[-1].lstrip("*") for a in sib[3:]]


def _topk(lib, d, *, tags=4096, value=4096, mask=4096, hv=None, hm=None, nq=8, k=10, qmode=0):
    return lib.lmi_bucket_topk_masked(C.byref(d), tags, value, mask, hv, hm, 4096, nq, d.d, 4096, 2, k, qmode,
                                      4096, 4096, 4096, 4096, 1 << 40, None)


def _range(lib, d, *, tags=4096, value=4096, mask=4096, hv=None, hm=None, nq=8, qmode=0, cap=256):
    return lib.lmi_bucket_range_masked(C.byref(d), tags, value, mask, hv, hm, 4096, nq, d.d, 4096, 2, qmode,
                                       4096, cap, 4096, 4096, 4096, 4096, 1 << 40, None)


def _words(*w):
    a = np.array(w, np.uint32)
    return a, a.ctypes.data


@pytest.mark.parametrize("call,fn", [(_topk, "lmi_bucket_topk_masked"), (_range, "lmi_bucket_range_masked")])
def test_masked_entries_refuse_before_any_launch(call, fn):
    lib = _lib.load()
    good_v, pv = _words(*([1] * 8))
    good_m, pm = _words(*([3] * 8))
    bad_v, pbv = _words(1, 1, 1, 1, 1, 5, 1, 1)                       # query 5 wants bit 2, which its mask lacks
    cases = [
        ("null tags", {}, dict(tags=None)),
        ("null value", {}, dict(value=None)),
        ("null mask", {}, dict(mask=None)),
        ("value outside mask", {}, dict(hv=pbv, hm=pm)),
        ("host value without host mask", {}, dict(hv=pv)),
        ("host mask without host value", {}, dict(hm=pm)),
        ("corpus32", dict(corpus32=4096), {}),
        ("chunk_centroid", dict(chunk_centroid=4096), {}),
        ("scan phase", {}, dict(qmode=_lib.LMI_Q_PHASE_SCAN)),
        ("seed", {}, dict(qmode=_lib.LMI_Q_SEED_ROUND0)),
    ]
    if call is _topk:
        cases.append(("k > LMI_MAX_K", {}, dict(k=_lib.LMI_MAX_K + 1)))
    else:
        cases.append(("pair_cap", {}, dict(cap=0)))
    for what, desc_kw, call_kw in cases:
        rc = call(lib, _desc(**desc_kw), **call_kw)
        assert rc == _lib.LMI_E_INVALID, what
        assert "lmi_bucket_" in _message(lib), (what, _message(lib))
    rc = call(lib, _desc(), hv=pbv, hm=pm)
    assert rc == _lib.LMI_E_INVALID and fn in _message(lib) and "query 5" in _message(lib)
    # (sound words pass that check: the next refusal is another one)
    rc = call(lib, _desc(corpus32=4096), hv=pv, hm=pm)
    assert rc == _lib.LMI_E_INVALID and "corpus32" in _message(lib)
    del good_v, good_m, bad_v


def test_the_want_entries_still_refuse_as_before():
    lib = _lib.load()
    d = _desc()
    rc = lib.lmi_bucket_topk_tagged(C.byref(d), 4096, None, 4096, 8, d.d, 4096, 2, 10, 0, 4096, 4096, 4096, 4096,
                                    1 << 40, None)
    assert rc == _lib.LMI_E_INVALID and "lmi_bucket_topk_tagged" in _message(lib)
    rc = lib.lmi_bucket_range(C.byref(d), 4096, None, 4096, 8, d.d, 4096, 2, 0, 4096, 256, 4096, 4096, 4096, 4096,
                              1 << 40, None)
    assert rc == _lib.LMI_E_INVALID and "lmi_bucket_range" in _message(lib)


def test_edit_tags_entry_refuses_without_a_device():
    lib = _lib.load()
    assert lib.lmi_index_edit_tags(None, 10, None, None, None, 0, None, None) == _lib.LMI_OK   # n = 0: a no-op
    for what, kw in (("null tags", dict(tags=None)), ("null rows", dict(rows=None)), ("null clear", dict(clear=None)),
                     ("null set", dict(set=None)), ("null status", dict(status=None)), ("n < 0", dict(n=-1)),
                     ("n_rows < 0", dict(n_rows=-1))):
        a = dict(tags=4096, n_rows=10, rows=4096, clear=4096, set=4096, n=3, status=4096)
        a.update(kw)
        rc = lib.lmi_index_edit_tags(a["tags"], a["n_rows"], a["rows"], a["clear"], a["set"], a["n"], a["status"],
                                     None)
        assert rc == _lib.LMI_E_INVALID, what
        assert "lmi_index_edit_tags" in _message(lib), what
