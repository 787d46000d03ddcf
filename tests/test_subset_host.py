"""Search inside an id allow-list, host side (CPU): lmi_bucket_topk_subset and the
Python calls with `subset=` refuse what they do not take before any device call,
naming the subset; lmi_scan_subset_workspace_bytes is 0 for each refusal and
grows with nq * R; unknown ids raise KeyError, duplicates ValueError."""
import ctypes as C

import numpy as np
import pytest

from li import _lib, index, subset
from li.index import DeviceIndex, Searcher

U, I = _lib.LMI_E_UNSUPPORTED, _lib.LMI_E_INVALID


def _desc(d_pad=96, dtype=_lib.LMI_F16, **kw):
    d = _lib.IndexDesc()
    d.corpus = d.inv_norm = d.gpos = d.bucket_off = d.chunk_first = 64
    d.dtype, d.d, d.d_pad, d.n_rows = dtype, d_pad, d_pad, 100000
    d.n_buckets, d.chunk_rows, d.n_chunks, d.max_chunks = 4, 8192, 16, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


C_REFUSED = [  # (the message, the code, descriptor fields, n_sub, max_range, k, sub_rows)
    ("k <= 16", U, {}, 1000, 400, 17, 0),
    ("d_pad <= 992", U, dict(d_pad=1024), 1000, 400, 10, 0),
    ("fp16 storage", U, dict(dtype=_lib.LMI_F32), 1000, 400, 10, 0),
    ("fp16 storage", U, dict(dtype=_lib.LMI_I8), 1000, 400, 10, 0),
    ("fp16 storage", U, dict(dtype=_lib.LMI_MX4), 1000, 400, 10, 0),
    ("corpus32", U, dict(corpus32=64), 1000, 400, 10, 0),
    ("corpus32", U, dict(corpus64=64), 1000, 400, 10, 0),
    ("chunk_centroid", U, dict(chunk_centroid=64), 1000, 400, 10, 0),
    ("2 GiB", U, dict(chunk_rows=1 << 22), 1000, 400, 10, 0),
    ("multiple of 32", I, {}, 1000, 400, 10, 48),
    ("max_range", I, {}, 1000, 1001, 10, 0),
    ("max_range", I, {}, 100001, 400, 10, 0),
    ("k >= 1", I, {}, 1000, 400, 0, 0),
]


@pytest.mark.parametrize("msg,code,fields,n_sub,max_range,k,sub_rows", C_REFUSED)
def test_c_refusals_name_the_subset_and_the_reason(msg, code, fields, n_sub, max_range, k, sub_rows):
    lib, d = _lib.load(), _desc(**fields)
    rc = lib.lmi_bucket_topk_subset(C.byref(d), 64, 64, n_sub, max_range, 64, 3, d.d_pad, 64, 4, k, sub_rows, 64,
                                    1 << 30, 64, 64, 64, None)
    err = lib.lmi_last_error().decode()
    assert rc == code and msg in err and "subset" in err
    assert lib.lmi_scan_subset_workspace_bytes(C.byref(d), n_sub, max_range, 3, 4, k, sub_rows) == 0


def test_workspace_grows_with_pairs_and_with_smaller_slices():
    lib, d = _lib.load(), _desc(768)
    ws = lambda nq, R, rows=0: lib.lmi_scan_subset_workspace_bytes(C.byref(d), 20000, 8000, nq, R, 10, rows)  # noqa: E731
    assert 0 < ws(1, 4) < ws(100, 4) < ws(100, 8) < ws(10000, 8)
    assert ws(64, 4, 1024) < ws(64, 4, 256) < ws(64, 4, 32)
    assert lib.lmi_abi_version() == 13 == _lib.ABI_VERSION


def _stub(**kw):
    """A live one-GPU fp16 cosine index of 8 objects with no device behind it."""
    ix = object.__new__(DeviceIndex)
    ix.metric, ix.storage, ix.world, ix.d, ix.d_pad, ix.n_rows = "cosine", "f16", 1, 32, 32, 8
    ix.device, ix.chunk_centroid, ix.pos_to_id = "cpu", None, np.arange(10, 90, 10)
    ix.max_chunks, ix.chunk_rows = 1, 32
    for k, v in kw.items():
        setattr(ix, k, v)
    return ix


Q, CLS, IDS = np.zeros((2, 32), np.float32), np.zeros((2, 1), np.int32), np.array([30, 10])
topk = lambda ix, k=10, q=Q, **kw: index.bucket_topk(ix, q, CLS, k, subset=IDS, **kw)  # noqa: E731
lists = lambda s, q=Q, **kw: s.lists(None, q, 1, 10, classes=CLS, subset=IDS, **kw)  # noqa: E731
search = lambda s, q=Q, **kw: s.search(None, q, 1, classes=CLS, subset=IDS, **kw)  # noqa: E731
PY_REFUSED = {
    **{f"storage {st}": (dict(storage=st), lambda ix, s: topk(ix)) for st in ("i8", "mx4", "mx6", "f32", "f32x")},
    "corpus64": (dict(corpus64=object()), lambda ix, s: topk(ix)),
    "corpus64 lists": (dict(corpus64=object()), lambda ix, s: lists(s)),
    "corpus64 search": (dict(corpus64=object()), lambda ix, s: search(s)),
    "bucket of 2 GiB": (dict(max_chunks=1 << 10, chunk_rows=1 << 15), lambda ix, s: topk(ix)),
    "bucket of 2 GiB lists": (dict(max_chunks=1 << 10, chunk_rows=1 << 15), lambda ix, s: lists(s)),
    "metric l2": (dict(metric="l2"), lambda ix, s: topk(ix)),
    "metric ip search": (dict(metric="ip"), lambda ix, s: search(s)),
    "d_pad 1024": (dict(d=1024, d_pad=1024), lambda ix, s: topk(ix, q=np.zeros((2, 1024), np.float32))),
    "subcluster": (dict(chunk_centroid=object()), lambda ix, s: topk(ix)),
    "striped": (dict(world=2), lambda ix, s: topk(ix)),
    "k 17": ({}, lambda ix, s: topk(ix, k=17)),
    "want": ({}, lambda ix, s: topk(ix, want=CLS)),
    "avoid": ({}, lambda ix, s: topk(ix, avoid=CLS)),
    "few": ({}, lambda ix, s: topk(ix, few=True)),
    "seed": ({}, lambda ix, s: topk(ix, seed_round0=True)),
    "phase": ({}, lambda ix, s: topk(ix, phases=_lib.LMI_Q_PHASE_PLAN)),
    "join phase": ({}, lambda ix, s: topk(ix, phases=_lib.LMI_Q_PHASE_SCAN_JOIN)),
    "lists16": ({}, lambda ix, s: topk(ix, lists16=True)),
    "qmode f32": ({}, lambda ix, s: topk(ix, qmode=_lib.LMI_Q_F32)),
    "sub_rows 48": ({}, lambda ix, s: topk(ix, sub_rows=48)),
    "sub_rows alone": ({}, lambda ix, s: index.bucket_topk(ix, Q, CLS, 10, sub_rows=64)),
    "lists f64": ({}, lambda ix, s: lists(s, dist="f64")),
    "lists rerank": ({}, lambda ix, s: lists(s, rerank=16)),
    "lists want": ({}, lambda ix, s: lists(s, want=1)),
    "lists few": ({}, lambda ix, s: lists(s, few=True)),
    "lists lists16": ({}, lambda ix, s: lists(s, lists16=True)),
    "lists exchange": ({}, lambda ix, s: (setattr(s, "exchange", True), lists(s))),
    "lists not fp16-exact": ({}, lambda ix, s: lists(s, q=Q + np.float32(1e-9))),
    "search f64": ({}, lambda ix, s: search(s, dist="f64")),
    "search avoid": ({}, lambda ix, s: search(s, avoid=1)),
    "search k17 exact": ({}, lambda ix, s: search(s, k=17, semantics="exact")),
    "search not fp16-exact": ({}, lambda ix, s: search(s, q=Q + np.float32(1e-9))),
    "streamed": ({}, lambda ix, s: s.streamed(None, Q, 1, subset=IDS)),
    "graph": ({}, lambda ix, s: s.graph(None, Q, 1, subset=IDS)),
    "range_search": ({}, lambda ix, s: s.range_search(None, Q, 1, 0.5, classes=CLS, subset=IDS)),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
def test_python_refusals_come_before_any_device_call(what):
    fields, call = PY_REFUSED[what]
    ix = _stub(**fields)
    ix.bucket_off_local = None  # (nothing reaches the preparation's device half)
    with pytest.raises(ValueError, match="subset"):
        call(ix, Searcher(ix, None, exchange=False))


@pytest.mark.parametrize("ids,error", [([10, 35], KeyError), ([95], KeyError), ([20, 30, 20], ValueError),
                                       ([1.5], ValueError)])
def test_unknown_ids_are_a_key_error_and_duplicates_a_value_error(ids, error):
    ix = _stub()
    with pytest.raises(error):
        subset.prepare(ix, np.array(ids))
    with pytest.raises(error):
        index.bucket_topk(ix, Q, CLS, 10, subset=np.array(ids))
