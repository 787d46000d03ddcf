"""The few-query scan's host side (CPU): lmi_bucket_topk_few refuses what it
does not take before any launch (placeholder pointers, no device) with a message
that names the reason, lmi_scan_few_workspace_bytes is 0 for each refusal and
grows with nq and with smaller slices, and the ABI version stands."""
import ctypes as C

import pytest

from li import _lib

U, I = _lib.LMI_E_UNSUPPORTED, _lib.LMI_E_INVALID


def _desc(d_pad=96, dtype=_lib.LMI_F16, **kw):
    d = _lib.IndexDesc()
    d.corpus = d.inv_norm = d.gpos = d.bucket_off = d.chunk_first = 64
    d.dtype, d.d, d.d_pad, d.n_rows = dtype, d_pad, d_pad, 100000
    d.n_buckets, d.chunk_rows, d.n_chunks, d.max_chunks = 4, 8192, 16, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSED = [  # (the message, the code, descriptor fields, nq, R, k, few_rows)
    ("256 pairs", U, {}, 65, 4, 10, 0),
    ("k <= 16", U, {}, 1, 4, 17, 0),
    ("d_pad <= 992", U, dict(d_pad=1024), 1, 4, 10, 0),
    ("fp16 storage", U, dict(dtype=_lib.LMI_F32), 1, 4, 10, 0),
    ("fp16 storage", U, dict(dtype=_lib.LMI_I8), 1, 4, 10, 0),
    ("corpus32", U, dict(corpus32=64), 1, 4, 10, 0),
    ("corpus32", U, dict(corpus64=64), 1, 4, 10, 0),
    ("chunk_centroid", U, dict(chunk_centroid=64), 1, 4, 10, 0),
    ("multiple of 32", I, {}, 1, 4, 10, 48),
    ("multiple of 32", I, {}, 1, 4, 10, -32),
]


@pytest.mark.parametrize("msg,code,fields,nq,R,k,few_rows", REFUSED)
def test_c_refusals_name_the_reason(msg, code, fields, nq, R, k, few_rows):
    lib, d = _lib.load(), _desc(**fields)
    rc = lib.lmi_bucket_topk_few(C.byref(d), 64, nq, d.d_pad, 64, R, k, few_rows, 64, 1 << 30, 64, 64, 64, None)
    assert rc == code and msg in lib.lmi_last_error().decode()
    assert lib.lmi_scan_few_workspace_bytes(C.byref(d), nq, R, k, few_rows) == 0


def test_join_workgroups_are_refused():
    lib = _lib.load()
    lib.lmi_scan_set_join_workgroups(8)
    try:
        rc = lib.lmi_bucket_topk_few(C.byref(_desc()), 64, 1, 96, 64, 4, 10, 0, 64, 1 << 30, 64, 64, 64, None)
        assert rc == I and "join" in lib.lmi_last_error().decode()
    finally:
        lib.lmi_scan_set_join_workgroups(0)


def test_workspace_grows_with_nq_and_with_smaller_slices():
    lib, d = _lib.load(), _desc(768)
    ws = lambda nq, rows: lib.lmi_scan_few_workspace_bytes(C.byref(d), nq, 4, 10, rows)  # noqa: E731
    assert 0 < ws(1, 0) < ws(16, 0) < ws(64, 0)
    assert ws(4, 1024) < ws(4, 256) < ws(4, 32)
    assert lib.lmi_abi_version() == 13 == _lib.ABI_VERSION


# ---------------------------------------------------------------------------
# the refusals that exist in Python alone (the C entry has no qmode, metric or
# tag argument): ValueError before anything touches a device
# ---------------------------------------------------------------------------
import numpy as np  # noqa: E402

from li import index  # noqa: E402
from li.index import DeviceIndex, Searcher  # noqa: E402


def _stub(**kw):
    """A live one-GPU fp16 cosine index with no device behind it."""
    ix = object.__new__(DeviceIndex)
    ix.metric, ix.storage, ix.world, ix.d, ix.d_pad, ix.n_rows = "cosine", "f16", 1, 32, 32, 8
    ix.device, ix.chunk_centroid = "cpu", None
    for k, v in kw.items():
        setattr(ix, k, v)
    return ix


Q, CLS = np.zeros((2, 32), np.float32), np.zeros((2, 1), np.int32)
topk = lambda ix, k=10, cls=CLS, q=Q, **kw: index.bucket_topk(ix, q, cls, k, few=True, **kw)  # noqa: E731
PY_REFUSED = {
    "metric l2": (dict(metric="l2"), lambda ix, s: topk(ix)),
    "metric ip lists": (dict(metric="ip"), lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few=True)),
    "storage i8": (dict(storage="i8"), lambda ix, s: topk(ix)),
    "storage f32": (dict(storage="f32"), lambda ix, s: topk(ix)),
    "d_pad 1024": (dict(d=1024, d_pad=1024), lambda ix, s: topk(ix, q=np.zeros((2, 1024), np.float32))),
    "subcluster": (dict(chunk_centroid=object()), lambda ix, s: topk(ix)),
    "striped": (dict(world=2), lambda ix, s: topk(ix)),
    "257 pairs": ({}, lambda ix, s: topk(ix, cls=np.zeros((2, 129), np.int32))),
    "k 17": ({}, lambda ix, s: topk(ix, k=17)),
    "want": ({}, lambda ix, s: topk(ix, want=CLS)),
    "avoid": ({}, lambda ix, s: topk(ix, avoid=CLS)),
    "seed": ({}, lambda ix, s: topk(ix, seed_round0=True)),
    "phase": ({}, lambda ix, s: topk(ix, phases=_lib.LMI_Q_PHASE_PLAN)),
    "lists16": ({}, lambda ix, s: topk(ix, lists16=True)),
    "qmode f32": ({}, lambda ix, s: topk(ix, qmode=_lib.LMI_Q_F32)),
    "few_rows 48": ({}, lambda ix, s: topk(ix, few_rows=48)),
    "few_rows alone": ({}, lambda ix, s: index.bucket_topk(ix, Q, CLS, 10, few_rows=64)),
    "few_rows alone lists16": ({}, lambda ix, s: index.bucket_topk(ix, Q, CLS, 10, lists16=True, few_rows=64)),
    "family tagged": ({}, lambda ix, s: index.scan_family(ix, 10, tagged=True, few=True)),
    "lists f64": ({}, lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few=True, dist="f64")),
    "lists rerank": ({}, lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few=True, rerank=16)),
    "lists want": ({}, lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few=True, want=1)),
    "lists lists16": ({}, lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few=True, lists16=True)),
    "lists few_rows alone": ({}, lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, few_rows=64)),
    "lists exchange": ({}, lambda ix, s: (setattr(s, "exchange", True), s.lists(None, Q, 1, 10, classes=CLS, few=True))),
    "lists not fp16-exact": ({}, lambda ix, s: s.lists(None, Q + np.float32(1e-9), 1, 10, classes=CLS, few=True)),
    "search f64": ({}, lambda ix, s: s.search(None, Q, 1, classes=CLS, few=True, dist="f64")),
    "search lists16": ({}, lambda ix, s: s.search(None, Q, 1, classes=CLS, few=True, lists16=True)),
    "search avoid": ({}, lambda ix, s: s.search(None, Q, 1, classes=CLS, few=True, avoid=1)),
    "search k17 exact": ({}, lambda ix, s: s.search(None, Q, 1, k=17, classes=CLS, few=True, semantics="exact")),
    "search not fp16-exact": ({}, lambda ix, s: s.search(None, Q + np.float32(1e-9), 1, classes=CLS, few=True)),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
def test_python_refusals_come_before_any_launch(what):
    fields, call = PY_REFUSED[what]
    ix = _stub(**fields)
    with pytest.raises(ValueError, match="few"):
        call(ix, Searcher(ix, None, exchange=False))
