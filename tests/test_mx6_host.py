"""The 6-bit storage's refusals and its plan, on the CPU: every refusal names the
storage ("mx6" in Python's ValueError, LMI_MX6 with LMI_E_INVALID in C) and
comes before anything is allocated or launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from li import _lib
from li.index import DeviceIndex, Searcher, bucket_topk, bucket_topk_f64, i8_lists16

X = np.zeros((40, 768), np.float16)
LAB = np.arange(40) % 4


def _desc(dtype=_lib.LMI_MX6, d_pad=768, **kw):
    d = _lib.IndexDesc()
    d.dtype, d.d, d.d_pad, d.n_rows, d.n_buckets = dtype, d_pad, d_pad, 10**6, 122
    d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _refused(rc):
    assert rc in (_lib.LMI_E_INVALID, -_lib.LMI_E_INVALID)
    assert "LMI_MX6" in _lib.load().lmi_last_error().decode()


@pytest.mark.parametrize("k,lists16", [(1, False), (10, False), (11, True), (16, True)])
def test_plan_family_and_workspace(k, lists16):
    lib = _lib.load()
    args = (C.byref(_desc()), 100, 4, k, _lib.LMI_Q_MX6)
    if lists16:
        _refused(lib.lmi_scan_family(C.byref(_desc()), k, _lib.LMI_Q_MX6, 0))
        assert lib.lmi_scan_workspace_bytes(*args) == 0
        with i8_lists16():
            assert lib.lmi_scan_family(C.byref(_desc()), k, _lib.LMI_Q_MX6, 0) == 5
            ws16 = lib.lmi_scan_workspace_bytes(*args)
        # the partial lists follow the setting: 16 entries a (pair, chunk) where k <= 10 takes 10
        assert ws16 > lib.lmi_scan_workspace_bytes(C.byref(_desc()), 100, 4, 10, _lib.LMI_Q_MX6)
    else:
        assert lib.lmi_scan_family(C.byref(_desc()), k, _lib.LMI_Q_MX6, 0) == 5
        assert lib.lmi_scan_workspace_bytes(*args) > 100 * 608   # the query records alone


@pytest.mark.parametrize("desc,k,qmode", [
    (_desc(d_pad=736), 10, _lib.LMI_Q_MX6),                       # d_pad != 768
    (_desc(d_pad=96), 10, _lib.LMI_Q_MX6),
    (_desc(), 10, _lib.LMI_Q_F16),                                # the storage without its query class
    (_desc(_lib.LMI_F16), 10, _lib.LMI_Q_MX6),                    # and the reverse
    (_desc(), 10, _lib.LMI_Q_MX4),                                # the 4-bit storage's class
    (_desc(), 17, _lib.LMI_Q_MX6),
    (_desc(), 10, _lib.LMI_Q_MX6 | _lib.LMI_Q_SEED_ROUND0),
    (_desc(), 10, _lib.LMI_Q_MX6 | _lib.LMI_Q_PHASE_SCAN_JOIN),
    (_desc(chunk_centroid=C.cast(1 << 12, C.c_void_p)), 10, _lib.LMI_Q_MX6),
    (_desc(corpus64=C.cast(1 << 12, C.c_void_p)), 10, _lib.LMI_Q_MX6),
], ids=["d736", "d96", "q_f16", "rows_f16", "q_mx4", "k17", "seed", "join", "subcluster", "corpus64"])
def test_c_refusals(desc, k, qmode):
    lib = _lib.load()
    rc = lib.lmi_bucket_topk(C.byref(desc), None, 8, 768, None, 2, k, qmode, None, None, None, None, 0, None)
    assert rc == _lib.LMI_E_INVALID and "MX6" in lib.lmi_last_error().decode()
    assert lib.lmi_scan_family(C.byref(desc), k, qmode, 0) == -_lib.LMI_E_INVALID
    assert lib.lmi_scan_workspace_bytes(C.byref(desc), 8, 2, k, qmode) == 0


def test_c_refuses_tags_metric_and_the_other_entries():
    lib = _lib.load()
    w = np.zeros(8, np.uint32)
    p = w.ctypes.data
    _refused(lib.lmi_bucket_topk_masked(C.byref(_desc()), p, p, p, None, None, None, 8, 768, None, 2, 10,
                                        _lib.LMI_Q_MX6, None, None, None, None, 0, None))
    assert lib.lmi_scan_tagged_workspace_bytes(C.byref(_desc()), 8, 2, 10, _lib.LMI_Q_MX6) == 0
    _refused(lib.lmi_bucket_topk_metric(C.byref(_desc()), _lib.LMI_METRIC_L2, None, 8, 768, None, 2, 10,
                                        _lib.LMI_Q_MX6, None, None, None, None, 0, None))
    assert lib.lmi_scan_f64_workspace_bytes(C.byref(_desc()), 8, 2, 10, _lib.LMI_Q_MX6) == 0
    assert "LMI_MX6" in lib.lmi_last_error().decode()
    # the quantiser's own, as lmi_quantize_rows_mx4: d_pad no multiple of 64, a bad dtype, ld < d
    for dtype, ld, d_pad in ((_lib.LMI_F16, 96, 96), (_lib.LMI_MX6, 768, 768), (_lib.LMI_F32, 700, 768)):
        assert lib.lmi_quantize_rows_mx6(p, dtype, 1, ld, d_pad, d_pad, None, p, p, p, None) == _lib.LMI_E_INVALID
        assert "mx6" in lib.lmi_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(data=np.zeros((40, 96), np.float16)), dict(data=np.zeros((40, 800), np.float16)),
    dict(tags=np.zeros(40, np.uint32)), dict(metric="l2"), dict(metric="ip"), dict(capacity=64),
    dict(subcluster=True), dict(world=2),
], ids=["d96", "d800", "tags", "l2", "ip", "capacity", "subcluster", "world2"])
def test_build_refusals_name_the_storage(kw):
    kw = dict(kw)
    with pytest.raises(ValueError, match="mx6"):
        DeviceIndex(kw.pop("data", X), LAB, 4, storage="mx6", device="cuda", **kw)


def _index():
    """A DeviceIndex of storage "mx6" with no device behind it: what the entry
    points read before they refuse."""
    ix = object.__new__(DeviceIndex)
    ix.storage, ix.metric, ix.world, ix.d, ix.d_pad, ix.device = "mx6", "cosine", 1, 768, 768, torch.device("cpu")
    return ix


Q, CLS = torch.zeros((2, 768)), torch.zeros((2, 2), dtype=torch.int32)
REFUSED = {
    "lists_f64": lambda s: s.lists(None, Q, 2, 10, classes=CLS, dist="f64"),
    "lists_k16": lambda s: s.lists(None, Q, 2, 16, classes=CLS),         # 11..16 entries: lists16=True alone
    "lists_k17": lambda s: s.lists(None, Q, 2, 17, classes=CLS, lists16=True),
    "lists_want": lambda s: s.lists(None, Q, 2, 10, classes=CLS, want=1),
    "lists_avoid": lambda s: s.lists(None, Q, 2, 10, classes=CLS, avoid=1, lists16=True),
    "search_want": lambda s: s.search(None, Q, 2, classes=CLS, want=1),
    "search_avoid": lambda s: s.search(None, Q, 2, classes=CLS, avoid=np.ones(2, np.int64), semantics="exact"),
    "search_f64": lambda s: s.search(None, Q, 2, classes=CLS, dist="f64"),
    "search_k_round16": lambda s: s.search(None, Q, 2, classes=CLS, k_round=16),
    "topk_k16": lambda s: bucket_topk(s.index, Q, CLS, 16),
    "topk_k17": lambda s: bucket_topk(s.index, Q, CLS, 17, lists16=True),
    "topk_want": lambda s: bucket_topk(s.index, Q, CLS, 10, want=CLS[:, 0]),
    "topk_f64": lambda s: bucket_topk_f64(s.index, Q, CLS, 10),
    "edit_tags": lambda s: s.index.edit_tags([1], set_bits=1),
    "set_tags": lambda s: s.index.set_tags([1], 1),
    "streamed": lambda s: s.streamed(None, Q, 2),
    "graph": lambda s: s.graph(None, Q, 2),
    "range": lambda s: s.range_search(None, Q, 2, 0.5, classes=CLS),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_search_refusals_name_the_storage(name):
    with pytest.raises(ValueError, match="mx6"):
        REFUSED[name](Searcher(_index(), None, exchange=False))


def test_rerank_needs_kept_rows():
    s = Searcher(_index(), None, exchange=False)
    with pytest.raises(ValueError, match="keeps no fp16 rows"):
        s.lists(None, Q, 2, 10, classes=CLS, dist="f64", rerank=16)
    with pytest.raises(ValueError, match="dist='f64'"):
        s.index.rows16 = Q
        s.lists(None, Q, 2, 10, classes=CLS, rerank=16)
