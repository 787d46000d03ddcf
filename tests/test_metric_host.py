"""The metric scans' host side (CPU): lmi_bucket_topk_metric refuses what a
metric other than cosine does not offer with LMI_E_INVALID and a message that
names the metric, before any launch (dummy pointers, no device); the Python
interface raises ValueError before anything is allocated; the ABI version
stands; the workspace equals the cosine call's wherever both plans pick the
same kernel family."""
import ctypes as C

import numpy as np
import pytest

from li import _lib
from li.Baseline import Baseline
from li import index
from li.index import DeviceIndex, Searcher, check_metric

L2, IP = _lib.LMI_METRIC_L2, _lib.LMI_METRIC_IP


def _desc(d_pad=96, dtype=_lib.LMI_F16, **kw):
    d = _lib.IndexDesc()
    d.corpus = d.inv_norm = d.gpos = d.bucket_off = d.chunk_first = 64
    d.dtype, d.d, d.d_pad, d.n_rows = dtype, d_pad, d_pad, 1000
    d.n_buckets, d.chunk_rows, d.n_chunks, d.max_chunks = 4, 256, 4, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSED = [
    ("l2", L2, dict(dtype=_lib.LMI_I8), 10, _lib.LMI_Q_I8),
    ("ip", IP, dict(corpus32=64), 10, _lib.LMI_Q_F32),
    ("l2", L2, dict(corpus64=64), 10, _lib.LMI_Q_F32),
    ("ip", IP, dict(chunk_centroid=64), 10, _lib.LMI_Q_F16),
    ("l2", L2, {}, 17, _lib.LMI_Q_F16),
    ("ip", IP, {}, 10, _lib.LMI_Q_F16 | _lib.LMI_Q_SEED_ROUND0),
    ("l2", L2, {}, 10, _lib.LMI_Q_F16 | _lib.LMI_Q_PHASE_SCAN_JOIN),
    ("ip", IP, dict(d_pad=1024), 10, _lib.LMI_Q_F16),
    ("unknown metric 7", 7, {}, 10, _lib.LMI_Q_F16),
]


@pytest.mark.parametrize("name,metric,fields,k,qmode", REFUSED)
def test_c_refusals_name_the_metric(name, metric, fields, k, qmode):
    lib = _lib.load()
    rc = lib.lmi_bucket_topk_metric(C.byref(_desc(**fields)), metric, 64, 8, fields.get("d_pad", 96), 64, 2, k, qmode,
                                    64, 64, 64, 64, 1 << 30, None)
    assert rc == _lib.LMI_E_INVALID and name in lib.lmi_last_error().decode()
    assert lib.lmi_scan_metric_workspace_bytes(C.byref(_desc(**fields)), metric, 8, 2, k, qmode) == 0


def test_abi_version_stands():
    assert _lib.load().lmi_abi_version() == 13 == _lib.ABI_VERSION


@pytest.mark.parametrize("d_pad,dtype,qmode,k", [(768, _lib.LMI_F16, _lib.LMI_Q_F16, 10), (768, _lib.LMI_F16, _lib.LMI_Q_F32, 16),
                                                 (96, _lib.LMI_F16, _lib.LMI_Q_F16, 16), (32, _lib.LMI_F32, _lib.LMI_Q_F32, 1),
                                                 (992, _lib.LMI_F32, _lib.LMI_Q_F32, 10)])
def test_workspace_equals_the_cosine_call(d_pad, dtype, qmode, k):
    lib, d = _lib.load(), _desc(d_pad, dtype)
    want = lib.lmi_scan_workspace_bytes(C.byref(d), 100, 3, k, qmode)
    assert want > 0 and all(lib.lmi_scan_metric_workspace_bytes(C.byref(d), m, 100, 3, k, qmode) == want
                            for m in (_lib.LMI_METRIC_COSINE, L2, IP))


def test_workspace_of_the_rerouted_ring_shapes():
    """d_pad 768, fp16 math, k = 11..16: the cosine plan's 15- and 16-entry
    ring lists go to the general kernel, whose 64-query tiles need more tile slots."""
    lib, d = _lib.load(), _desc(768)
    for k in (12, 16):
        assert lib.lmi_scan_metric_workspace_bytes(C.byref(d), L2, 100, 3, k, _lib.LMI_Q_F16) > 0


@pytest.mark.parametrize("kw", [dict(storage="i8"), dict(storage="f32x"), dict(subcluster=True), dict(capacity=100),
                                dict(world=2), dict(tags=np.zeros(8, np.uint32)), dict(metric="hamming")])
def test_construction_refusals_come_before_any_allocation(kw):
    kw = dict(dict(metric="l2"), **kw)
    with pytest.raises(ValueError, match="metric"):
        DeviceIndex(np.zeros((8, 32), np.float16), np.zeros(8, np.int64), 2, device="cuda:0", **kw)


def _stub(metric="l2"):
    """A live one-GPU fp16 index of that metric with no device behind it:
    every refusal below must come before anything touches one."""
    ix = object.__new__(DeviceIndex)
    ix.metric, ix.storage, ix.world, ix.d, ix.d_pad, ix.n_rows = metric, "f16", 1, 32, 32, 8
    ix.device, ix.chunk_centroid = "cpu", None
    return ix


Q, CLS = np.zeros((2, 32), np.float32), np.zeros((2, 1), np.int32)
CALLS = {
    "add": lambda ix, s: ix.add(Q.astype(np.float16), [0, 0]),
    "remove": lambda ix, s: ix.remove([1]),
    "relabel": lambda ix, s: ix.relabel(np.zeros(8, np.int64)),
    "reserve": lambda ix, s: ix.reserve(16),
    "quantized": lambda ix, s: ix.quantized(),
    "bucket_topk want": lambda ix, s: index.bucket_topk(ix, Q, CLS, 10, want=CLS),
    "bucket_topk avoid": lambda ix, s: index.bucket_topk(ix, Q, CLS, 10, avoid=CLS),
    "bucket_topk k17": lambda ix, s: index.bucket_topk(ix, Q, CLS, 17),
    "bucket_topk_f64": lambda ix, s: index.bucket_topk_f64(ix, Q, CLS, 10),
    "bucket_range": lambda ix, s: index.bucket_range(ix, Q, CLS, 0.5),
    "lists f64": lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, dist="f64"),
    "lists rerank": lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, dist="f64", rerank=16),
    "lists want": lambda ix, s: s.lists(None, Q, 1, 10, classes=CLS, want=1),
    "lists k17": lambda ix, s: s.lists(None, Q, 1, 17, classes=CLS),
    "search f64": lambda ix, s: s.search(None, Q, 1, classes=CLS, dist="f64"),
    "search avoid": lambda ix, s: s.search(None, Q, 1, classes=CLS, avoid=1),
    "search k17": lambda ix, s: s.search(None, Q, 1, k=17, classes=CLS, semantics="exact"),
    "range_search": lambda ix, s: s.range_search(None, Q, 1, 0.5, classes=CLS),
    "streamed": lambda ix, s: s.streamed(Q, Q, 1),
    "graph": lambda ix, s: s.graph(Q, Q, 1),
    "exchange": lambda ix, s: Searcher(ix, None, exchange=True),
}


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("what", sorted(CALLS))
def test_python_refusals_at_their_call_sites(what, metric):
    ix = _stub(metric)
    with pytest.raises(ValueError, match=f"metric '{metric}'"):
        CALLS[what](ix, Searcher(ix, None, exchange=False))


@pytest.mark.parametrize("kw", [dict(capacity=100), dict(tags=np.zeros(8, np.uint32)), dict(storage="i8"),
                                dict(storage="f32x"), dict(storage="i8", keep_rows=True, rerank=12)])
def test_attach_refusals_come_before_the_build(kw):
    from li.LearnedIndex import LearnedIndex
    with pytest.raises(ValueError, match="metric 'ip'"):
        LearnedIndex().attach(None, None, None, metric="ip", **kw)
    with pytest.raises(ValueError, match="metric must be"):
        LearnedIndex().attach(None, None, None, metric="dot")


def test_metric_names():
    check_metric("cosine", "anything")
    with pytest.raises(ValueError, match="metric"):
        Baseline(metric="dot")
