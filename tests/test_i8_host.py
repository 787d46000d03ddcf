"""The 8-bit storage (LMI_I8), the parts that need no device: the numpy
restatement's own quality against the float64 cosine order, every refusal of
the C ABI (before any launch, with a message that names the storage) and the
workspace size of an i8 descriptor."""
import ctypes as C

import numpy as np
import pytest

import i8_cases as I8
from li import _lib


# ---- the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 96, 200, 992])
def test_restatement_keeps_the_float64_cosine_order(d):
    """Gaussian fp16-exact rows, 2 100 rows x 300 queries: the mean top-10
    overlap of the i8 order with the float64 cosine order is at least 0.95
    (I8.distances asserts |acc| < 2^24 and p >= 2^-29 on the way)."""
    rng = np.random.default_rng(5302 + d)
    x = rng.standard_normal((2100, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((300, d)).astype(np.float16).astype(np.float32)
    cx, ix = I8.quantize(x)
    cq, iq = I8.quantize(q)
    assert cx.shape == (2100, I8.d_pad_of(d)) and not cx[:, d:].any() and np.abs(cx.astype(int)).max() == 127
    d8 = I8.distances(cq, iq, cx, ix)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    d64 = 1.0 - (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (x64 / np.linalg.norm(x64, axis=1, keepdims=True)).T
    pos = np.arange(2100)
    overlap = np.mean([len(set(np.lexsort((pos, d8[i]))[:10]) & set(np.lexsort((pos, d64[i]))[:10])) / 10.0
                       for i in range(300)])
    print(f"d={d}: mean top-10 overlap {overlap:.4f}")
    assert overlap >= 0.95


def test_restatement_edge_rows():
    """Zero, tiny and NaN rows quantise to zero codes and inv = 1; s = 1 rounds
    the half-way values to even; float64 input is rounded to float32 first."""
    v = np.zeros((5, 40), np.float32)
    v[1, 3] = 2.0 ** -101
    v[2, 5] = np.nan
    v[2, 6] = 1.0
    v[3, :6] = [127.0, 0.5, 1.5, 2.5, -0.5, -126.5]
    v[4, :2] = [2.0 ** -100, -(2.0 ** -100)]
    c, inv = I8.quantize(v)
    assert c.shape == (5, 64) and not c[:3].any() and inv[:3].tolist() == [1.0, 1.0, 1.0]
    assert c[3, :6].tolist() == [127, 0, 2, 2, 0, -126]
    assert c[4, :3].tolist() == [127, -127, 0]
    assert inv[4] == np.float32(1.0 / np.sqrt(np.float64(2 * 127 * 127)))
    w = np.array([[1.0 + 2.0 ** -30, 0.3]], np.float64)
    assert np.array_equal(I8.quantize(w)[0], I8.quantize(w.astype(np.float32))[0])


# ---- refusals of the C ABI -----------------------------------------------------------------
A = 4096   # (a dummy address: never dereferenced)


def _desc(dtype=None, d_pad=768, **kw):
    d = _lib.IndexDesc()
    d.dtype = _lib.LMI_I8 if dtype is None else dtype
    d.d, d.d_pad, d.n_rows, d.n_buckets = d_pad, d_pad, 10**6, 122
    d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _msg(lib):
    m = lib.lmi_last_error()
    return m.decode() if isinstance(m, bytes) else str(m)


def _topk(lib, d, k=10, qmode=None):
    qmode = _lib.LMI_Q_I8 if qmode is None else qmode
    return lib.lmi_bucket_topk(C.byref(d), A, 8, d.d, A, 2, k, qmode, A, A, A, A, 1 << 40, None)


def _masked(lib, d, k=10, qmode=None, tagged=False):
    qmode = _lib.LMI_Q_I8 if qmode is None else qmode
    if tagged:
        return lib.lmi_bucket_topk_tagged(C.byref(d), A, A, A, 8, d.d, A, 2, k, qmode, A, A, A, A, 1 << 40, None)
    return lib.lmi_bucket_topk_masked(C.byref(d), A, A, A, None, None, A, 8, d.d, A, 2, k, qmode, A, A, A, A,
                                      1 << 40, None)


def test_constants_and_symbol():
    lib = _lib.load()
    assert _lib.LMI_I8 == 2 and _lib.LMI_Q_I8 == 2 and "lmi_quantize_rows_i8" in _lib.EXPORTS
    getattr(lib, "lmi_quantize_rows_i8")
    assert lib.lmi_abi_version() == 13


@pytest.mark.parametrize("what,desc_kw,call_kw", [
    ("i8 rows, fp16 queries", {}, dict(qmode=_lib.LMI_Q_F16)),
    ("i8 rows, fp32 queries", {}, dict(qmode=_lib.LMI_Q_F32)),
    ("fp16 rows, i8 queries", dict(dtype=_lib.LMI_F16), {}),
    ("fp32 rows, i8 queries", dict(dtype=_lib.LMI_F32), {}),
    ("k = 17", {}, dict(k=17)),
    ("k = 1024", {}, dict(k=1024)),
    ("seed", {}, dict(qmode=_lib.LMI_Q_I8 | _lib.LMI_Q_SEED_ROUND0)),
    ("join phase", {}, dict(qmode=_lib.LMI_Q_I8 | _lib.LMI_Q_PHASE_SCAN_JOIN)),
    ("corpus32", dict(corpus32=A), {}),
    ("corpus64", dict(corpus64=A), {}),
    ("chunk_centroid", dict(chunk_centroid=A), {}),
    ("d_pad = 1024", dict(d_pad=1024), {}),
])
def test_bucket_topk_refusals_without_a_device(what, desc_kw, call_kw):
    lib = _lib.load()
    d = _desc(**desc_kw)
    for fn, call in (("lmi_bucket_topk", _topk), ("lmi_bucket_topk_masked", _masked)):
        if fn == "lmi_bucket_topk_masked" and ("seed" in what or "join" in what or call_kw.get("k", 0) > 16):
            continue   # (the masked call refuses every flag and k > 16 on any storage: its own tests)
        assert call(lib, d, **call_kw) == _lib.LMI_E_INVALID, (fn, what)
        assert "LMI_I8" in _msg(lib), (fn, what, _msg(lib))
        assert lib.lmi_scan_workspace_bytes(C.byref(d), 8, 2, call_kw.get("k", 10),
                                            call_kw.get("qmode", _lib.LMI_Q_I8)) == 0, what
        assert lib.lmi_scan_tagged_workspace_bytes(C.byref(d), 8, 2, call_kw.get("k", 10),
                                                   call_kw.get("qmode", _lib.LMI_Q_I8)) == 0, what
    assert _masked(lib, d, tagged=True, **call_kw) == _lib.LMI_E_INVALID


def test_masked_call_keeps_its_own_refusals_on_i8():
    lib = _lib.load()
    d = _desc()
    for kw in (dict(k=17), dict(qmode=_lib.LMI_Q_I8 | _lib.LMI_Q_SEED_ROUND0),
               dict(qmode=_lib.LMI_Q_I8 | _lib.LMI_Q_PHASE_PLAN), dict(qmode=_lib.LMI_Q_I8 | _lib.LMI_Q_PHASE_SCAN_JOIN)):
        assert _masked(lib, d, **kw) == _lib.LMI_E_INVALID, kw
        assert "lmi_bucket_topk_masked" in _msg(lib)


def test_the_phases_pass_the_gate():
    """PLAN / SCAN / MERGE are taken: such a call gets past every refusal of the
    storage and fails only on its (too small) workspace, still before any launch."""
    lib = _lib.load()
    d = _desc(bucket_off=A, chunk_first=A, corpus=A, inv_norm=A, gpos=A)
    for ph in (0, _lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_MERGE):
        rc = lib.lmi_bucket_topk(C.byref(d), A, 8, d.d, A, 2, 10, _lib.LMI_Q_I8 | ph, A, A, A, A, 16, None)
        assert rc == _lib.LMI_E_WORKSPACE, (ph, _msg(lib))


def test_every_other_entry_point_refuses_i8_without_a_device():
    lib = _lib.load()
    d = _desc()
    p = C.byref(d)
    eps = _lib.LMI_REFINE_EPS
    cnt = C.c_int32(0)
    calls = {
        "lmi_bucket_topk_f64": lambda: lib.lmi_bucket_topk_f64(p, A, 8, d.d, A, 2, 10, 0, eps, A, A, A, A, 1 << 40, None),
        "lmi_bucket_topk_f64q": lambda: lib.lmi_bucket_topk_f64q(p, A, 8, d.d, A, d.d, A, 2, 10, 0, eps, A, A, A, A,
                                                                 1 << 40, None),
        "lmi_bucket_topk_f64g": lambda: lib.lmi_bucket_topk_f64g(p, A, 8, d.d, A, d.d, A, 2, 10, 0, eps, A, A, 1,
                                                                 8 * 2 * 10, A, A, A, A, 1 << 40, None),
        "lmi_bucket_range": lambda: lib.lmi_bucket_range(p, None, None, A, 8, d.d, A, 2, 0, A, 64, A, A, A, A, 1 << 40,
                                                         None),
        "lmi_bucket_range_masked": lambda: lib.lmi_bucket_range_masked(p, A, A, A, None, None, A, 8, d.d, A, 2, 0, A,
                                                                       64, A, A, A, A, 1 << 40, None),
        "lmi_range_rescore_f64": lambda: lib.lmi_range_rescore_f64(p, A, 8, d.d, 2, A, 64, A, A, A, A, None),
        "lmi_range_pack": lambda: lib.lmi_range_pack(p, 8, 2, 64, A, A, A, None, None, A, A, A, None),
        "lmi_refine_fallback_count": lambda: lib.lmi_refine_fallback_count(A, p, 8, 2, 10, 0, C.byref(cnt), None),
        "lmi_split_sample_fallback_count": lambda: lib.lmi_split_sample_fallback_count(A, p, 8, 2, 10, C.byref(cnt),
                                                                                       None),
    }
    for name, call in calls.items():
        assert call() == _lib.LMI_E_INVALID, name
        assert "LMI_I8" in _msg(lib), (name, _msg(lib))
    # the size functions answer 0, and the yes / no predicates "no" (a
    # non-zero answer means yes to their callers) with the same message
    assert lib.lmi_scan_f64_workspace_bytes(p, 8, 2, 10, 0) == 0
    assert lib.lmi_range_workspace_bytes(p, 8, 2, 0, 0, 64) == 0
    for name in ("lmi_scan_joinable", "lmi_scan_f64_joinable", "lmi_f64_global_band"):
        lib.lmi_merge_topk(None, None, 0, 10, 10, None, None, None)    # (another message in between)
        assert getattr(lib, name)(p, 8, 2, 10, 0) == 0, name
        assert "LMI_I8" in _msg(lib) and name in _msg(lib), (name, _msg(lib))


def test_quantize_rows_refusals_without_a_device():
    lib = _lib.load()
    ok = dict(rows=A, dtype=_lib.LMI_F32, m=4, ld=768, d=768, d_pad=768, dst=None, codes=A, inv=A)
    for what, kw in (("dtype", dict(dtype=_lib.LMI_I8)), ("m", dict(m=-1)), ("d", dict(d=0)),
                     ("d_pad", dict(d=700, d_pad=768)), ("d_pad", dict(d_pad=800)), ("ld", dict(ld=767)),
                     ("null", dict(rows=None)), ("null", dict(codes=None)), ("null", dict(inv=None)),
                     ("aligned", dict(codes=A + 2))):
        a = dict(ok, **kw)
        rc = lib.lmi_quantize_rows_i8(a["rows"], a["dtype"], a["m"], a["ld"], a["d"], a["d_pad"], a["dst"],
                                      a["codes"], a["inv"], None)
        assert rc == _lib.LMI_E_INVALID and "quantize rows" in _msg(lib), (what, kw, _msg(lib))
    assert lib.lmi_quantize_rows_i8(None, _lib.LMI_F16, 0, 768, 768, 768, None, None, None, None) == _lib.LMI_OK


# ---- workspace sizes -------------------------------------------------------------------------
@pytest.mark.parametrize("d_pad", [32, 96, 224, 768, 992])
def test_workspace_is_positive_and_monotone(d_pad):
    lib = _lib.load()
    d = _desc(d_pad=d_pad)
    for k in (1, 10, 16):
        for fn in (lib.lmi_scan_workspace_bytes, lib.lmi_scan_tagged_workspace_bytes):
            sizes = [fn(C.byref(d), nq, 4, k, _lib.LMI_Q_I8) for nq in (1, 100, 1000, 10000)]
            assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (k, sizes)
        # the phases size the same call; one byte a component in the query buffer
        assert lib.lmi_scan_workspace_bytes(C.byref(d), 1000, 4, k, _lib.LMI_Q_I8 | _lib.LMI_Q_PHASE_SCAN) == \
            lib.lmi_scan_workspace_bytes(C.byref(d), 1000, 4, k, _lib.LMI_Q_I8)
    f32 = _desc(dtype=_lib.LMI_F32, d_pad=d_pad)
    assert lib.lmi_scan_workspace_bytes(C.byref(d), 10000, 4, 10, _lib.LMI_Q_I8) < \
        lib.lmi_scan_workspace_bytes(C.byref(f32), 10000, 4, 10, _lib.LMI_Q_F32)
