"""Re-ranking 8-bit lists from kept fp16 rows, the parts that need no device:
the plan sends k = 11..16 of the 8-bit storage at d_pad == 768 to its ring (16-
entry lists) on a thread that asked (lmi_scan_set_i8_lists16) and nowhere else,
and LMI_SCAN_V1 still forces the general kernel; lmi_rerank_f64 is
exported and refuses every malformed call with LMI_E_INVALID and a message that
names it, before any launch; li.index.check_rerank, DeviceIndex(keep_rows=...)
and LearnedIndex.attach(rerank=...) raise their ValueErrors before anything is
built."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from li import _lib
from li.index import DeviceIndex, RowSource, check_rerank

A = 4096   # a non-null pointer nobody follows: every call below is refused first


def _desc(dtype=_lib.LMI_F16, d=768, d_pad=768, n_rows=1000, **kw):
    x = _lib.IndexDesc()
    x.dtype, x.d, x.d_pad, x.n_rows, x.n_buckets = dtype, d, d_pad, n_rows, 3
    x.corpus = A
    for name, v in kw.items():
        setattr(x, name, v)
    return x


def _rerank(lib, desc, q=A, nq=8, ldq=None, R=2, pos=A, k_in=16, k=10, out_d=A, out_pos=A, status=A):
    return lib.lmi_rerank_f64(None if desc is None else C.byref(desc), q, nq, desc.d if ldq is None else ldq, R,
                              pos, k_in, k, out_d, out_pos, status, None)


def test_symbol_and_abi_version():
    lib = _lib.load()
    assert "lmi_rerank_f64" in _lib.EXPORTS and hasattr(lib, "lmi_rerank_f64")
    assert lib.lmi_abi_version() == _lib.ABI_VERSION == 13          # an addition: the version stays


@pytest.mark.parametrize("what,desc,kw", [
    ("int8 rows", _desc(dtype=_lib.LMI_I8), {}),
    ("float32 rows", _desc(dtype=_lib.LMI_F32), {}),
    ("corpus32", _desc(corpus32=A), {}),
    ("corpus64", _desc(corpus64=A), {}),
    ("chunk_centroid", _desc(chunk_centroid=A), {}),
    ("d > 1024", _desc(d=1056, d_pad=1056), {}),
    ("d < 1", _desc(d=0), {}),
    ("d_pad < d", _desc(d=768, d_pad=736), {}),
    ("null corpus", _desc(corpus=None), {}),
    ("k < 1", _desc(), dict(k=0)),
    ("k > k_in", _desc(), dict(k=11, k_in=10)),
    ("k_in > LMI_MAX_K", _desc(), dict(k=10, k_in=17)),
    ("R < 1", _desc(), dict(R=0)),
    ("nq < 0", _desc(), dict(nq=-1)),
    ("ldq < d", _desc(), dict(ldq=767)),
    ("null q", _desc(), dict(q=None)),
    ("null pos", _desc(), dict(pos=None)),
    ("null out_d", _desc(), dict(out_d=None)),
    ("null out_pos", _desc(), dict(out_pos=None)),
    ("null status", _desc(), dict(status=None)),
])
def test_rerank_refusals_without_a_device(what, desc, kw):
    lib = _lib.load()
    assert _rerank(lib, desc, **kw) == _lib.LMI_E_INVALID, what
    assert "lmi_rerank_f64" in lib.lmi_last_error().decode(), what


def test_rerank_null_descriptor_and_empty_batch():
    lib = _lib.load()
    assert lib.lmi_rerank_f64(None, A, 8, 768, 2, A, 16, 10, A, A, A, None) == _lib.LMI_E_INVALID
    assert "lmi_rerank_f64" in lib.lmi_last_error().decode()
    assert _rerank(lib, _desc(), nq=0, q=None, pos=None, out_d=None, out_pos=None, status=None) == _lib.LMI_OK


def _scan_desc(d_pad):
    x = _desc(dtype=_lib.LMI_I8, d=d_pad, d_pad=d_pad, n_rows=10**6)
    x.chunk_rows, x.n_chunks, x.max_chunks, x.n_buckets = 8192, 200, 5, 122
    return x


def _family(lib, d_pad, k, tagged):
    return lib.lmi_scan_family(C.byref(_scan_desc(d_pad)), k, _lib.LMI_Q_I8, tagged)


def test_plan_sends_16_entry_lists_to_the_i8_ring_for_a_thread_that_asks():
    import threading
    lib = _lib.load()
    saved = {n: os.environ.pop(n, None) for n in ("LMI_SCAN_V1", "LMI_SCAN_V2")}
    try:
        lib.lmi_config_reload()
        # by default every k keeps the plan it had
        for t in (0, 1):
            assert [_family(lib, 768, k, t) for k in range(1, 17)] == [3] * 10 + [0] * 6, t
        plain = [lib.lmi_scan_workspace_bytes(C.byref(_scan_desc(768)), 1000, 4, k, _lib.LMI_Q_I8) for k in (10, 16)]
        assert lib.lmi_scan_set_i8_lists16(1) == 0
        try:
            for k in range(1, 17):
                for t in (0, 1):
                    assert _family(lib, 768, k, t) == 3, (k, t)          # "ring8-i8"
                    assert _family(lib, 736, k, t) == 0, (k, t)          # other widths: scan_i8_kernel
            assert _family(lib, 768, 17, 0) < 0
            asked = [lib.lmi_scan_workspace_bytes(C.byref(_scan_desc(768)), 1000, 4, k, _lib.LMI_Q_I8)
                     for k in (10, 16)]
            # (k = 10 is untouched; k = 16 takes the ring's 256-pair tiles: a smaller tile array)
            assert asked[0] == plain[0] and 0 < asked[1] < plain[1]
            # the setting is the calling thread's own
            seen = []
            th = threading.Thread(target=lambda: seen.append((_family(lib, 768, 16, 0),
                                                              lib.lmi_scan_set_i8_lists16(0))))
            th.start()
            th.join()
            assert seen == [(0, 0)]
            os.environ["LMI_SCAN_V1"] = "1"
            lib.lmi_config_reload()
            for k in (10, 11, 16):
                for t in (0, 1):
                    assert _family(lib, 768, k, t) == 0, (k, t)
        finally:
            assert lib.lmi_scan_set_i8_lists16(0) == 1
        assert lib.lmi_scan_set_i8_lists16(7) == 0 and lib.lmi_scan_set_i8_lists16(0) == 1      # (any non-zero: on)
    finally:
        os.environ.pop("LMI_SCAN_V1", None)
        for n, v in saved.items():
            if v is not None:
                os.environ[n] = v
        lib.lmi_config_reload()


def _ix(storage="i8", rows16=object()):
    return types.SimpleNamespace(storage=storage, rows16=rows16)


@pytest.mark.parametrize("index,rerank,k_list,dist,what", [
    (_ix(rows16=None), 16, 10, "f64", "keeps no fp16 rows"),
    (_ix(storage="f16"), 16, 10, "f64", "storage 'i8'"),
    (_ix(storage="f32"), 16, 10, "f64", "storage 'i8'"),
    (_ix(), 10, 10, "f64", "must lie in"),
    (_ix(), 9, 10, "f64", "must lie in"),
    (_ix(), 17, 10, "f64", "must lie in"),
    (_ix(), 16, 16, "f64", "must lie in"),
    (_ix(), 16, 10, "f32", "float64"),
    (_ix(), 16.0, 10, "f64", "integer"),
    (_ix(), True, 10, "f64", "integer"),
])
def test_check_rerank_refuses(index, rerank, k_list, dist, what):
    with pytest.raises(ValueError, match=what):
        check_rerank(index, rerank, k_list, dist)


def test_check_rerank_accepts():
    for k2, k in ((16, 10), (11, 10), (16, 15), (2, 1), (np.int64(16), 10)):
        check_rerank(_ix(), k2, k, "f64")


def test_keep_rows_refused_before_anything_is_built():
    x = np.zeros((4, 768), np.float16)
    lab = np.zeros(4, np.int64)
    for storage in ("auto", "f16", "f32", "f32x"):
        with pytest.raises(ValueError, match="keep_rows"):
            DeviceIndex(x, lab, 1, device="cpu", storage=storage, keep_rows=True)
    with pytest.raises(ValueError, match="RowSource"):
        DeviceIndex(RowSource(4, 768, lambda a, b: None), lab, 1, device="cpu", storage="i8", keep_rows=True)


def test_attach_rerank_refused_before_anything_is_built():
    from li.LearnedIndex import LearnedIndex
    li_ = LearnedIndex()
    for kw, what in ((dict(rerank=16), "keep_rows"),
                     (dict(rerank=16, storage="i8"), "keep_rows"),
                     (dict(rerank=16, keep_rows=True), "storage='i8'"),
                     (dict(rerank=16, storage="f16", keep_rows=True), "storage='i8'"),
                     (dict(rerank=10, storage="i8", keep_rows=True), "must lie in"),
                     (dict(rerank=17, storage="i8", keep_rows=True), "must lie in"),
                     (dict(rerank=True, storage="i8", keep_rows=True), "integer")):
        with pytest.raises(ValueError, match=what):
            li_.attach(None, None, None, **kw)
