"""Range search (K11), the parts that need no device: the four C symbols,
every refusal of lmi_bucket_range, lmi_range_rescore_f64 and lmi_range_pack
(before any launch, with a message that names the symbol), and the workspace
size (positive, monotone in nq and in pair_cap on the 8-wave ring, 0 for what
the call refuses)."""
import ctypes as C

import pytest

from li import _lib

SYMBOLS = ("lmi_range_workspace_bytes", "lmi_bucket_range", "lmi_range_rescore_f64", "lmi_range_pack")


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


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.lmi_abi_version() == _lib.ABI_VERSION == 13


def _scan(lib, d, *, tags=None, want=None, nq=8, R=2, qmode=0, bound=4096, cap=256, cand=4096, ldq=None,
          ws_bytes=1 << 40):
    return lib.lmi_bucket_range(C.byref(d), tags, want, 4096, nq, d.d if ldq is None else ldq, 4096, R, qmode,
                                bound, cap, cand, 4096, 4096, 4096, ws_bytes, None)


@pytest.mark.parametrize("what,desc_kw,call_kw", [
    ("tags without want", {}, dict(tags=4096)),
    ("want without tags", {}, dict(want=4096)),
    ("corpus32", dict(corpus32=4096), {}),
    ("corpus64", dict(corpus64=4096), {}),
    ("chunk_centroid", dict(chunk_centroid=4096), {}),
    ("bad dtype", dict(dtype=7), {}),
    ("d_pad not a multiple of 32", dict(d_pad=100), {}),
    ("chunk_rows", dict(chunk_rows=100), {}),
    ("plan phase", {}, dict(qmode=_lib.LMI_Q_PHASE_PLAN)),
    ("scan phase", {}, dict(qmode=_lib.LMI_Q_F32 | _lib.LMI_Q_PHASE_SCAN)),
    ("join", {}, dict(qmode=_lib.LMI_Q_PHASE_SCAN_JOIN)),
    ("seed", {}, dict(qmode=_lib.LMI_Q_SEED_ROUND0)),
    ("pair_cap 0", {}, dict(cap=0)),
    ("pair_cap > 2^24", {}, dict(cap=(1 << 24) + 1)),
    ("nq < 0", {}, dict(nq=-1)),
    ("R < 1", {}, dict(R=0)),
    ("ldq < d", {}, dict(ldq=8)),
    ("null bound", {}, dict(bound=None)),
    ("null cand", {}, dict(cand=None)),
])
def test_scan_refusals_without_a_device(what, desc_kw, call_kw):
    lib = _lib.load()
    rc = _scan(lib, _desc(**desc_kw), **call_kw)
    assert rc == _lib.LMI_E_INVALID, what
    assert "lmi_bucket_range" in _message(lib), (what, _message(lib))


def test_scan_refuses_a_small_workspace_and_join_workgroups():
    lib = _lib.load()
    for dtype, d_pad in ((None, 768), (None, 96), (_lib.LMI_F32, 96)):
        d = _desc(dtype, d_pad, corpus=4096, inv_norm=4096, gpos=4096, bucket_off=4096, chunk_first=4096)
        rc = _scan(lib, d, ws_bytes=1024)
        assert rc == _lib.LMI_E_WORKSPACE
        assert "lmi_bucket_range" in _message(lib)
    prev = lib.lmi_scan_set_join_workgroups(8)
    try:
        assert _scan(lib, _desc()) == _lib.LMI_E_INVALID
        assert "lmi_bucket_range" in _message(lib)
    finally:
        lib.lmi_scan_set_join_workgroups(prev)
    # an empty batch is no work and no error, whatever the pointers
    assert _scan(lib, _desc(), nq=0, bound=None, cand=None) == _lib.LMI_OK


def test_null_index_is_refused_by_every_call():
    lib = _lib.load()
    assert lib.lmi_bucket_range(None, None, None, 4096, 8, 768, 4096, 2, 0, 4096, 256, 4096, 4096, 4096, 4096,
                                1 << 40, None) == _lib.LMI_E_INVALID
    assert "lmi_bucket_range" in _message(lib)
    assert lib.lmi_range_rescore_f64(None, 4096, 8, 768, 2, 4096, 256, 4096, 4096, 4096, 4096,
                                     None) == _lib.LMI_E_INVALID
    assert "lmi_range_rescore_f64" in _message(lib)
    assert lib.lmi_range_pack(None, 8, 2, 256, 4096, 4096, 4096, None, None, 4096, 4096, 4096,
                              None) == _lib.LMI_E_INVALID
    assert "lmi_range_pack" in _message(lib)
    assert lib.lmi_range_workspace_bytes(None, 8, 2, 0, 0, 256) == 0


@pytest.mark.parametrize("what,desc_kw,kw", [
    ("corpus32", dict(corpus32=4096), {}),
    ("corpus64", dict(corpus64=4096), {}),
    ("d > 1024", dict(d_pad=1056), {}),
    ("R < 1", {}, dict(R=0)),
    ("pair_cap 0", {}, dict(cap=0)),
    ("ldq < d", {}, dict(ldq=8)),
    ("null radius", {}, dict(radius=None)),
    ("null d64", {}, dict(d64=None)),
])
def test_rescore_refusals_without_a_device(what, desc_kw, kw):
    lib = _lib.load()
    d = _desc(**desc_kw)
    rc = lib.lmi_range_rescore_f64(C.byref(d), 4096, 8, kw.get("ldq", d.d), kw.get("R", 2),
                                   kw.get("radius", 4096), kw.get("cap", 256), 4096, 4096,
                                   kw.get("d64", 4096), 4096, None)
    assert rc == _lib.LMI_E_INVALID, what
    assert "lmi_range_rescore_f64" in _message(lib), (what, _message(lib))


@pytest.mark.parametrize("what,kw", [
    ("R < 1", dict(R=0)),
    ("pair_cap 0", dict(cap=0)),
    ("d64 without radius64", dict(d64=4096)),
    ("radius64 without d64", dict(radius64=4096)),
    ("null offsets", dict(off=None)),
    ("null gpos", dict(gpos=None)),
])
def test_pack_refusals_without_a_device(what, kw):
    lib = _lib.load()
    d = _desc(gpos=kw.get("gpos", 4096))
    rc = lib.lmi_range_pack(C.byref(d), 8, kw.get("R", 2), kw.get("cap", 256), 4096, 4096, kw.get("off", 4096),
                            kw.get("d64"), kw.get("radius64"), 4096, 4096, 4096, None)
    assert rc == _lib.LMI_E_INVALID, what
    assert "lmi_range_pack" in _message(lib), (what, _message(lib))


def test_workspace_is_positive_and_monotone():
    lib = _lib.load()
    for dtype, d_pad, qmode in ((None, 768, _lib.LMI_Q_F16), (None, 768, _lib.LMI_Q_F32),
                                (None, 96, _lib.LMI_Q_F16), (None, 224, _lib.LMI_Q_F16),
                                (_lib.LMI_F32, 96, _lib.LMI_Q_F32)):
        d = _desc(dtype, d_pad)
        for tagged in (0, 1):
            sizes = [lib.lmi_range_workspace_bytes(C.byref(d), nq, 4, qmode, tagged, 256)
                     for nq in (0, 1, 100, 1000, 10000)]
            assert sizes[0] > 0
            assert all(a < b for a, b in zip(sizes[1:], sizes[2:])), (d_pad, qmode, tagged, sizes)
            assert sizes[0] <= sizes[1]
            # the 8-wave ring keeps its grouped candidates in the workspace: pair_cap counts there
            small = lib.lmi_range_workspace_bytes(C.byref(d), 1000, 4, qmode, tagged, 32)
            ring = dtype is None and d_pad == 768 and qmode == _lib.LMI_Q_F16 and not tagged
            assert (small < sizes[3]) if ring else (small == sizes[3])
    # what the call refuses has no size
    d = _desc()
    assert lib.lmi_range_workspace_bytes(C.byref(_desc(corpus32=4096)), 10, 2, 0, 0, 256) == 0
    assert lib.lmi_range_workspace_bytes(C.byref(_desc(chunk_centroid=4096)), 10, 2, 0, 0, 256) == 0
    assert lib.lmi_range_workspace_bytes(C.byref(d), 10, 2, _lib.LMI_Q_PHASE_SCAN, 0, 256) == 0
    assert lib.lmi_range_workspace_bytes(C.byref(d), 10, 0, 0, 0, 256) == 0
    assert lib.lmi_range_workspace_bytes(C.byref(d), 10, 2, 0, 0, 0) == 0
    # the list scans' workspaces are what they were
    assert lib.lmi_scan_workspace_bytes(C.byref(d), 1000, 4, 10, 0) > 0


def test_a_width_past_the_query_tiles_lds_is_refused_without_a_device():
    """range_scan_kernel stages QB queries of d_pad + QPAD elements: 64 x (d_pad
    + 8) halves in fp16 math, 32 x (d_pad + 4) floats in fp32 math, plus the slot
    arrays -- 160 KB of LDS hold d_pad = 1248 in both and 1280 in neither.  The
    refusal comes before the workspace check and names the symbol; the workspace
    size of such a width is 0, which is what the Python layer asks before it
    allocates."""
    lib = _lib.load()
    ptrs = dict(corpus=4096, inv_norm=4096, gpos=4096, bucket_off=4096, chunk_first=4096)
    for dtype, qmode in ((None, _lib.LMI_Q_F16), (None, _lib.LMI_Q_F32), (_lib.LMI_F32, _lib.LMI_Q_F32)):
        for tagged in (0, 1):
            assert lib.lmi_range_workspace_bytes(C.byref(_desc(dtype, 1248)), 10, 2, qmode, tagged, 256) > 0
            assert lib.lmi_range_workspace_bytes(C.byref(_desc(dtype, 1280)), 10, 2, qmode, tagged, 256) == 0
        for ws_bytes in (1 << 40, 1024):
            rc = _scan(lib, _desc(dtype, 1280, **ptrs), qmode=qmode, ws_bytes=ws_bytes)
            assert rc == _lib.LMI_E_UNSUPPORTED, (dtype, qmode, ws_bytes)
            assert "lmi_bucket_range" in _message(lib) and "1280" in _message(lib)
        assert _scan(lib, _desc(dtype, 1248, **ptrs), qmode=qmode, ws_bytes=1024) == _lib.LMI_E_WORKSPACE
