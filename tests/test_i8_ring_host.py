"""lmi_scan_family (CPU, no device): which kernel family the scan's plan chooses,
read from the same scan_plan the launch uses.  The 8-bit storage goes to its
8-wave ring ("ring8-i8", 3) at d_pad == 768 with 10-entry lists, plain and
tagged, and nowhere else; LMI_SCAN_V1 forces the general i8 kernel, LMI_SCAN_V2
does nothing to it; the fp16 / fp32 rows of the table are the families the
plan has always chosen."""
import ctypes as C
import os

import pytest

from li import _lib

I8_RING = [(k, t) for k in (1, 10) for t in (0, 1)]


def _desc(dtype, d_pad):
    d = _lib.IndexDesc()
    d.dtype, d.d, d.d_pad, d.n_rows, d.n_buckets = dtype, d_pad, d_pad, 10**6, 122
    d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
    return d


def _family(lib, dtype, d_pad, k, qmode, tagged=0):
    return lib.lmi_scan_family(C.byref(_desc(dtype, d_pad)), k, qmode, tagged)


class _knob:
    """One LMI_* switch set and loaded, the environment restored on the way out."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.saved = {n: os.environ.pop(n, None) for n in ("LMI_SCAN_V1", "LMI_SCAN_V2")}
        if self.name:
            os.environ[self.name] = "1"
        _lib.load().lmi_config_reload()

    def __exit__(self, *exc):
        os.environ.pop(self.name or "LMI_SCAN_V1", None)
        for n, v in self.saved.items():
            if v is not None:
                os.environ[n] = v
        _lib.load().lmi_config_reload()


def _i8_answers(lib):
    out = {}
    for d_pad in (768, 96, 736, 800, 992):
        for k in (1, 10, 11, 16):
            for t in (0, 1):
                out[d_pad, k, t] = _family(lib, _lib.LMI_I8, d_pad, k, _lib.LMI_Q_I8, t)
    return out


def test_i8_goes_to_its_ring_at_768_with_10_entry_lists_alone():
    lib = _lib.load()
    with _knob(None):
        for k, t in I8_RING:
            assert _family(lib, _lib.LMI_I8, 768, k, _lib.LMI_Q_I8, t) == 3, (k, t)
        for k in (11, 16):
            for t in (0, 1):
                assert _family(lib, _lib.LMI_I8, 768, k, _lib.LMI_Q_I8, t) == 0, (k, t)
        for d_pad in (96, 736, 800, 992):
            for k in (1, 10, 16):
                for t in (0, 1):
                    assert _family(lib, _lib.LMI_I8, d_pad, k, _lib.LMI_Q_I8, t) == 0, (d_pad, k, t)


def test_scan_v1_forces_the_general_i8_kernel_and_scan_v2_does_nothing():
    lib = _lib.load()
    with _knob(None):
        plain = _i8_answers(lib)
    assert 3 in plain.values()
    with _knob("LMI_SCAN_V1"):
        assert set(_i8_answers(lib).values()) == {0}
    with _knob("LMI_SCAN_V2"):
        assert _i8_answers(lib) == plain
    with _knob(None):
        assert _i8_answers(lib) == plain


def test_fp16_and_fp32_families_are_the_plans():
    lib = _lib.load()
    F16, F32, QF16, QF32 = _lib.LMI_F16, _lib.LMI_F32, _lib.LMI_Q_F16, _lib.LMI_Q_F32
    with _knob(None):
        assert _family(lib, F16, 768, 10, QF16) == 2
        assert _family(lib, F16, 768, 12, QF16) == 2
        assert _family(lib, F16, 768, 16, QF16) == 1
        assert _family(lib, F16, 768, 16, QF16, 1) == 0
        assert _family(lib, F16, 768, 10, QF16, 1) == 2
        assert _family(lib, F16, 96, 10, QF16) == 0
        assert _family(lib, F16, 768, 10, QF32) == 0
        assert _family(lib, F32, 768, 10, QF32) == 0
        assert _family(lib, F32, 768, 10, QF16) == 0
    with _knob("LMI_SCAN_V1"):
        assert _family(lib, F16, 768, 10, QF16) == 0
    with _knob("LMI_SCAN_V2"):
        assert _family(lib, F16, 768, 10, QF16) == 1


@pytest.mark.parametrize("dtype,qmode", [
    (_lib.LMI_I8, _lib.LMI_Q_F16), (_lib.LMI_I8, _lib.LMI_Q_F32), (_lib.LMI_F16, _lib.LMI_Q_I8),
    (_lib.LMI_I8, _lib.LMI_Q_I8 | _lib.LMI_Q_SEED_ROUND0)])
def test_refused_combinations_are_negative_and_name_the_storage(dtype, qmode):
    lib = _lib.load()
    rc = _family(lib, dtype, 768, 10, qmode)
    assert rc == -_lib.LMI_E_INVALID
    assert "LMI_I8" in lib.lmi_last_error().decode()
    assert _family(lib, _lib.LMI_I8, 768, 17, _lib.LMI_Q_I8) < 0
    assert lib.lmi_scan_family(None, 10, _lib.LMI_Q_I8, 0) < 0


def test_workspace_of_the_ring_and_of_the_general_plan_under_the_switch():
    lib = _lib.load()
    ring, general = {}, {}
    batches = ((1, 1), (1000, 4), (10000, 7))

    def sizes(d_pad, k):
        return [lib.lmi_scan_workspace_bytes(C.byref(_desc(_lib.LMI_I8, d_pad)), nq, R, k, _lib.LMI_Q_I8)
                for nq, R in batches] + \
               [lib.lmi_scan_tagged_workspace_bytes(C.byref(_desc(_lib.LMI_I8, d_pad)), nq, R, k, _lib.LMI_Q_I8)
                for nq, R in batches]

    with _knob(None):
        for k in (1, 10):
            ring[k] = sizes(768, k)
            assert min(ring[k]) > 0
        wide = {k: sizes(768, k) for k in (11, 16)}          # the general i8 plan, switch or no switch
        near = {k: sizes(736, k) for k in (1, 10)}           # the general plan one width down
    with _knob("LMI_SCAN_V1"):
        for k in (1, 10):
            general[k] = sizes(768, k)
            assert min(general[k]) > 0
        assert {k: sizes(768, k) for k in (11, 16)} == wide
        # The general i8 plan's size: 64-pair tiles and 10-entry lists at this
        # width.  It is the plan every other width has, whose size differs from
        # this one in the query codes alone: nq * d_pad bytes, rounded to 256.
        for k in (1, 10):
            for (nq, R), a, b in zip(batches * 2, general[k], near[k]):
                up = lambda n: (n + 255) // 256 * 256
                assert a - b == up(nq * 768) - up(nq * 736), (k, nq, R)
    # the ring's tiles are 256 pairs wide: fewer tiles, a smaller tile array
    for k in (1, 10):
        assert all(r <= g for r, g in zip(ring[k], general[k])) and ring[k] != general[k]
