"""CPU tests of the in-place re-bucket's ABI (K10: csrc/lmi_rebucket.hip): the
argument checks of lmi_perm_involutions / lmi_index_swap_rows fail before any
device call, the plan's workspace is sized as the header says, and the
additions leave the ABI version alone."""
import inspect

import numpy as np

from li import _lib


def test_inplace_rebucket_additions_keep_the_abi_version():
    lib = _lib.load()
    assert lib.lmi_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert {"lmi_perm_involutions_ws_bytes", "lmi_perm_involutions",
            "lmi_index_swap_rows"} <= set(_lib.EXPORTS)
    assert _lib.LMI_STATUS_BAD_PERM == 32
    bits = [_lib.LMI_STATUS_QUERY_NOT_F16, _lib.LMI_STATUS_INTERNAL, _lib.LMI_STATUS_ROWS_NOT_F16,
            _lib.LMI_STATUS_BAD_LABEL, _lib.LMI_STATUS_ROWS_LOW_NORM, _lib.LMI_STATUS_BAD_PERM]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)


def test_relabel_and_rebucket_take_inplace_off_by_default():
    from li.index import DeviceIndex
    from li.LearnedIndex import LearnedIndex
    for fn in (DeviceIndex.relabel, LearnedIndex.rebucket):
        p = inspect.signature(fn).parameters["inplace"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_plan_workspace_sizing():
    ws = _lib.load().lmi_perm_involutions_ws_bytes
    for n in (0, -1, -2 ** 40):
        assert ws(n) == 0, n
    # two ping-pong arrays of n (value, next) pairs, the leaders, one sum per
    # 2048 rows of the prefix scan -- int64, rounded up to 16 bytes
    up = lambda b: (b + 15) // 16 * 16
    for n in (1, 2, 2047, 2048, 2049, 65537, 10_000_000, 100_000_000):
        assert ws(n) == up((5 * n + (n + 2047) // 2048) * 8), n
    assert ws(100_000_000) < 41 * 100_000_000                     # ~40 B a row against 1536 B of corpus


def test_inplace_rebucket_entry_points_check_arguments_without_a_device():
    """Bad arguments are LMI_E_INVALID / LMI_E_WORKSPACE before any device call
    (the pointers here are host memory that is never read)."""
    lib = _lib.load()
    bufs = [np.zeros(4096, np.int64) for _ in range(5)]
    assert all(b.ctypes.data % 16 == 0 for b in bufs)
    s, a, b, st, w = (x.ctypes.data for x in bufs)
    n = 100
    need = lib.lmi_perm_involutions_ws_bytes(n)
    assert 0 < need <= bufs[4].nbytes

    def plan(**kw):
        g = dict(src=s, n=n, p1=a, p2=b, status=st, ws=w, ws_bytes=need)
        g.update(kw)
        return lib.lmi_perm_involutions(g["src"], g["n"], g["p1"], g["p2"], g["status"], g["ws"],
                                        g["ws_bytes"], None)

    for bad in (dict(src=None), dict(p1=None), dict(p2=None), dict(status=None), dict(n=-1),
                dict(n=0, status=None),
                dict(src=s + 4), dict(p1=a + 4), dict(p2=b + 2), dict(status=st + 2),   # misaligned
                dict(p2=a), dict(p1=s), dict(p2=s)):                                    # one buffer twice
        assert plan(**bad) == _lib.LMI_E_INVALID, bad
        assert lib.lmi_last_error()
    for bad in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None), dict(ws=w + 8)):
        assert plan(**bad) == _lib.LMI_E_WORKSPACE, bad
        assert lib.lmi_last_error()
    # nothing to plan: valid, and no device call
    assert plan(n=0, src=None, p1=None, p2=None, ws=None, ws_bytes=0) == _lib.LMI_OK

    def swap(**kw):
        g = dict(corpus=a, inv=b, n=4, d_pad=32, partner=s, status=st)
        g.update(kw)
        return lib.lmi_index_swap_rows(g["corpus"], g["inv"], g["n"], g["d_pad"], g["partner"],
                                       g["status"], None)

    for bad in (dict(corpus=None), dict(inv=None), dict(partner=None), dict(status=None), dict(n=-1),
                dict(d_pad=0), dict(d_pad=-8), dict(d_pad=12), dict(d_pad=100), dict(d_pad=7),
                dict(corpus=a + 8), dict(corpus=a + 2),          # corpus not 16-byte aligned
                dict(inv=b + 2), dict(partner=s + 4), dict(status=st + 1)):
        assert swap(**bad) == _lib.LMI_E_INVALID, bad
        assert lib.lmi_last_error()
    assert swap(n=0, corpus=None, inv=None, partner=None) == _lib.LMI_OK
