"""CPU tests of the index re-bucket's ABI (K8: csrc/lmi_rebucket.hip): the
argument checks of lmi_bucket_sort_labels / lmi_index_gather_rows fail before
any device call, the additions leave the ABI version alone, and the exported
bucket cap is at least 1024."""
import numpy as np

from li import _lib


def test_rebucket_additions_keep_the_abi_version():
    lib = _lib.load()
    assert lib.lmi_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert {"lmi_bucket_sort_labels_ws_bytes", "lmi_bucket_sort_labels",
            "lmi_index_gather_rows"} <= set(_lib.EXPORTS)
    assert _lib.LMI_STATUS_BAD_LABEL == 8
    assert _lib.LMI_REBUCKET_MAX_BUCKETS >= 1024
    assert _lib.LMI_REBUCKET_MAX_WAVES % 4 == 0 and _lib.LMI_REBUCKET_MAX_WAVES >= 4
    assert _lib.LMI_GATHER_MAX_GRID >= 1 and _lib.LMI_GATHER_TILE_ROWS >= 1


def test_sort_workspace_sizing():
    lib = _lib.load()
    ws = lib.lmi_bucket_sort_labels_ws_bytes
    cap, waves = _lib.LMI_REBUCKET_MAX_BUCKETS, _lib.LMI_REBUCKET_MAX_WAVES
    # nothing to sort, or arguments the sort refuses: no workspace
    for n, c in ((0, 4), (-1, 4), (10, 0), (10, -3), (10, cap + 1)):
        assert ws(n, c) == 0, (n, c)
    # counts[c][waves] + total[c], int64; the waves are whole workgroups of 4
    # waves, one per group of 64 labels up to the cap
    assert ws(1, 1) == (1 * 4 + 1) * 8
    assert ws(64 * 5, 7) == (7 * 8 + 7) * 8
    assert ws(64 * waves, 122) == (122 * waves + 122) * 8
    assert ws(10_000_000, 122) == (122 * waves + 122) * 8        # capped: longer intervals
    assert ws(10_000_000, cap) == (cap * waves + cap) * 8


def test_rebucket_entry_points_check_arguments_without_a_device():
    """Bad arguments are LMI_E_INVALID / LMI_E_UNSUPPORTED / LMI_E_WORKSPACE
    before any device call (the pointers here are host memory that is never
    read)."""
    lib = _lib.load()
    buf = np.zeros(4096, np.int64)
    other = np.zeros(4096, np.int64)
    p, o = buf.ctypes.data, other.ctypes.data
    need = lib.lmi_bucket_sort_labels_ws_bytes(100, 4)
    assert 0 < need <= buf.nbytes

    def sort(**kw):
        a = dict(labels=p, label_bytes=8, n=100, C=4, off=o, order=o, status=o, ws=p, ws_bytes=need)
        a.update(kw)
        return lib.lmi_bucket_sort_labels(a["labels"], a["label_bytes"], a["n"], a["C"], a["off"],
                                          a["order"], a["status"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(labels=None), dict(order=None), dict(off=None), dict(status=None),
                dict(n=-1), dict(C=0), dict(C=-2), dict(label_bytes=2), dict(label_bytes=0),
                dict(n=0, off=None), dict(n=0, status=None)):
        assert sort(**bad) == _lib.LMI_E_INVALID, bad
        assert lib.lmi_last_error()
    assert sort(C=_lib.LMI_REBUCKET_MAX_BUCKETS + 1) == _lib.LMI_E_UNSUPPORTED
    for bad in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None), dict(ws=p + 4)):
        assert sort(**bad) == _lib.LMI_E_WORKSPACE, bad
        assert lib.lmi_last_error()

    def gather(**kw):
        a = dict(src=p, src_inv=p, n_src=4, d_pad=32, src_pos=p, dst=o, dst_inv=o, n_dst=4, status=p)
        a.update(kw)
        return lib.lmi_index_gather_rows(a["src"], a["src_inv"], a["n_src"], a["d_pad"], a["src_pos"],
                                         a["dst"], a["dst_inv"], a["n_dst"], a["status"], None)

    for bad in (dict(d_pad=24), dict(d_pad=0), dict(d_pad=-32), dict(n_src=-1), dict(n_dst=-1),
                dict(src=None), dict(src_inv=None), dict(src_pos=None), dict(dst=None),
                dict(dst_inv=None), dict(status=None),
                dict(dst=p), dict(dst_inv=p),              # source == destination
                dict(src=p + 2), dict(dst=o + 8)):         # corpus not 16-byte aligned
        assert gather(**bad) == _lib.LMI_E_INVALID, bad
        assert lib.lmi_last_error()
    # nothing to write: valid, and no device call
    assert gather(n_dst=0, src=None, dst=None, src_pos=None) == _lib.LMI_OK
    assert gather(n_dst=0, n_src=0) == _lib.LMI_OK
