"""The scan workspace sizes are ABI-visible (a caller sizes its workspace once):
lmi_scan_workspace_bytes and lmi_scan_f64_workspace_bytes over a fixed grid of
index shapes, query classes, k, batch sizes and knobs, against the sizes the
library gave before the scan's host code was reorganised around one plan
(tests/golden/scan_ws_bytes.json, written by `python tests/test_scan_workspace_table.py
OUT.json` with the package of that earlier commit first on PYTHONPATH).

The table also records which knobs move a size: LMI_SCAN_SPLIT and
LMI_SCAN_NO_PREF and the index's chunk centroids never do (a workspace sized
once fits every call); LMI_SCAN_SPLIT_PARTS does, on the 8-wave ring (the
buffers are sized for the parts), as do the kernel-family switches."""
import ctypes as C
import json
import os
import sys

KNOBS = ("", "LMI_SCAN_SPLIT=-1", "LMI_SCAN_SPLIT_PARTS=4", "LMI_SCAN_NO_PREF=1", "LMI_WIDE_PASSES=1",
         "LMI_SCAN_V1=1", "LMI_SCAN_V2=1")
KS = (1, 10, 11, 15, 16, 17, 30, 100)
BATCHES = ((1, 1), (1000, 4), (10000, 7))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_ws_bytes.json")


def cases():
    """(dtype, d_pad, qmode, k, nq, R, centroid, corpus32) in table order."""
    from li import _lib
    for dtype in (_lib.LMI_F16, _lib.LMI_F32):
        for d_pad in (96, 768):
            for qmode in (_lib.LMI_Q_F16, _lib.LMI_Q_F32):
                for k in KS:
                    for nq, R in BATCHES:
                        for centroid in (False, True):
                            for corpus32 in (False, True) if k <= _lib.LMI_MAX_K else (False,):
                                yield dtype, d_pad, qmode, k, nq, R, centroid, corpus32


def sizes(lib):
    """[[scan bytes, f64 bytes], ...] over cases() under the knobs now loaded."""
    from li import _lib
    out = []
    for dtype, d_pad, qmode, k, nq, R, centroid, corpus32 in cases():
        d = _lib.IndexDesc()
        d.dtype, d.d, d.d_pad, d.n_rows, d.n_buckets = dtype, d_pad, d_pad, 10**6, 122
        d.chunk_rows, d.n_chunks, d.max_chunks = 8192, 200, 5
        # (dummy addresses: sizing never dereferences them)
        d.chunk_centroid = 4096 if centroid else None
        d.corpus32 = 4096 if corpus32 else None
        out.append([lib.lmi_scan_workspace_bytes(C.byref(d), nq, R, k, qmode),
                    lib.lmi_scan_f64_workspace_bytes(C.byref(d), nq, R, k, qmode)])
    return out


def table(lib):
    """{knob setting: sizes()}; the environment is left as it was found."""
    names = [kn.split("=")[0] for kn in KNOBS if kn]
    saved = {n: os.environ.get(n) for n in names}
    out = {}
    try:
        for kn in KNOBS:
            for n in names:
                os.environ.pop(n, None)
            if kn:
                os.environ[kn.split("=")[0]] = kn.split("=")[1]
            lib.lmi_config_reload()
            out[kn or "none"] = sizes(lib)
    finally:
        for n, v in saved.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
        lib.lmi_config_reload()
    return out


def test_scan_workspace_sizes_match_the_recorded_table():
    from li import _lib
    got = table(_lib.load())
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want)
    cs = list(cases())
    for kn in got:
        assert len(got[kn]) == len(want[kn]) == len(cs)
        bad = [(c, g, w) for c, g, w in zip(cs, got[kn], want[kn]) if g != w]
        assert not bad, f"{kn}: {len(bad)} sizes differ, first {bad[0]}"
    # a workspace sized once fits every call: these knobs and the chunk
    # centroids (cases differing only in `centroid` are neighbours or two apart)
    for kn in ("LMI_SCAN_SPLIT=-1", "LMI_SCAN_NO_PREF=1"):
        assert got[kn] == got["none"], kn
    by_case = dict(zip(cs, got["none"]))
    for c, v in by_case.items():
        assert v == by_case[c[:6] + (not c[6],) + c[7:]], c
    # (recorded, not required: the parts knob and the family switches move sizes)
    assert got["LMI_SCAN_SPLIT_PARTS=4"] != got["none"]
    assert all(min(v) > 0 for v in got["none"])


if __name__ == "__main__":
    from li import _lib
    with open(sys.argv[1], "w") as f:
        json.dump(table(_lib.load()), f, separators=(",", ":"))
        f.write("\n")
