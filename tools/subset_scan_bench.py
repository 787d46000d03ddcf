#!/usr/bin/env python3
"""The scan inside an id allow-list (Searcher.lists(subset=), scan_subset_kernel)
against the default scan and the tagged scan, one GPU, one process:

    python tools/subset_scan_bench.py         # 10M x 768 -> profiles/subset_scan_10M.json

A tagged index; bit b of a row's tag word is set with probability 1/2, 1/8 and
1/64 (b = 0, 1, 2), and the subset of a selectivity is the ids with that bit --
the tagged scan (want = the bit) and the subset scan answer the same lists.
Sides: the default scan of the whole index, want = bit b, subset = those ids
(prepared once, outside the timed launches: li.subset.prepare, whose own wall
time is recorded beside them as prepare_ms), and the subset of every id.  Per side
Searcher.lists(k_list=10) (router + scan + merge) between device events -- per
repeat the median of --launches launches, the sides taken in turn inside every
repeat; the spread is max - min of the repeat medians.  For the subset sides
also the scan kernel alone (lmi_timing) and the gathered bytes (each bucket's
subset rows once per group of 32 of its pairs) per second of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, subset, synth  # noqa: E402
from li.index import DeviceIndex, DeviceRouter, Searcher, scan_family  # noqa: E402

SCALES = {"10M": 10_000_000, "1M": 1_000_000, "300K": 300_000}
SHARES = (2, 8, 64)
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", default="10M", choices=list(SCALES))
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("subset_scan_bench needs a HIP device (no CPU path)")
    n, nq, R, k = SCALES[a.scale], a.nq, a.R, a.k
    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, a.buckets, "MLP-5", DEV, d=a.d)
    router = DeviceRouter(layers, device=DEV)
    rng = np.random.default_rng(5)
    tags = sum((rng.random(n) < 1.0 / share).astype(np.uint32) << b for b, share in enumerate(SHARES))
    ix = DeviceIndex(x, router.argmax(xn), a.buckets, device=DEV, tags=tags)
    del xn
    s = Searcher(ix, router)
    lib = _lib.load()
    # the preparation a caller who passes raw ids pays on every call (ids -> positions on the host, the upload,
    # the device sort, the ranges): wall time of three, the median; the first call of an index also sorts its
    # id table once, left out here
    import time
    subset.prepare(ix, ix.pos_to_id[:1])
    subs, prep_ms = {}, {}
    for name, ids in [(f"1/{share}", ix.ids_with(want=1 << b)) for b, share in enumerate(SHARES)] + \
            [("whole", ix.pos_to_id)]:
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            subs[name] = subset.prepare(ix, ids)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        prep_ms[name] = float(np.median(ts))
    sides = {"default": lambda: s.lists(qn, q, R, k)}
    for b, share in enumerate(SHARES):
        sides[f"tagged 1/{share}"] = lambda b=b: s.lists(qn, q, R, k, want=1 << b)
    for name, sub in subs.items():
        sides[f"subset {name}"] = lambda sub=sub: s.lists(qn, q, R, k, subset=sub)
    med, out = {m: [] for m in sides}, {}
    for rep in range(-1, a.repeats):          # (repeat -1: every side's warm-up)
        for m, fn in sides.items():
            ms = []
            for _ in range(a.warmup if rep < 0 else a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out[m] = fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            if rep >= 0:
                med[m].append(float(np.median(ms)))
    rows = {m: {"median_of_medians_ms": float(np.median(v)), "repeat_medians_ms": [round(t, 4) for t in v],
                "spread_ms": float(max(v) - min(v))} for m, v in med.items()}
    cls = out["default"][0].cpu().numpy()
    groups = (np.bincount(cls[cls >= 0], minlength=a.buckets) + 31) // 32
    for name, sub in subs.items():
        row = rows[f"subset {name}"]
        if name != "whole":
            row["positions_equal_tagged"] = bool(torch.equal(out[f"subset {name}"][2], out[f"tagged {name}"][2]))
            row["speedup_vs_tagged"] = rows[f"tagged {name}"]["median_of_medians_ms"] / row["median_of_medians_ms"]
        lib.lmi_timing_read(None, 0)
        lib.lmi_timing_enable(1)
        for _ in range(a.launches):
            sides[f"subset {name}"]()
        torch.cuda.synchronize()
        lib.lmi_timing_enable(0)
        buf = (_lib.C.c_float * a.launches)()
        got = lib.lmi_timing_read(buf, a.launches)
        kern = float(np.median(list(buf)[:got]))
        gathered = int((sub.bucket_size * groups).sum()) * (ix.d_pad * 2 + 8)  # (row, norm, position)
        row.update(subset_rows=sub.n, prepare_ms=prep_ms[name], scan_kernel_ms=kern, gathered_bytes=gathered,
                   subset_bytes=sub.n * (ix.d_pad * 2 + 8), gathered_TBps=gathered / kern / 1e9)
    for m, row in rows.items():
        print(json.dumps({"side": m, **{key: (round(v, 4) if isinstance(v, float) else v) for key, v in row.items()
                                        if key != "repeat_medians_ms"}}), flush=True)
    res = {"scale": a.scale, "n": n, "d": a.d, "nq": nq, "R": R, "k": k, "buckets": a.buckets,
           "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "family_default": scan_family(ix, k),
           "family_tagged": scan_family(ix, k, tagged=True),
           "timing": "device events around Searcher.lists (router + scan + merge); per repeat the median of the "
                     "launches, the sides in turn inside every repeat, one process; scan_kernel_ms: lmi_timing",
           "sides": rows}
    out_path = a.out or os.path.join(ROOT, "profiles", f"subset_scan_{a.scale}{'' if a.d == 768 else f'_d{a.d}'}.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
