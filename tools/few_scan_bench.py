#!/usr/bin/env python3
"""A small batch on the default scan against the few-query scan
(Searcher.lists(few=True), scan_few_kernel), one GPU, one process:

    python tools/few_scan_bench.py            # 10M x 768 -> profiles/few_scan_10M.json
    python tools/few_scan_bench.py --d 96     # against the general kernel -> profiles/few_scan_10M_d96.json

Per nq in --nqs: Searcher.lists(k_list=10) (router + scan + merge) between
device events on the default path and, while nq * R <= 256, with few=True --
per repeat the median of --launches launches, the two sides taken in turn inside
every repeat; the spread is max - min of the repeat medians.  For the few side
also the scan kernel alone (lmi_timing) and the bytes of the probed buckets'
rows (once per group of 32 pairs) per second of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import FEW_MAX_PAIRS, DeviceIndex, DeviceRouter, Searcher, scan_family  # noqa: E402

SCALES = {"10M": 10_000_000, "1M": 1_000_000, "300K": 300_000}
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", default="10M", choices=list(SCALES))
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nqs", default="1,4,16,64,256")
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("few_scan_bench needs a HIP device (no CPU path)")
    n, R, k = SCALES[a.scale], a.R, a.k
    nqs = [int(v) for v in a.nqs.split(",")]
    x, q, qn, xn, layers = synth.build_lmi_workload(n, max(nqs), a.buckets, "MLP-5", DEV, d=a.d)
    router = DeviceRouter(layers, device=DEV)
    ix = DeviceIndex(x, router.argmax(xn), a.buckets, device=DEV)
    del xn
    s = Searcher(ix, router)
    lib = _lib.load()
    sizes = np.asarray(ix.bucket_size, dtype=np.int64)
    rows = {}
    for nq in nqs:
        sides = {"default": lambda nq=nq: s.lists(qn[:nq], q[:nq], R, k)}
        if nq * R <= FEW_MAX_PAIRS:
            sides["few"] = lambda nq=nq: s.lists(qn[:nq], q[:nq], R, k, few=True)
        med = {m: [] for m in sides}
        for rep in range(-1, a.repeats):          # (repeat -1: every side's warm-up)
            for m, fn in sides.items():
                ms = []
                for _ in range(a.warmup if rep < 0 else a.launches):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    out = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                if rep >= 0:
                    med[m].append(float(np.median(ms)))
        row = {m: {"median_of_medians_ms": float(np.median(v)), "repeat_medians_ms": [round(t, 4) for t in v],
                   "spread_ms": float(max(v) - min(v))} for m, v in med.items()}
        if "few" in sides:
            same = s.lists(qn[:nq], q[:nq], R, k)
            row["positions_equal_default"] = bool(torch.equal(out[2], same[2]))
            lib.lmi_timing_read(None, 0)
            lib.lmi_timing_enable(1)
            for _ in range(a.launches):
                sides["few"]()
            torch.cuda.synchronize()
            lib.lmi_timing_enable(0)
            buf = (_lib.C.c_float * a.launches)()
            got = lib.lmi_timing_read(buf, a.launches)
            kern = float(np.median(list(buf)[:got]))
            cls = out[0].cpu().numpy()
            # (a bucket's rows are read once per group of <= 32 of its pairs)
            cnt = np.bincount(cls[cls >= 0], minlength=len(sizes))
            probed = int((sizes * ((cnt + 31) // 32)).sum()) * (ix.d_pad * 2 + 4)
            row["few"].update(scan_kernel_ms=kern, probed_bytes=probed, probed_TBps=probed / kern / 1e9,
                              speedup=row["default"]["median_of_medians_ms"] / row["few"]["median_of_medians_ms"])
        rows[str(nq)] = row
        print(json.dumps({"nq": nq, **{m: round(row[m]["median_of_medians_ms"], 4) for m in sides},
                          **({key: round(row["few"][key], 4) for key in ("scan_kernel_ms", "probed_TBps", "speedup")}
                             if "few" in row else {})}), flush=True)
    res = {"scale": a.scale, "n": n, "d": a.d, "R": R, "k": k, "buckets": a.buckets, "launches": a.launches,
           "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "family_default": scan_family(ix, k),
           "timing": "device events around Searcher.lists (router + scan + merge); per repeat the median of the "
                     "launches, the sides in turn inside every repeat, one process; scan_kernel_ms: lmi_timing",
           "by_nq": rows}
    out_path = a.out or os.path.join(ROOT, "profiles", f"few_scan_{a.scale}{'' if a.d == 768 else f'_d{a.d}'}.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
