#!/usr/bin/env python3
"""The l2 and ip scans (lmi_bucket_topk_metric) against the cosine scan
(lmi_bucket_topk) on the benchmark's workload, one GPU, one process:

    python tools/metric_scan_bench.py              # 10M x 768 -> profiles/metric_scan_10M.json
    python tools/metric_scan_bench.py --d 96       # the general kernel -> profiles/metric_scan_10M_d96.json
    python tools/metric_scan_bench.py --scale 300K

Three indexes over the same rows (li.synth.build_lmi_workload, labels = router
argmax), metric "cosine", "l2" and "ip".  Scan time: the call alone between
device events, the router's classes given -- per repeat the median of
--launches launches, the three sides taken in turn inside every repeat, every
side with its own workspace.  The cosine side is the yardstick.  Expectation to
confirm or refute: l2 costs the cosine's VALU work and ip drops the row-word
traffic, so both lie within a few of the cosine side's spreads; a side slower
than cosine by more than three times the larger spread (max - min of the
repeat medians) is flagged."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import DeviceIndex, DeviceRouter, bucket_topk, scan_family  # noqa: E402

SCALES = {"10M": 10_000_000, "1M": 1_000_000, "300K": 300_000}
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", default="10M", choices=list(SCALES))
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metric_scan_bench needs a HIP device (no CPU path)")
    n, nq, R, k = SCALES[a.scale], a.nq, a.R, a.k
    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, a.buckets, "MLP-5", DEV, d=a.d)
    router = DeviceRouter(layers, device=DEV)
    labels = router.argmax(xn)
    del xn
    classes = router.topr(qn, R)[0]

    def side(metric):
        ix = DeviceIndex(x, labels, a.buckets, device=DEV, metric=metric)
        assert ix.storage == "f16"
        ws = torch.empty_like(ix.workspace(nq, R, k, _lib.LMI_Q_F16))
        out = (torch.empty((nq, R, k), dtype=torch.float32, device=DEV),
               torch.empty((nq, R, k), dtype=torch.int32, device=DEV),
               torch.zeros((1,), dtype=torch.int32, device=DEV))
        return ix, (lambda: bucket_topk(ix, q, classes, k, qmode=_lib.LMI_Q_F16, out=out, ws=ws)), out

    sides = {m: side(m) for m in ("cosine", "l2", "ip")}
    medians = {m: [] for m in sides}
    launches = {m: [] for m in sides}
    for rep in range(-1, a.repeats):          # (repeat -1: every side's warm-up)
        for m, (_, fn, _) in sides.items():
            ms = []
            for _ in range(a.warmup if rep < 0 else a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            if rep >= 0:
                medians[m].append(float(np.median(ms)))
                launches[m].append([round(float(v), 4) for v in ms])
    for m, (_, _, out) in sides.items():
        assert int(out[2].item()) == 0, (m, int(out[2].item()))

    scan = {m: {"median_of_medians_ms": float(np.median(v)), "repeat_medians_ms": [round(t, 4) for t in v],
                "spread_ms": float(max(v) - min(v)), "launches_ms": launches[m]} for m, v in medians.items()}
    for m in ("l2", "ip"):
        over = scan[m]["median_of_medians_ms"] - scan["cosine"]["median_of_medians_ms"]
        spread = max(scan[m]["spread_ms"], scan["cosine"]["spread_ms"])
        scan[f"{m}_minus_cosine_ms"] = over
        scan[f"{m}_over_cosine"] = scan[m]["median_of_medians_ms"] / scan["cosine"]["median_of_medians_ms"]
        scan[f"{m}_slower_by_more_than_three_spreads"] = bool(over > 3 * spread)
    res = {"scale": a.scale, "n": n, "d": a.d, "nq": nq, "R": R, "k": k, "buckets": a.buckets,
           "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "family": {m: scan_family(ix, k) for m, (ix, _, _) in sides.items()},
           "timing": "device events around each call (classes given); per repeat the median of the launches, "
                     "the three sides in turn inside every repeat, one process",
           "scan": scan}
    out = a.out or os.path.join(ROOT, "profiles", f"metric_scan_{a.scale}{'' if a.d == 768 else f'_d{a.d}'}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"scan_ms": {m: scan[m]["median_of_medians_ms"] for m in sides},
                      "spread_ms": {m: scan[m]["spread_ms"] for m in sides},
                      **{key: v for key, v in scan.items() if key.endswith(("_over_cosine", "_three_spreads"))}}))


if __name__ == "__main__":
    main()
