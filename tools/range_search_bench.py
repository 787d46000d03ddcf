#!/usr/bin/env python3
"""Range search (K11) against the top-k lists it replaces a guess of, on one GPU:

    python tools/range_search_bench.py                 # 10M -> profiles/range_search_10M.json
    python tools/range_search_bench.py --size 300K

bench.py's synthetic index (n x 768 fp16, 122 buckets, the fitted router),
10 000 queries, R = 4.  Two per-query radii: each query's 10th-nearest and its
1 000th-nearest float32 distance over its probed buckets (from the lists).  In
one process, after a warm-up of each, --reps rounds alternate

  range_search(dist="f32") and (dist="f64") per radius choice: the stages by
      its `timings` (scan, rescore, pack, sort, d2h; stream synchronisations
      between them) and the whole call by a host clock to the host arrays
  the collect scan alone (bucket_range) by device events
  Searcher.lists(k_list=10) in both arithmetics and lists(k_list=1000) in
      float32, by device events: the yardsticks

and the general kernel's collect form on its own: bucket_range over an
n x 96 fp16 corpus with the same labels (the width tagged calls and every
width but 768 run), against lists(k_list=10) there.  The JSON holds every time
with its spread, results per query, the second scans that ran at the default
pair_cap and the ratios range / lists."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import synth  # noqa: E402
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_range  # noqa: E402

DEV = "cuda:0"
SIZES = {"10M": 10_000_000, "1M": 1_000_000, "300K": 300_000}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                       # ms


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
            "spread_ms": float(max(v) - min(v)), "all_ms": [round(float(x), 4) for x in v]}


def kth_over_probes(d, k):
    """the k-th smallest of every query's R lists [nq, R, k_list] (float32, device)."""
    return torch.sort(d.reshape(d.shape[0], -1), dim=1).values[:, k - 1].contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="10M", choices=list(SIZES))
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("range_search_bench needs a HIP device (no CPU path)")
    n, nq, R, C = SIZES[a.size], a.nq, a.R, a.buckets
    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, C, "MLP-5", DEV)
    router = DeviceRouter(layers, device=DEV)
    labels = router.argmax(xn)
    del xn
    s = Searcher(DeviceIndex(x, labels, C, device=DEV), router)
    del x
    classes = s.route(qn, R)
    qmode = s.qmode(q)

    # the radii, from the lists
    d10 = s.lists(None, q, R, 10, classes=classes)[1]
    d1000 = s.lists(None, q, R, 1000, classes=classes)[1]
    radii = {"r10": kth_over_probes(d10, 10), "r1000": kth_over_probes(d1000, 1000)}
    del d1000

    runs = {}

    def add(name, fn):
        runs[name] = fn

    for rn, r in radii.items():
        for dist in ("f32", "f64"):
            def whole(r=r, dist=dist, rn=rn):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lims, _, _ = s.range_search(None, q, R, r, classes=classes, dist=dist, timings=tm)
                tm["total_ms"] = (time.perf_counter() - t0) * 1e3
                tm["results_per_query"] = float(lims[-1]) / nq
                return tm
            add(f"range_{rn}_{dist}", whole)
        add(f"collect_scan_{rn}", lambda r=r: {"ms": events(
            lambda: bucket_range(s.index, q, classes, r, qmode=qmode))})
    add("lists_k10_f32", lambda: {"ms": events(lambda: s.lists(None, q, R, 10, classes=classes))})
    add("lists_k10_f64", lambda: {"ms": events(lambda: s.lists(None, q, R, 10, classes=classes, dist="f64"))})
    add("lists_k1000_f32", lambda: {"ms": events(lambda: s.lists(None, q, R, 1000, classes=classes))})

    # the general kernel's collect form on its own: the same labels, 96 wide
    x96, cen = synth.torch_mixture(n, 96, 400, seed=2023, device=DEV)
    q96, _ = synth.torch_mixture(nq, 96, 400, seed=4242, device=DEV, centres=cen, out_dtype=torch.float32)
    s96 = Searcher(DeviceIndex(x96, labels, C, device=DEV), None)
    del x96
    r96 = kth_over_probes(s96.lists(None, q96, R, 10, classes=classes)[1], 10)
    add("general96_collect_scan_r10", lambda: {"ms": events(
        lambda: bucket_range(s96.index, q96, classes, r96, qmode=s96.qmode(q96)))})
    add("general96_lists_k10_f32", lambda: {"ms": events(lambda: s96.lists(None, q96, R, 10, classes=classes))})

    for fn in runs.values():                         # warm-up (allocations, attributes)
        fn()
    got = {k: [] for k in runs}
    for _ in range(a.reps):                          # interleaved
        for k, fn in runs.items():
            got[k].append(fn())
    out = {"size": a.size, "n": n, "d": 768, "nq": nq, "R": R, "buckets": C, "reps": a.reps,
           "pair_cap": 256, "device": torch.cuda.get_device_name(0),
           "how": "one process, interleaved repeats after a warm-up of each; device events for scans and "
                  "lists, range_search's own stage timings (stream synchronisations between stages) and a "
                  "host clock for the whole call"}
    for k, v in got.items():
        if "ms" in v[0]:
            out[k] = stats([t["ms"] for t in v])
            continue
        e = {"total": stats([t["total_ms"] for t in v]), "results_per_query": v[0]["results_per_query"],
             "scans": v[0]["scans"], "second_scans": v[0]["scans"] - 1}
        for stage in ("scan", "rescore", "pack", "sort", "d2h"):
            if stage in v[0]:
                e[stage] = stats([t[stage] for t in v])
        out[k] = e
    med = lambda k: out[k]["total"]["median_ms"] if "total" in out[k] else out[k]["median_ms"]
    out["ratios"] = {
        "range_r10_f32 / lists_k10_f32": med("range_r10_f32") / med("lists_k10_f32"),
        "range_r10_f64 / lists_k10_f64": med("range_r10_f64") / med("lists_k10_f64"),
        "range_r1000_f32 / lists_k1000_f32": med("range_r1000_f32") / med("lists_k1000_f32"),
        "collect_scan_r10 / lists_k10_f32": med("collect_scan_r10") / med("lists_k10_f32"),
        "general96_collect_scan_r10 / general96_lists_k10_f32":
            med("general96_collect_scan_r10") / med("general96_lists_k10_f32"),
    }
    path = a.out or os.path.join(ROOT, "profiles", f"range_search_{a.size}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("ratios",)}, indent=1))
    for k in got:
        print(k, round(med(k), 3), "ms")


if __name__ == "__main__":
    main()
