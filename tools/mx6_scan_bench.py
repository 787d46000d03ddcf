#!/usr/bin/env python3
"""The 6-bit ring (storage "mx6") against the 4-bit, 8-bit and fp16 rings, on one GPU:

    python tools/mx6_scan_bench.py                  # 10M -> profiles/mx6_ring_10M.json
    python tools/mx6_scan_bench.py --scale 300K

The benchmark's workload (li.synth.build_lmi_workload) is indexed in fp16 and
quantised on the device three times, quantized(storage=s, keep_rows=True) for s
in "i8", "mx4", "mx6": all share the fp16 index's rows.  Then, in one process,
the router's classes given:

  time     device events around each call: the median of --launches launches,
           --repeats times, the sides taken in turn inside every repeat --
             f16_ring       lmi_bucket_topk on the fp16 index (its 8-wave ring), k
             <s>_ring10 / <s>_ring16   the storage's ring, k and --k2 entries
             <s>_16_rerank  the 16-entry scan + lmi_rerank_f64 -> k
             f16_f64        lmi_bucket_topk_f64 on the fp16 index, k
           and the three quantisers over the whole fp16 store (one launch each,
           --repeats times).  No ratio is a condition: the numbers are reported
           with their spreads (max - min of the repeat medians).
  quality  recall@10 of Searcher.search's answer on each side's lists against a
           brute force over the fp16 rows (--recall-sample queries)
  bytes    what each index keeps resident for its scan (codes, scales, norms)
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import (DeviceIndex, DeviceRouter, Searcher, bucket_topk, bucket_topk_f64, quantize_rows,  # noqa: E402
                      quantize_rows_mx4, quantize_rows_mx6, rerank_f64, scan_family)
from i8_scan_bench import SCALES, exact_knn, overlap  # noqa: E402

DEV = "cuda:0"
QMODE = {"i8": _lib.LMI_Q_I8, "mx4": _lib.LMI_Q_MX4, "mx6": _lib.LMI_Q_MX6, "f16": _lib.LMI_Q_F16}
FAMILY = {"i8": "ring8-i8", "mx4": "ring8-mx4", "mx6": "ring8-mx6", "f16": "ring8"}
LOSSY = ("i8", "mx4", "mx6")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", default="10M", choices=list(SCALES))
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--k2", type=int, default=16)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recall-sample", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx6_scan_bench needs a HIP device (no CPU path)")
    n, nq, R, k, k2 = SCALES[a.scale], a.nq, a.R, a.k, a.k2
    lib = _lib.load()

    def note(msg):
        print(f"[mx6_scan_bench] {msg}", file=sys.stderr, flush=True)

    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, a.buckets, "MLP-5", DEV)
    router = DeviceRouter(layers, device=DEV)
    labels = router.argmax(xn)
    del xn
    f16 = DeviceIndex(x, labels, a.buckets, device=DEV)
    assert f16.storage == "f16"
    ix = {s: f16.quantized(storage=s, keep_rows=True) for s in LOSSY}
    classes = router.topr(qn, R)[0]
    note("the four indexes built")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def scan_side(index, kk):
        lists16 = kk > 10 and index.storage != "f16"
        assert scan_family(index, kk, lists16=lists16) == FAMILY[index.storage]
        qmode = QMODE[index.storage]
        prev = lib.lmi_scan_set_i8_lists16(1 if lists16 else 0)   # (the plan the launch will make)
        need = lib.lmi_scan_workspace_bytes(C.byref(index.desc), nq, R, kk, qmode)
        lib.lmi_scan_set_i8_lists16(prev)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        out = (torch.empty((nq, R, kk), dtype=torch.float32, device=DEV),
               torch.empty((nq, R, kk), dtype=torch.int32, device=DEV),
               torch.zeros((1,), dtype=torch.int32, device=DEV))
        return (lambda: bucket_topk(index, q, classes, kk, qmode=qmode, out=out, ws=ws, lists16=lists16)), out

    def out64():
        return (torch.empty((nq, R, k), dtype=torch.float64, device=DEV),
                torch.empty((nq, R, k), dtype=torch.int32, device=DEV),
                torch.zeros((1,), dtype=torch.int32, device=DEV))

    def rerank_side(index, side16):
        o = out64()
        return (lambda: (side16[0](), rerank_f64(index, q, side16[1][1], k, out=o))), o

    o64 = out64()
    sides = {"f16_ring": scan_side(f16, k)}
    for s in LOSSY:
        sides[f"{s}_ring10"], sides[f"{s}_ring16"] = scan_side(ix[s], k), scan_side(ix[s], k2)
    for s in LOSSY:
        sides[f"{s}_16_rerank"] = rerank_side(ix[s], sides[f"{s}_ring16"])
    sides["f16_f64"] = (lambda: bucket_topk_f64(f16, q, classes, k, qmode=_lib.LMI_Q_F16, out=o64)), o64
    medians = {name: [] for name in sides}
    for rep in range(-1, a.repeats):          # (repeat -1: every side's warm-up)
        for name, (fn, _) in sides.items():
            ms = [timed(fn) for _ in range(a.warmup if rep < 0 else a.launches)]
            if rep >= 0:
                medians[name].append(float(np.median(ms)))
        note(f"repeat {rep} done")
    for name, (_, out) in sides.items():
        assert int(out[2].item()) == 0, (name, int(out[2].item()))

    # the quantisers over the whole fp16 store, into scratch stores of their own
    rows, nr, dp = f16.corpus[:, : f16.d], f16.n_rows, f16.d_pad
    inv = torch.empty((nr,), dtype=torch.float32, device=DEV)
    sc = torch.empty((nr, dp // 32), dtype=torch.uint8, device=DEV)
    quant = {}
    for s, width, fn in (("i8", dp, None), ("mx4", dp // 2, quantize_rows_mx4), ("mx6", dp // 4 * 3, quantize_rows_mx6)):
        c = torch.empty((nr, width), dtype=torch.int8 if fn is None else torch.uint8, device=DEV)
        run = (lambda: quantize_rows(rows, dp, c, inv)) if fn is None else (lambda: fn(rows, dp, c, sc, inv))
        quant[s] = [timed(run) for _ in range(a.repeats + 1)][1:]
        del c
    del sc, inv

    def summary(m):
        return {"median_of_medians_ms": float(np.median(m)), "repeat_medians_ms": [round(v, 4) for v in m],
                "spread_ms": float(max(m) - min(m))}

    times = {name: summary(m) for name, m in medians.items()}
    for s in LOSSY:
        times[f"quantize_{s}"] = summary(quant[s])

    def mm(name):
        return times[name]["median_of_medians_ms"]

    ratios = {f"{a_}_over_{b_}": mm(a_) / mm(b_) for a_, b_ in (
        ("mx6_ring10", "mx4_ring10"), ("mx6_ring16", "mx4_ring16"), ("mx6_ring10", "i8_ring10"),
        ("mx6_ring16", "i8_ring16"), ("mx6_ring10", "f16_ring"), ("mx6_16_rerank", "i8_16_rerank"),
        ("mx6_16_rerank", "mx4_16_rerank"), ("mx6_16_rerank", "f16_f64"), ("mx4_16_rerank", "i8_16_rerank"))}

    # ---- quality ----------------------------------------------------------------------
    sample = min(a.recall_sample, nq)
    truth = exact_knn(x, q[:sample], k)
    note("brute force done")

    def recall(index, **kw):
        ans = Searcher(index, router).search(qn, q, R, k=k, use_threshold=True, **kw)
        return overlap(ans[1][:sample].astype(np.int64), truth, k)

    quality = {"recall_sample": sample,
               "recall_at_k_f16_ring": recall(f16), "recall_at_k_f16_f64": recall(f16, dist="f64")}
    for s in LOSSY:
        quality[f"recall_at_k_{s}"] = recall(ix[s])
        quality[f"recall_at_k_{s}_16_rerank"] = recall(ix[s], dist="f64", rerank=k2)
    resident = {"f16": f16.corpus.numel() * 2 + f16.inv_norm.numel() * 4}
    for s in LOSSY:
        resident[s] = ix[s].corpus.numel() + ix[s].inv_norm.numel() * 4
    res = {"scale": a.scale, "n": n, "d": 768, "nq": nq, "R": R, "k": k, "k2": k2, "buckets": a.buckets,
           "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "device events around each call (classes given); per repeat the median of the launches, "
                     "the sides in turn inside every repeat, one process; the quantisers: one launch a repeat",
           "time": times, "ratios": ratios, "quality": quality, "resident_bytes": resident}
    out = a.out or os.path.join(ROOT, "profiles", f"mx6_ring_{a.scale}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms": {s: round(mm(s), 4) for s in times},
                      "spread_ms": {s: round(times[s]["spread_ms"], 4) for s in times},
                      **{r: round(v, 4) for r, v in ratios.items()}, **quality, "resident_bytes": resident}))


if __name__ == "__main__":
    main()
