#!/usr/bin/env python3
"""Re-ranking 16-entry 8-bit lists from kept fp16 rows against the fp16 index,
on one GPU:

    python tools/i8_rerank_bench.py                  # 10M -> profiles/i8_rerank_10M.json
    python tools/i8_rerank_bench.py --scale 300K

The benchmark's workload (li.synth.build_lmi_workload) is indexed in fp16 and
quantised on the device with quantized(keep_rows=True): the 8-bit index shares
the fp16 index's rows.  Then, in one process, the router's classes given:

  time     device events around each call: the median of --launches launches,
           --repeats times, the sides taken in turn inside every repeat --
             f16_f32        lmi_bucket_topk on the fp16 index (its 8-wave ring), k
             f16_f64        lmi_bucket_topk_f64 on the fp16 index, k
             i8_ring10      scan3_i8_kernel<10>, k
             i8_ring16      scan3_i8_kernel<16>, --k2 entries (bucket_topk(..., lists16=True):
                            the re-rank's scan)
             i8_v1_16       scan_i8_kernel (LMI_SCAN_V1=1) at --k2 entries: the kernel
                            that 11..16 entries run on by default
             rerank         lmi_rerank_f64 alone on the --k2-entry lists -> k
             i8_16_rerank   i8_ring16 followed by rerank
           (the switch is re-read between sides, lmi_config_reload; every scan
           has its own workspace).  Conditions, each "the median of medians lies
           below the other side's by more than the larger of the two sides'
           spreads (max - min of the repeat medians)": i8_ring16 below i8_v1_16,
           and i8_16_rerank below f16_f64.  The lists of i8_ring16 and i8_v1_16
           must be the same bits.  The re-rank's gather bandwidth: the bytes of
           the live candidates' rows over its time.
  quality  recall@10 of Searcher.search's answer on each side's lists against a
           brute force over the fp16 rows (--recall-sample queries): the fp16
           index in float32 and float64, the 8-bit index at k, the 8-bit index
           with rerank=--k2 (dist="f64")
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
from li.index import (DeviceIndex, DeviceRouter, Searcher, bucket_topk, bucket_topk_f64, rerank_f64,  # noqa: E402
                      scan_family)
from i8_scan_bench import SCALES, exact_knn, overlap  # noqa: E402

DEV = "cuda:0"


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
        sys.exit("i8_rerank_bench needs a HIP device (no CPU path)")
    n, nq, R, k, k2 = SCALES[a.scale], a.nq, a.R, a.k, a.k2
    lib = _lib.load()

    def note(msg):
        print(f"[i8_rerank_bench] {msg}", file=sys.stderr, flush=True)

    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, a.buckets, "MLP-5", DEV)
    note("workload built")
    router = DeviceRouter(layers, device=DEV)
    labels = router.argmax(xn)
    del xn
    f16 = DeviceIndex(x, labels, a.buckets, device=DEV)
    assert f16.storage == "f16"
    i8 = f16.quantized(keep_rows=True)
    assert i8.rows16.data_ptr() == f16.corpus.data_ptr()
    classes = router.topr(qn, R)[0]
    note("both indexes built")

    def knob(v1):
        if v1:
            os.environ["LMI_SCAN_V1"] = "1"
        else:
            os.environ.pop("LMI_SCAN_V1", None)
        lib.lmi_config_reload()

    def scan_side(index, kk, v1, family, lists16=False):
        def setup():
            knob(v1)
            got = scan_family(index, kk, lists16=lists16)
            assert got == family, (got, family)
        setup()
        qmode = _lib.LMI_Q_I8 if index.storage == "i8" else _lib.LMI_Q_F16
        prev = lib.lmi_scan_set_i8_lists16(1 if lists16 else 0)   # (the plan the launch will make)
        need = lib.lmi_scan_workspace_bytes(C.byref(index.desc), nq, R, kk, qmode)
        lib.lmi_scan_set_i8_lists16(prev)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        out = (torch.empty((nq, R, kk), dtype=torch.float32, device=DEV),
               torch.empty((nq, R, kk), dtype=torch.int32, device=DEV),
               torch.zeros((1,), dtype=torch.int32, device=DEV))
        return setup, (lambda: bucket_topk(index, q, classes, kk, qmode=qmode, out=out, ws=ws,
                                           lists16=lists16)), out

    out64 = (torch.empty((nq, R, k), dtype=torch.float64, device=DEV),
             torch.empty((nq, R, k), dtype=torch.int32, device=DEV),
             torch.zeros((1,), dtype=torch.int32, device=DEV))
    outrr = (torch.empty((nq, R, k), dtype=torch.float64, device=DEV),
             torch.empty((nq, R, k), dtype=torch.int32, device=DEV),
             torch.zeros((1,), dtype=torch.int32, device=DEV))
    ring16 = scan_side(i8, k2, False, "ring8-i8", lists16=True)
    sides = {
        "f16_f32": scan_side(f16, k, False, "ring8"),
        "f16_f64": (lambda: knob(False), lambda: bucket_topk_f64(f16, q, classes, k, qmode=_lib.LMI_Q_F16, out=out64),
                    out64),
        "i8_ring10": scan_side(i8, k, False, "ring8-i8"),
        "i8_ring16": ring16,
        "i8_v1_16": scan_side(i8, k2, True, "general"),
        "rerank": (lambda: knob(False), lambda: rerank_f64(i8, q, ring16[2][1], k, out=outrr), outrr),
        "i8_16_rerank": (ring16[0], lambda: (ring16[1](), rerank_f64(i8, q, ring16[2][1], k, out=outrr)), outrr),
    }
    medians = {name: [] for name in sides}
    launches = {name: [] for name in sides}
    for rep in range(-1, a.repeats):          # (repeat -1: every side's warm-up)
        for name, (setup, fn, _) in sides.items():
            setup()
            ms = []
            for i in range(a.warmup if rep < 0 else a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            if rep >= 0:
                medians[name].append(float(np.median(ms)))
                launches[name].append([round(float(v), 4) for v in ms])
        note(f"repeat {rep} done")
    knob(False)
    for name, (_, _, out) in sides.items():
        assert int(out[2].item()) == 0, (name, int(out[2].item()))
    same_lists = bool(torch.equal(sides["i8_ring16"][2][0].view(torch.int32),
                                  sides["i8_v1_16"][2][0].view(torch.int32)) and
                      torch.equal(sides["i8_ring16"][2][1], sides["i8_v1_16"][2][1]))
    assert same_lists, "the i8 ring's 16-entry lists differ from the general i8 kernel's"

    def summary(name):
        m = medians[name]
        return {"median_of_medians_ms": float(np.median(m)), "repeat_medians_ms": [round(v, 4) for v in m],
                "spread_ms": float(max(m) - min(m)), "launches_ms": launches[name]}

    times = {name: summary(name) for name in sides}

    def mm(name):
        return times[name]["median_of_medians_ms"]

    def below(fast, slow):
        gain = mm(slow) - mm(fast)
        times[f"{fast}_below_{slow}_by_ms"] = gain
        times[f"condition_{fast}_below_{slow}_by_more_than_the_larger_spread"] = bool(
            gain > max(times[fast]["spread_ms"], times[slow]["spread_ms"]))

    below("i8_ring16", "i8_v1_16")
    below("i8_16_rerank", "f16_f64")
    below("i8_16_rerank", "f16_f32")
    times["i8_ring16_over_i8_ring10"] = mm("i8_ring16") / mm("i8_ring10")
    times["i8_ring16_over_i8_v1_16"] = mm("i8_ring16") / mm("i8_v1_16")
    times["i8_16_rerank_over_f16_f64"] = mm("i8_16_rerank") / mm("f16_f64")
    times["i8_16_rerank_over_f16_f32"] = mm("i8_16_rerank") / mm("f16_f32")
    times["i8_ring16_lists_equal_i8_v1_16_lists"] = same_lists
    live = int((ring16[2][1] >= 0).sum().item())
    gather_bytes = live * i8.d_pad * 2
    times["rerank_live_candidates"] = live
    times["rerank_gather_bytes"] = gather_bytes
    times["rerank_gather_TBps"] = gather_bytes / (mm("rerank") * 1e-3) / 1e12

    # ---- quality ----------------------------------------------------------------------
    sample = min(a.recall_sample, nq)
    truth = exact_knn(x, q[:sample], k)
    s16, s8 = Searcher(f16, router), Searcher(i8, router)

    def recall(ans):
        return overlap(ans[1][:sample].astype(np.int64), truth, k)

    note("brute force done")
    ans_f64 = s16.search(qn, q, R, k=k, use_threshold=True, dist="f64")
    ans_rr = s8.search(qn, q, R, k=k, use_threshold=True, dist="f64", rerank=k2)
    quality = {"recall_sample": sample,
               "recall_at_k_f16_f32": recall(s16.search(qn, q, R, k=k, use_threshold=True)),
               "recall_at_k_f16_f64": recall(ans_f64),
               "recall_at_k_i8": recall(s8.search(qn, q, R, k=k, use_threshold=True)),
               "recall_at_k_i8_rerank": recall(ans_rr),
               "mean_top_k_overlap_i8_rerank_vs_f16_f64": overlap(ans_rr[1].astype(np.int64),
                                                                  ans_f64[1].astype(np.int64), k),
               "queries_with_the_f16_f64_answer": float(np.mean((ans_rr[1] == ans_f64[1]).all(axis=1))),
               "note": "the scan sides i8_ring16 / i8_v1_16 list 16 entries whose first 10 are i8_ring10's: "
                       "recall_at_k_i8; rerank and i8_16_rerank give recall_at_k_i8_rerank"}

    res = {"scale": a.scale, "n": n, "d": 768, "nq": nq, "R": R, "k": k, "k2": k2, "buckets": a.buckets,
           "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "device events around each call (classes given); per repeat the median of the launches, "
                     "the sides in turn inside every repeat, one process",
           "time": times, "quality": quality}
    out = a.out or os.path.join(ROOT, "profiles", f"i8_rerank_{a.scale}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms": {s: round(mm(s), 4) for s in sides},
                      "spread_ms": {s: round(times[s]["spread_ms"], 4) for s in sides},
                      "condition_ring16_below_general": times[
                          "condition_i8_ring16_below_i8_v1_16_by_more_than_the_larger_spread"],
                      "condition_rerank_path_below_f16_f64": times[
                          "condition_i8_16_rerank_below_f16_f64_by_more_than_the_larger_spread"],
                      "rerank_gather_TBps": times["rerank_gather_TBps"], **quality}))


if __name__ == "__main__":
    main()
