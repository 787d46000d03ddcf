#!/usr/bin/env python3
"""The 8-bit storage (storage "i8") against the fp16 index, on one GPU:

    python tools/i8_scan_bench.py                  # 10M -> profiles/i8_ring_10M.json
    python tools/i8_scan_bench.py --scale 300K

The benchmark's workload (li.synth.build_lmi_workload: the clip768-like mixture,
a router fitted to k-means buckets, labels = router argmax) is indexed in fp16
and quantised on the device (DeviceIndex.quantized, timed).  Then, in one
process:

  scan time   lmi_bucket_topk alone between device events, the router's classes
              given: the median of --launches launches, --repeats times, the
              four sides taken in turn inside every repeat --
                i8_ring   scan3_i8_kernel, the 8-wave ring the i8 index runs by
                          default at this width (k <= 10)
                i8        scan_i8_kernel on the i8 index (LMI_SCAN_V1=1): the
                          general kernel's structure, what every other i8 shape runs
                f16_v1    the fp16 general kernel on the fp16 index (LMI_SCAN_V1=1):
                          the same structure at twice the bytes and MFMA cycles
                f16_ring  the 8-wave ring, what the fp16 index runs by default
              (the switch is re-read between sides, lmi_config_reload; every
              side has its own workspace).  Two conditions, each "the median of
              medians lies below the other side's by more than the larger of
              the two sides' spreads (max - min of the repeat medians)": i8_ring
              below i8, and i8 below f16_v1.  Against the fp16 ring the ratios
              are reported whatever they are.  The lists of i8_ring and i8 must
              be the same bits.
  quality     recall@10 of Searcher.search on either index against a brute
              force over the fp16 rows (--recall-sample queries), and the mean
              top-10 overlap of the two answers over the whole batch; the i8
              answer is taken on the ring and under LMI_SCAN_V1=1 and must be
              one answer
  footprint   resident bytes of both indexes; quantized(): seconds and GB/s
              (fp16 bytes read + code bytes written)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_topk, scan_family  # noqa: E402

SCALES = {"10M": 10_000_000, "1M": 1_000_000, "300K": 300_000}
DEV = "cuda:0"


@torch.no_grad()
def exact_knn(x, qs, k, chunk=1 << 20):
    """Exact cosine k-NN ids (1-based) of the sample queries over the fp16 rows."""
    qn = qs / qs.norm(dim=1, keepdim=True)
    best_s = torch.full((qs.shape[0], k), -2.0, device=qs.device)
    best_i = torch.zeros((qs.shape[0], k), dtype=torch.int64, device=qs.device)
    for a in range(0, x.shape[0], chunk):
        blk = x[a:a + chunk].float()
        v, i = (qn @ (blk / blk.norm(dim=1, keepdim=True)).T).topk(k, dim=1)
        cs, ci = torch.cat([best_s, v], 1), torch.cat([best_i, i + a], 1)
        o = cs.topk(k, dim=1).indices
        best_s, best_i = cs.gather(1, o), ci.gather(1, o)
    return (best_i + 1).cpu().numpy()


def resident_bytes(ix):
    return int(sum(t.numel() * t.element_size() for t in (ix.corpus, ix.inv_norm, ix.gpos)))


def overlap(a, b, k):
    return float(np.mean([len(set(a[i][:k]) & set(b[i][:k])) / k for i in range(a.shape[0])]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", default="10M", choices=list(SCALES))
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recall-sample", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("i8_scan_bench needs a HIP device (no CPU path)")
    n, nq, R, k = SCALES[a.scale], a.nq, a.R, a.k
    lib = _lib.load()
    x, q, qn, xn, layers = synth.build_lmi_workload(n, nq, a.buckets, "MLP-5", DEV)
    router = DeviceRouter(layers, device=DEV)
    labels = router.argmax(xn)
    del xn
    f16 = DeviceIndex(x, labels, a.buckets, device=DEV)
    assert f16.storage == "f16"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    i8 = f16.quantized()                      # (returns after a stream synchronisation)
    t_quant = time.perf_counter() - t0
    classes = router.topr(qn, R)[0]

    # ---- scan time -------------------------------------------------------------------
    def side(index, v1, family):
        def setup():
            if v1:
                os.environ["LMI_SCAN_V1"] = "1"
            else:
                os.environ.pop("LMI_SCAN_V1", None)
            lib.lmi_config_reload()
            assert scan_family(index, k) == family, (scan_family(index, k), family)
        setup()
        qmode = _lib.LMI_Q_I8 if index.storage == "i8" else _lib.LMI_Q_F16
        need = lib.lmi_scan_workspace_bytes(C.byref(index.desc), nq, R, k, qmode)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
        out = (torch.empty((nq, R, k), dtype=torch.float32, device=DEV),
               torch.empty((nq, R, k), dtype=torch.int32, device=DEV),
               torch.zeros((1,), dtype=torch.int32, device=DEV))
        return setup, (lambda: bucket_topk(index, q, classes, k, qmode=qmode, out=out, ws=ws)), out

    sides = {"i8_ring": side(i8, False, "ring8-i8"), "i8": side(i8, True, "general"),
             "f16_v1": side(f16, True, "general"), "f16_ring": side(f16, False, "ring8")}
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
    for name, (_, _, out) in sides.items():
        assert int(out[2].item()) == 0, (name, int(out[2].item()))
    same_lists = bool(torch.equal(sides["i8_ring"][2][0].view(torch.int32), sides["i8"][2][0].view(torch.int32)) and
                      torch.equal(sides["i8_ring"][2][1], sides["i8"][2][1]))
    assert same_lists, "the i8 ring's lists differ from the general i8 kernel's"
    os.environ.pop("LMI_SCAN_V1", None)
    lib.lmi_config_reload()

    def summary(name):
        m = medians[name]
        return {"median_of_medians_ms": float(np.median(m)), "repeat_medians_ms": [round(v, 4) for v in m],
                "spread_ms": float(max(m) - min(m)), "launches_ms": launches[name]}

    scan = {name: summary(name) for name in sides}

    def mm(name):
        return scan[name]["median_of_medians_ms"]

    def below(fast, slow):
        gain = mm(slow) - mm(fast)
        scan[f"{fast}_below_{slow}_by_ms"] = gain
        scan[f"condition_{fast}_below_{slow}_by_more_than_the_larger_spread"] = bool(
            gain > max(scan[fast]["spread_ms"], scan[slow]["spread_ms"]))

    below("i8_ring", "i8")
    below("i8", "f16_v1")
    scan["i8_ring_over_i8"] = mm("i8_ring") / mm("i8")
    scan["i8_over_f16_v1"] = mm("i8") / mm("f16_v1")
    scan["i8_over_f16_ring"] = mm("i8") / mm("f16_ring")
    scan["i8_ring_over_f16_ring"] = mm("i8_ring") / mm("f16_ring")
    scan["i8_ring_lists_equal_i8_lists"] = same_lists

    # ---- quality ----------------------------------------------------------------------
    ans16 = Searcher(f16, router).search(qn, q, R, k=k, use_threshold=True)[1]
    ans8 = Searcher(i8, router).search(qn, q, R, k=k, use_threshold=True)[1]
    os.environ["LMI_SCAN_V1"] = "1"
    lib.lmi_config_reload()
    try:
        ans8_v1 = Searcher(i8, router).search(qn, q, R, k=k, use_threshold=True)[1]
    finally:
        os.environ.pop("LMI_SCAN_V1", None)
        lib.lmi_config_reload()
    assert np.array_equal(ans8, ans8_v1), "the i8 answers on the ring and on the general kernel differ"
    sample = min(a.recall_sample, nq)
    truth = exact_knn(x, q[:sample], k)
    quality = {"recall_sample": sample,
               "recall_at_k_f16": overlap(ans16[:sample].astype(np.int64), truth, k),
               "recall_at_k_i8": overlap(ans8[:sample].astype(np.int64), truth, k),
               "i8_answer_on_the_ring_equals_the_general_kernels": True,
               "mean_top_k_overlap_i8_vs_f16": overlap(ans8.astype(np.int64), ans16.astype(np.int64), k)}

    # ---- footprint --------------------------------------------------------------------
    moved = f16.corpus.numel() * 2 + i8.corpus.numel()
    footprint = {"f16_resident_bytes": resident_bytes(f16), "i8_resident_bytes": resident_bytes(i8),
                 "quantized_seconds": t_quant, "quantized_GBps": moved / t_quant / 1e9,
                 "quantized_bytes_moved": int(moved)}

    res = {"scale": a.scale, "n": n, "d": 768, "nq": nq, "R": R, "k": k, "buckets": a.buckets,
           "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "timing": "device events around each lmi_bucket_topk call (classes given); per repeat the median of "
                     "the launches, the four sides in turn inside every repeat, one process",
           "scan": scan, "quality": quality, "footprint": footprint}
    out = a.out or os.path.join(ROOT, "profiles", f"i8_ring_{a.scale}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"scan_ms": {s: scan[s]["median_of_medians_ms"] for s in sides},
                      "spread_ms": {s: scan[s]["spread_ms"] for s in sides},
                      "condition_ring_below_general_i8": scan[
                          "condition_i8_ring_below_i8_by_more_than_the_larger_spread"],
                      "i8_ring_over_i8": scan["i8_ring_over_i8"],
                      "i8_ring_over_f16_ring": scan["i8_ring_over_f16_ring"], **quality, **footprint}))


if __name__ == "__main__":
    main()
