#!/usr/bin/env python3
"""The tagged scan (lmi_bucket_topk_tagged) against the untagged one, on one GPU:

    python tools/tagged_scan_bench.py                  # 10M -> profiles/tagged_scan_10M.json
    python tools/tagged_scan_bench.py --n 300000 --tag 300K

An n x 768 fp16 corpus is generated in HBM (li.synth.torch_mixture) with random
bucket labels and random 6-bit tags, and indexed once tagged.  In one process,
after a warm-up of each side, --launches timed launches per side by device
events, the two sides of every comparison alternated launch by launch:

  (a) the cost of the predicate: the tagged scan with want = 0 against the
      untagged scan of the same index (selectivity 1), and the same call with
      avoid = a bit no row carries (the second word of the predicate)
  (b) per want word keeping ~1/2, ~1/8, ~1/64 of the rows: the tagged scan
      against the untagged scan of the index built from the eligible rows
      alone (the per-predicate index a caller would otherwise hold)
  (c) at the same points, recall@10 of "unfiltered k = 10, then post-filter"
      against the tagged lists, computed from the lists

and the JSON receives every mean with its spread (max - min) and all values.
--no-selectivity stops after (a).  --pkg DIR imports the `li` package from DIR
(another checkout's, for a run against the parent commit: alternate whole
processes of the two trees and compare their medians of (a))."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd")
if "--pkg" in sys.argv[1:-1]:
    PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import synth  # noqa: E402
from li.index import DeviceIndex, bucket_topk, want_words  # noqa: E402
try:
    from li.index import mask_words  # noqa: E402
except ImportError:      # (--pkg: a tree from before `avoid`)
    mask_words = None

DEV = "cuda:0"


def stats(v):
    return {"mean_ms": float(np.mean(v)), "median_ms": float(np.median(v)), "min_ms": float(min(v)),
            "max_ms": float(max(v)), "spread_ms": float(max(v) - min(v)),
            "all_ms": [round(float(x), 4) for x in v]}


def alternate(sides, launches, warmup):
    """{name: [ms]}: the sides launched in turn, each launch between device events."""
    out = {name: [] for name in sides}
    for rep in range(-warmup, launches):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                out[name].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="10M")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-selectivity", action="store_true", help="(a) only")
    ap.add_argument("--pkg", default=None, help="directory that holds the `li` package to measure")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tagged_scan_bench needs a HIP device (no CPU path)")
    n, nq, R, k, C, d = a.n, a.nq, a.R, a.k, a.buckets, 768
    x, centres = synth.torch_mixture(n, d, 400, a.seed, DEV)
    q, _ = synth.torch_mixture(nq, d, 400, a.seed + 7, DEV, centres=centres)
    g = torch.Generator(device=DEV)
    g.manual_seed(a.seed + 1)
    labels = torch.randint(0, C, (n,), generator=g, device=DEV)
    tags = torch.randint(0, 64, (n,), generator=g, device=DEV).cpu().numpy().astype(np.uint32)
    base = torch.randint(0, C, (nq, 1), generator=g, device=DEV)
    classes = ((base + 7 * torch.arange(R, device=DEV)) % C).to(torch.int32).contiguous()
    lab_host = labels.cpu().numpy()
    full = DeviceIndex.empty(d, C, device=DEV, tags=True).add(x, labels, tags=tags)

    def scan(index, want=None, avoid=None):
        if avoid is not None:
            ww = mask_words(index, want, avoid, nq, k)
        else:
            ww = None if want is None else want_words(index, want, nq, k)
        return lambda: bucket_topk(index, q, classes, k, want=ww)

    res = {"package": os.path.relpath(PKG, ROOT), "n": n, "d": d, "nq": nq, "R": R, "k": k, "buckets": C, "launches": a.launches,
           "warmup": a.warmup, "timing": "device events around each lmi_bucket_topk[_tagged] call, "
           "the two sides of a comparison alternated launch by launch in one process"}
    sides = {"untagged": scan(full), "tagged_want0": scan(full, 0)}
    if mask_words is not None:   # (tags are 6 bits wide: no row has bit 20)
        sides["tagged_want0_avoid_unused_bit"] = scan(full, 0, 1 << 20)
    t = alternate(sides, a.launches, a.warmup)
    res["predicate_cost"] = {name: stats(v) for name, v in t.items()}
    if a.no_selectivity:
        out = a.out or os.path.join(ROOT, "profiles", f"tagged_scan_{a.tag}.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"package": os.path.relpath(PKG, ROOT)} | {name: s["median_ms"] for name, s in res["predicate_cost"].items()}))
        return
    plain_d, plain_pos, _ = bucket_topk(full, q, classes, k)
    plain_pos = plain_pos.clone()
    res["selectivity"] = []
    for w in (1, 7, 63):
        m = (tags & np.uint32(w)) == np.uint32(w)
        keep = torch.from_numpy(m).to(DEV)
        elig = DeviceIndex.empty(d, C, device=DEV).add(x[keep], labels[keep],
                                                       ids=np.flatnonzero(m).astype(np.int64) + 1)
        t = alternate({"tagged": scan(full, w), "eligible_rows_index": scan(elig)}, a.launches, a.warmup)
        td, tp, _ = bucket_topk(full, q, classes, k, want=want_words(full, w, nq, k))
        ed, ep, _ = bucket_topk(elig, q, classes, k)
        torch.cuda.synchronize()
        same = bool(torch.equal(td, ed))
        # over-fetch: the unfiltered top-k, post-filtered, against the tagged lists
        tag_dev = full.tags                                     # int32 bits by position (one GPU)
        pp = plain_pos.long().clamp(min=0)
        ok = ((tag_dev[pp] & w) == w) & (plain_pos >= 0)
        truth_n = (tp >= 0).sum(-1)
        hit = torch.zeros_like(truth_n)
        for j in range(k):                                      # |post-filtered ∩ truth| per pair
            hit += (ok & (plain_pos == tp[..., j:j + 1]) & (tp[..., j:j + 1] >= 0)).any(-1).long()
        has = truth_n > 0
        recall = float((hit[has].double() / truth_n[has].double()).mean().item())
        res["selectivity"].append({
            "want": w, "kept_share": float(m.mean()), "eligible_rows": int(m.sum()),
            "tagged": stats(t["tagged"]), "eligible_rows_index": stats(t["eligible_rows_index"]),
            "lists_bitwise_equal_distances": same,
            "overfetch_k10_postfilter_recall_at_10": recall})
        del elig
        torch.cuda.empty_cache()
    out = a.out or os.path.join(ROOT, "profiles", f"tagged_scan_{a.tag}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({kk: (v if kk != "selectivity" else [
        {a_: b_ for a_, b_ in s.items() if not isinstance(b_, dict)} |
        {"tagged_mean_ms": s["tagged"]["mean_ms"], "eligible_mean_ms": s["eligible_rows_index"]["mean_ms"]}
        for s in v]) for kk, v in res.items() if kk != "predicate_cost"} |
        {"untagged_mean_ms": res["predicate_cost"]["untagged"]["mean_ms"],
         "tagged_want0_mean_ms": res["predicate_cost"]["tagged_want0"]["mean_ms"]}))


if __name__ == "__main__":
    main()
