#!/usr/bin/env python3
"""Index re-bucket in place against the copying one (K10: lmi_perm_involutions,
lmi_index_swap_rows in csrc/lmi_rebucket.hip), on one GPU:

    python tools/index_rebucket_inplace_bench.py --n 10000000 --tag 10M
    python tools/index_rebucket_inplace_bench.py --n 300000 --tag 300K

The corpus, the router labels and the two new label sets ('recluster',
'random') are those of tools/index_rebucket_bench.py.  In one process, per
label set, after a warm-up, --reps rounds measure on the SAME corpus

  (a) lmi_index_gather_rows into a second buffer (device events)
  (b) index.relabel(labels) from the call to its return (host clock), and the
      rise of the allocator's peak over it
  (c) index.relabel(labels, inplace=True) likewise; the in-place call consumes
      its index, so the rounds alternate between the new labels and the old
      ones (every round moves as many rows), and the index of the last round
      is compared with the copying relabel of the same labels
  (d) the last round with the stage clock on, and then the plan
      (lmi_perm_involutions, with its doubling rounds) and each swap pass alone
      by device events, --reps times each, for the move between the same two
      label sets once more; rows and bytes moved per pass

and profiles/index_rebucket_inplace_<tag>.json receives every time as median
[min, max] and the rates."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from index_rebucket_bench import DEV, events, router_labels, stats, wall  # noqa: E402
from li import _lib, synth  # noqa: E402
from li.index import DeviceIndex  # noqa: E402


def rise(fn):
    """(result, ms to the return, rise of the allocator's peak in bytes)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    out, ms = wall(fn)
    return out, ms, torch.cuda.max_memory_allocated(DEV) - base


def same(a, b):
    return bool(torch.equal(a.corpus, b.corpus) and torch.equal(a.inv_norm, b.inv_norm)
                and np.array_equal(a.pos_to_id, b.pos_to_id)
                and np.array_equal(a.layout.order, b.layout.order)
                and torch.equal(a.chunk_first, b.chunk_first)
                and torch.equal(a.bucket_off_local, b.bucket_off_local))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("index_rebucket_inplace_bench needs a HIP device (no CPU path)")
    lib = _lib.load()
    n, d, C = a.n, a.d, a.buckets
    x, _ = synth.torch_mixture(n, d, 400, a.seed, DEV)
    g = torch.Generator(device="cpu")
    g.manual_seed(96)
    xn = synth.torch_nav(x, (torch.randn((d, 96), generator=g) / d ** 0.5).to(DEV))
    lab_old = router_labels(xn, C, 7)
    gd = torch.Generator(device=DEV)
    gd.manual_seed(a.seed + 1)
    sets = {"recluster": router_labels(xn, C, 8),
            "random": torch.randint(0, C, (n,), generator=gd, device=DEV)}
    del xn
    index = DeviceIndex.empty(d, C, device=DEV).add(x, lab_old)
    del x
    d_pad = index.d_pad
    row_b = 2 * d_pad + 4
    corpus_bytes = n * d_pad * 2
    s = _lib.stream_handle(DEV)
    rate = lambda b, ms: b / (ms * 1e-3) / 1e9       # GB/s
    out = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "d_pad": d_pad, "buckets": C,
           "reps": a.reps, "corpus_bytes": corpus_bytes,
           "plan_workspace_bytes": int(lib.lmi_perm_involutions_ws_bytes(n)),
           "plan_bytes_per_row": (lib.lmi_perm_involutions_ws_bytes(n) + 16 * n) / n,
           "bytes_model": {"gather": 2 * n * row_b, "swap_pass": "2 * swapped_rows * (2 d_pad + 4)"}}
    for name, lab in sets.items():
        t = {k: [] for k in ("gather_ms", "relabel_ms", "relabel_inplace_ms", "plan_ms", "swap1_ms",
                             "swap2_ms")}
        peak = {"relabel": [], "relabel_inplace": []}
        cur, cur_lab = index, lab_old                # the index the in-place rounds hand on
        for rep in range(-1, a.reps):                # round -1: the warm-up
            target = lab if cur_lab is lab_old else lab_old
            # (a) the gather kernel alone, into a second corpus
            order, _ = DeviceIndex._sorted_by_bucket(target, C)
            inv = torch.empty(n, dtype=torch.int64, device=DEV)
            inv[torch.from_numpy(cur.layout.order).to(DEV)] = torch.arange(n, dtype=torch.int64, device=DEV)
            src_pos = inv[order]
            del inv, order
            dst = torch.empty((n, d_pad), dtype=torch.float16, device=DEV)
            dst_inv = torch.empty((n,), dtype=torch.float32, device=DEV)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            gather_ms = events(lambda: _lib.check("lmi_index_gather_rows", lib.lmi_index_gather_rows(
                cur.corpus.data_ptr(), cur.inv_norm.data_ptr(), n, d_pad, src_pos.data_ptr(),
                dst.data_ptr(), dst_inv.data_ptr(), n, status.data_ptr(), s)))
            assert int(status.item()) == 0
            del dst, dst_inv, src_pos
            # (b) the copying relabel, (c) the one in place; the last round with the stage clock
            copied, relabel_ms, up_copy = rise(lambda: cur.relabel(target))
            stages = {} if rep in (-1, a.reps - 1) else None   # (the warm-up warms the stage clock too)
            new, inplace_ms, up_inplace = rise(lambda: cur.relabel(target, inplace=True, timings=stages))
            if rep == a.reps - 1:
                out.setdefault("equal", {})[name] = same(new, copied)
                out.setdefault("stages", {})[name] = {
                    "seconds": {k: v for k, v in stages.items() if isinstance(v, float) and not k.endswith("_ms")},
                    "plan_ms": stages["plan_ms"], "plan_rounds": stages["plan_rounds"],
                    "swap_ms": stages["swap_ms"], "swapped_rows": stages["swapped_rows"],
                    "swap_bytes": [2 * r * row_b for r in stages["swapped_rows"]],
                    "swap_GBps": [rate(2 * r * row_b, ms) for r, ms in
                                  zip(stages["swapped_rows"], stages["swap_ms"])]}
            del copied
            cur, cur_lab = new, target
            if rep >= 0 and stages is None:
                t["gather_ms"].append(gather_ms)
                t["relabel_ms"].append(relabel_ms)
                t["relabel_inplace_ms"].append(inplace_ms)
                peak["relabel"].append(int(up_copy))
                peak["relabel_inplace"].append(int(up_inplace))
        # the plan and the passes alone, by device events, on the index as it is now: the move
        # between the same two label sets once more (towards the one the index does not have)
        target = lab if cur_lab is not lab else lab_old
        index, lab_old = cur, cur_lab                # the next label set goes on from here
        order, _ = DeviceIndex._sorted_by_bucket(target, C)
        inv = torch.empty(n, dtype=torch.int64, device=DEV)
        inv[torch.from_numpy(index.layout.order).to(DEV)] = torch.arange(n, dtype=torch.int64, device=DEV)
        src_pos = inv[order]
        del inv, order
        p1 = torch.empty(n, dtype=torch.int64, device=DEV)
        p2 = torch.empty(n, dtype=torch.int64, device=DEV)
        need = lib.lmi_perm_involutions_ws_bytes(n)
        ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        for rep in range(-1, a.reps):
            ms = events(lambda: _lib.check("lmi_perm_involutions", lib.lmi_perm_involutions(
                src_pos.data_ptr(), n, p1.data_ptr(), p2.data_ptr(), status.data_ptr(), ws.data_ptr(),
                need, s)))
            if rep >= 0:
                t["plan_ms"].append(ms)
        assert int(status.item()) == 0
        at = torch.arange(n, dtype=torch.int64, device=DEV)
        moved = [2 * int((p > at).sum()) for p in (p1, p2)]
        del ws, at
        # a pass applied twice puts every row back: the corpus is as before after each pair of calls
        for key, p in (("swap1_ms", p1), ("swap2_ms", p2)):
            for rep in range(-1, a.reps + (a.reps + 1) % 2):   # an even number of calls
                ms = events(lambda: _lib.check("lmi_index_swap_rows", lib.lmi_index_swap_rows(
                    index.corpus.data_ptr(), index.inv_norm.data_ptr(), n, d_pad, p.data_ptr(),
                    status.data_ptr(), s)))
                if rep >= 0:
                    t[key].append(ms)
        assert int(status.item()) == 0
        del p1, p2, src_pos
        r = {k: stats(v) for k, v in t.items()}
        med = lambda k: r[k]["median_ms"]
        r["plan_rounds"] = 2 * max(0, (n - 1).bit_length())
        r["plan_ms_per_round"] = med("plan_ms") / max(1, r["plan_rounds"])
        r["swapped_rows"] = moved
        r["swap_bytes"] = [2 * m * row_b for m in moved]
        r["gather_GBps"] = rate(out["bytes_model"]["gather"], med("gather_ms"))
        r["swap_GBps"] = [rate(b, med(k)) for b, k in zip(r["swap_bytes"], ("swap1_ms", "swap2_ms"))]
        r["swaps_over_gather_ms"] = (med("swap1_ms") + med("swap2_ms")) / med("gather_ms")
        r["inplace_over_relabel_ms"] = med("relabel_inplace_ms") / med("relabel_ms")
        r["peak_rise_bytes"] = {k: {"median": int(np.median(v)), "max": int(max(v))} for k, v in peak.items()}
        r["peak_rise_over_corpus"] = {k: max(v) / corpus_bytes for k, v in peak.items()}
        out[name] = r
    tag = a.tag or str(n)
    path = a.out or os.path.join(ROOT, "profiles", f"index_rebucket_inplace_{tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"n": n, "out": path, "equal": out["equal"]} | {
        name: {"gather_ms": out[name]["gather_ms"]["median_ms"],
               "relabel_ms": out[name]["relabel_ms"]["median_ms"],
               "relabel_inplace_ms": out[name]["relabel_inplace_ms"]["median_ms"],
               "plan_ms": out[name]["plan_ms"]["median_ms"],
               "swap_ms": [out[name]["swap1_ms"]["median_ms"], out[name]["swap2_ms"]["median_ms"]],
               "swap_GBps": [round(v, 1) for v in out[name]["swap_GBps"]],
               "peak_rise_over_corpus": out[name]["peak_rise_over_corpus"]} for name in sets}))


if __name__ == "__main__":
    main()
