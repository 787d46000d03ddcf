#!/usr/bin/env python3
"""In-place index updates against the copying ones (K9: lmi_index_move_rows_inplace
in csrc/lmi_update.hip), on one GPU:

    python tools/index_inplace_bench.py --n 10000000 --tag 10M --sweep
    python tools/index_inplace_bench.py --n 300000 --tag 300K --sweep

An n x 768 fp16 corpus is generated in HBM (li.synth.torch_mixture) with random
bucket labels and indexed with a capacity of n + batch rows.  In one process,
after a warm-up of each, --reps rounds alternate, on the same index state,

  add_spread   add of --batch rows whose labels spread over all buckets
  add_last10   add of --batch rows whose labels lie in the last 10 buckets
  remove       remove of --batch random ids (drawn anew every round)

each as the copying call and as the in-place call (which is then undone in
place, so every round starts from an index of n rows).  Per case and way:

  move_ms      device events around the row moves (the copying kernel; the
               whole in-place chain)
  call_ms      host clock from the call to its return
  peak_rise    rise of torch.cuda.max_memory_allocated over the call
  slabs, bytes the plan's direct / staged slabs and rows, and the byte model:
               (2 d_pad + 4) bytes per row, read + write = 2 x per moved row,
               4 x per row of a staged slab (it crosses HBM twice)

--sweep adds the in-place move_ms over slab_rows x direct_rows (the table the
defaults come from) and the staged copy by kernel against hipMemcpyAsync.
profiles/index_inplace_<tag>.json receives every time as median [min, max]."""
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
from li.index import DEFAULT_DIRECT_ROWS, DEFAULT_SLAB_ROWS, STAGING_MAX_BYTES, DeviceIndex  # noqa: E402

DEV = "cuda:0"
SWEEP_SLAB = (16 << 10, 64 << 10, 256 << 10)
SWEEP_DIRECT = (1 << 10, 4 << 10, 16 << 10, 64 << 10, 1 << 40)    # (1 << 40: every slab staged)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
            "all": [round(float(x), 4) for x in v]}


def call(fn, **kw):
    """fn(timings=..., **kw) -> (result, record): move_ms, call_ms, peak_rise and the plan."""
    t = {}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    t0 = time.perf_counter()
    out = fn(timings=t, **kw)
    torch.cuda.synchronize()
    t["call_ms"] = (time.perf_counter() - t0) * 1e3
    t["peak_rise"] = torch.cuda.max_memory_allocated(DEV) - base
    return out, t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-reps", type=int, default=3)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("index_inplace_bench needs a HIP device (no CPU path)")
    n, d, m, C = a.n, a.d, a.batch, a.buckets
    x, _ = synth.torch_mixture(n + m, d, 400, a.seed, DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(a.seed + 1)
    labels = torch.randint(0, C, (n + m,), generator=g, device=DEV)
    lab_host = labels.cpu().numpy()
    index = DeviceIndex.empty(d, C, device=DEV, capacity=n + m).add(x[:n], labels[:n], inplace=True)
    assert index.capacity == n + m
    store_ptr = index.corpus.data_ptr()
    new_rows, new_ids = x[n:], np.arange(n + 1, n + m + 1, dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(a.seed))
    mixes = {"add_spread": lab_host[n:], "add_last10": rng.integers(C - 10, C, m).astype(np.int64)}
    d_pad = index.d_pad
    row_b = 2 * d_pad + 4

    def model(t):
        if "staged_rows" not in t:
            return 2 * t["moved_rows"] * row_b
        return (2 * t["moved_rows"] + 2 * t["staged_rows"]) * row_b

    def round_(index, rec, **plan):
        """One round of the three cases, both ways; returns the index (n rows again)."""
        for name, lab in mixes.items():
            _, t = call(lambda **kw: index.add(new_rows, lab, new_ids, **kw))
            rec(name, "copy", t)
            index, t = call(lambda **kw: index.add(new_rows, lab, new_ids, inplace=True, **kw), **plan)
            rec(name, "inplace", t)
            index = index.remove(new_ids, inplace=True)        # (undo; not a measured case)
        gone = rng.choice(n, m, replace=False).astype(np.int64) + 1      # ids 1..n
        _, t = call(lambda **kw: index.remove(gone, **kw))
        rec("remove", "copy", t)
        index, t = call(lambda **kw: index.remove(gone, inplace=True, **kw), **plan)
        rec("remove", "inplace", t)
        index = index.add(x[gone - 1], lab_host[gone - 1], gone, inplace=True)   # (undo)
        assert index.n_rows == n and index.corpus.data_ptr() == store_ptr
        return index

    keys = ("move_ms", "call_ms", "peak_rise", "direct_slabs", "staged_slabs", "moved_rows", "staged_rows",
            "staging_rows", "bytes_model")
    main_rec = {}

    def rec_main(name, way, t):
        t["bytes_model"] = model(t)
        for k in keys:
            if k in t:
                main_rec.setdefault(name, {}).setdefault(way, {}).setdefault(k, []).append(t[k])

    for rep in range(-1, a.reps):                    # round -1: the warm-up
        index = round_(index, rec_main if rep >= 0 else (lambda *_: None))
        print(f"round {rep} done", flush=True)

    out = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "d_pad": d_pad, "buckets": C,
           "batch": m, "reps": a.reps, "capacity": index.capacity, "row_bytes": row_b,
           "corpus_bytes": n * 2 * d_pad,
           "defaults": {"slab_rows": min(DEFAULT_SLAB_ROWS, STAGING_MAX_BYTES // row_b),
                        "direct_rows": DEFAULT_DIRECT_ROWS}, "cases": {}}
    for name, ways in main_rec.items():
        c = out["cases"][name] = {w: {k: stats(v) for k, v in r.items()} for w, r in ways.items()}
        c["inplace_over_copy_move"] = c["inplace"]["move_ms"]["median"] / c["copy"]["move_ms"]["median"]
        c["inplace_over_copy_call"] = c["inplace"]["call_ms"]["median"] / c["copy"]["call_ms"]["median"]
        c["inplace_over_copy_bytes"] = c["inplace"]["bytes_model"]["median"] / c["copy"]["bytes_model"]["median"]

    if a.sweep:
        table = []
        for slab in SWEEP_SLAB:
            for direct in SWEEP_DIRECT:
                got = {}

                def rec(name, way, t, got=got):
                    if way == "inplace":
                        for k in ("move_ms", "direct_slabs", "staged_slabs", "staging_rows"):
                            got.setdefault(name, {}).setdefault(k, []).append(t[k])
                for _ in range(a.sweep_reps):
                    index = round_(index, rec, slab_rows=slab, direct_rows=direct)
                row = {"slab_rows": slab, "direct_rows": direct,
                       "staging_bytes": int(max(max(v["staging_rows"]) for v in got.values())) * row_b,
                       "within_staging_cap": slab * row_b <= STAGING_MAX_BYTES}
                for name, v in got.items():
                    row[name] = {"move_ms": stats(v["move_ms"]), "direct_slabs": int(np.median(v["direct_slabs"])),
                                 "staged_slabs": int(np.median(v["staged_slabs"]))}
                table.append(row)
                print(json.dumps({k: (v["move_ms"]["median"] if isinstance(v, dict) else v)
                                  for k, v in row.items()}), flush=True)
        out["sweep"] = table
        # the staged copy: the copy kernel against hipMemcpyAsync, defaults otherwise, alternating
        how = {"kernel": {}, "memcpy": {}}
        for _ in range(a.sweep_reps + 1):
            for name, env in (("kernel", "0"), ("memcpy", "1")):
                os.environ["LMI_INPLACE_MEMCPY"] = env

                def rec(case, way, t, name=name):
                    if way == "inplace":
                        how[name].setdefault(case, []).append(t["move_ms"])
                index = round_(index, rec)
        os.environ.pop("LMI_INPLACE_MEMCPY")
        out["staged_copy"] = {k: {c: stats(v[1:]) for c, v in r.items()} for k, r in how.items()}   # ([0]: warm-up)

    tag = a.tag or str(n)
    path = a.out or os.path.join(ROOT, "profiles", f"index_inplace_{tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    brief = {"n": n, "out": path}
    for name, c in out["cases"].items():
        brief[name] = {"copy_move_ms": c["copy"]["move_ms"]["median"],
                       "inplace_move_ms": c["inplace"]["move_ms"]["median"],
                       "ratio": round(c["inplace_over_copy_move"], 3),
                       "copy_call_ms": c["copy"]["call_ms"]["median"],
                       "inplace_call_ms": c["inplace"]["call_ms"]["median"],
                       "slabs": [c["inplace"]["direct_slabs"]["median"], c["inplace"]["staged_slabs"]["median"]],
                       "peak_rise": [c["copy"]["peak_rise"]["median"], c["inplace"]["peak_rise"]["median"]]}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
