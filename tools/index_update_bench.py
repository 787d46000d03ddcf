#!/usr/bin/env python3
"""Index updates against a rebuild (K7: csrc/lmi_update.hip), on one GPU:

    python tools/index_update_bench.py --n 10000000 --tag 10M
    python tools/index_update_bench.py --n 300000 --tag 300K

An n x 768 fp16 corpus is generated in HBM (li.synth.torch_mixture) with
random bucket labels and indexed as DeviceIndex.empty().add(all rows).  In one
process, after a warm-up of each, --reps rounds alternate

  (a) index.add of --batch rows: the two kernels alone by device events (the
      C-ABI calls on prepared tables), and a host clock from the call to its
      return (host tables, allocations, uploads, kernels, the status read)
  (b) index.remove of --batch ids, the same two ways
  (c) corpus.clone() of the same corpus: the copy-rate yardstick
  (d) twice only (it takes seconds): DeviceIndex(host rows, host labels), the
      only way to this index without updates

With --tag-edits the index is tagged and the rounds alternate instead

  (e) index.edit_tags of --batch ids (one bit set: a tombstone): a host clock
      from the call to its return, and lmi_index_edit_tags alone by device
      events on prepared tables
  (f) index.remove of the same ids, the host clock of (b): what hiding those
      objects from the next query costs without tag edits

and profiles/index_tag_edit_<tag>.json receives them.  Without it,
profiles/index_update_<tag>.json receives every time with its spread
(max - min), the byte model 2 n (2 d_pad + 4) + batch bytes, the move kernel's
bytes/s, that rate over (c)'s and over profiles/r05l_hbm_peak.txt's copy
rate, the host-table share of (a), and (d) over (a)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import BucketLayout, DeviceIndex  # noqa: E402

DEV = "cuda:0"


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                       # ms


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3      # ms


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
            "spread_ms": float(max(v) - min(v)), "all_ms": [round(float(x), 4) for x in v]}


def kernels(index, drop, rows, labels):
    """The update's kernels alone on prepared tables -> (move ms, ingest ms)."""
    lib = _lib.load()
    t0 = time.perf_counter()
    layout, new_dst, surv_off, drop_before = index.layout.updated(drop, labels)
    n_new = int(layout.bucket_off[-1])
    p2id = np.empty(n_new, np.int64)
    BucketLayout.place_survivors(np.delete(index.pos_to_id, drop) if drop.size else index.pos_to_id,
                                 surv_off, layout.bucket_off, p2id)
    host_ms = (time.perf_counter() - t0) * 1e3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    new_off, d_drop, d_before, d_dst = up(layout.bucket_off), up(drop), up(drop_before), up(new_dst)
    corpus = torch.empty((n_new, index.d_pad), dtype=torch.float16, device=DEV)
    inv = torch.empty((n_new,), dtype=torch.float32, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    s = _lib.stream_handle(DEV)
    r, m = int(drop.size), int(labels.size)
    move = events(lambda: _lib.check("lmi_index_move_rows", lib.lmi_index_move_rows(
        index.corpus.data_ptr(), index.inv_norm.data_ptr(), index.n_rows, index.d_pad,
        index.bucket_off_local.data_ptr(), new_off.data_ptr(), index.n_buckets,
        d_drop.data_ptr() if r else None, r, d_before.data_ptr() if r else None,
        corpus.data_ptr(), inv.data_ptr(), n_new, status.data_ptr(), s)))
    ingest = 0.0
    if m:
        ingest = events(lambda: _lib.check("lmi_index_ingest_rows", lib.lmi_index_ingest_rows(
            rows.data_ptr(), _lib.LMI_F16, m, rows.stride(0), index.d, index.d_pad, d_dst.data_ptr(),
            corpus.data_ptr(), inv.data_ptr(), n_new, status.data_ptr(), s)))
    assert int(status.item()) == 0
    return move, ingest, host_ms


def tag_edits(a):
    """(e), (f): edit_tags against remove on one tagged index."""
    n, d, m, C = a.n, a.d, a.batch, a.buckets
    x, _ = synth.torch_mixture(n, d, 400, a.seed, DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(a.seed + 1)
    labels = torch.randint(0, C, (n,), generator=g, device=DEV)
    tags = torch.randint(0, 64, (n,), generator=g, device=DEV).cpu().numpy().astype(np.uint32)
    index = DeviceIndex.empty(d, C, device=DEV, tags=True).add(x, labels, tags=tags)
    del x
    rng = np.random.Generator(np.random.PCG64(a.seed))
    ids = rng.choice(n, m, replace=False).astype(np.int64) + 1           # ids 1..n
    rows = torch.from_numpy(np.flatnonzero(np.isin(index.pos_to_id, ids)).astype(np.int64)).to(DEV)
    bit = torch.full((m,), 1 << 29, dtype=torch.int32, device=DEV)
    zero = torch.zeros((m,), dtype=torch.int32, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    lib, s = _lib.load(), _lib.stream_handle(DEV)
    t = {k: [] for k in ("edit_tags_ms", "edit_kernel_ms", "remove_ms")}
    for rep in range(-1, a.reps):                    # round -1: the warm-up
        got = {}
        _, got["edit_tags_ms"] = wall(lambda: index.edit_tags(ids, set_bits=1 << 29))
        got["edit_kernel_ms"] = events(lambda: _lib.check("lmi_index_edit_tags", lib.lmi_index_edit_tags(
            index.tags.data_ptr(), index.n_rows, rows.data_ptr(), bit.data_ptr(), zero.data_ptr(), m,
            status.data_ptr(), s)))                  # (clears the bit again)
        _, got["remove_ms"] = wall(lambda: index.remove(ids))
        if rep >= 0:
            for k, v in got.items():
                t[k].append(v)
    assert int(status.item()) == 0
    index.edit_tags(ids, set_bits=1 << 29)
    marked = bool(np.array_equal(np.sort(index.ids_with(want=1 << 29)), np.sort(ids))
                  and int((index.tags & (1 << 29) != 0).sum().item()) == m)
    out = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "buckets": C, "batch": m, "reps": a.reps,
           "timing": "edit_tags_ms, remove_ms: host clock from the call to its return, the device idle before "
                     "and after; edit_kernel_ms: device events around lmi_index_edit_tags on prepared tables",
           "marked_ids_equal_ids_with": marked}
    for k, v in t.items():
        out[k] = stats(v)
    out["remove_over_edit_tags"] = out["remove_ms"]["median_ms"] / out["edit_tags_ms"]["median_ms"]
    path = a.out or os.path.join(ROOT, "profiles", f"index_tag_edit_{a.tag or n}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k]["median_ms"] for k in t} | {"remove_over_edit_tags": out["remove_over_edit_tags"],
                                                             "marked": marked, "out": path}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rebuilds", type=int, default=2)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag-edits", action="store_true", help="(e), (f): edit_tags against remove")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("index_update_bench needs a HIP device (no CPU path)")
    if a.tag_edits:
        return tag_edits(a)
    n, d, m, C = a.n, a.d, a.batch, a.buckets
    x, _ = synth.torch_mixture(n + m, d, 400, a.seed, DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(a.seed + 1)
    labels = torch.randint(0, C, (n + m,), generator=g, device=DEV)
    lab_host = labels.cpu().numpy()
    (index, build_ms) = wall(lambda: DeviceIndex.empty(d, C, device=DEV).add(x[:n], labels[:n]))
    new_rows, new_lab = x[n:], lab_host[n:]
    rng = np.random.Generator(np.random.PCG64(a.seed))
    gone = rng.choice(n, m, replace=False).astype(np.int64) + 1          # ids 1..n
    drop = np.flatnonzero(np.isin(index.pos_to_id, gone))
    none = np.zeros(0, np.int64)
    d_pad = index.d_pad
    row_b = 2 * d_pad + 4
    t = {k: [] for k in ("add_ms", "add_move_ms", "add_ingest_ms", "add_host_tables_ms", "remove_ms",
                         "remove_move_ms", "remove_host_tables_ms", "clone_ms")}
    for rep in range(-1, a.reps):                    # round -1: the warm-up
        got = {}
        _, got["add_ms"] = wall(lambda: index.add(new_rows, new_lab))
        got["add_move_ms"], got["add_ingest_ms"], got["add_host_tables_ms"] = kernels(
            index, none, new_rows, new_lab)
        _, got["remove_ms"] = wall(lambda: index.remove(gone))
        got["remove_move_ms"], _, got["remove_host_tables_ms"] = kernels(index, drop, None, none)
        got["clone_ms"] = events(lambda: index.corpus.clone())
        if rep >= 0:
            for k, v in got.items():
                t[k].append(v)
    # (d) the rebuild from host arrays: the host copy is made outside the timer
    x_host = x[:n].cpu()
    rebuild = []
    for _ in range(a.rebuilds):
        ref, ms = wall(lambda: DeviceIndex(x_host, lab_host[:n], C, device=DEV))
        rebuild.append(ms)
    same = bool(torch.equal(ref.corpus, index.corpus) and torch.equal(ref.inv_norm, index.inv_norm)
                and np.array_equal(ref.pos_to_id, index.pos_to_id))
    del ref, x_host

    out = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "d_pad": d_pad, "buckets": C,
           "batch": m, "reps": a.reps, "chunk_rows": index.chunk_rows,
           "build_as_empty_add_ms": build_ms, "rebuild_equals_empty_add": same}
    for k, v in t.items():
        out[k] = stats(v)
    out["rebuild_from_host_ms"] = stats(rebuild)
    move_bytes = 2 * n * row_b
    out["bytes_model"] = {"add": move_bytes + m * (2 * d + row_b), "add_move": move_bytes,
                          "remove_move": move_bytes - m * row_b - m * row_b,
                          "clone": 2 * n * 2 * d_pad}
    rate = lambda b, ms: b / (ms * 1e-3) / 1e9       # GB/s
    out["add_move_GBps"] = rate(out["bytes_model"]["add_move"], out["add_move_ms"]["median_ms"])
    out["remove_move_GBps"] = rate(out["bytes_model"]["remove_move"], out["remove_move_ms"]["median_ms"])
    out["clone_GBps"] = rate(out["bytes_model"]["clone"], out["clone_ms"]["median_ms"])
    out["add_move_over_clone"] = out["add_move_GBps"] / out["clone_GBps"]
    out["remove_move_over_clone"] = out["remove_move_GBps"] / out["clone_GBps"]
    peak = os.path.join(ROOT, "profiles", "r05l_hbm_peak.txt")
    if os.path.exists(peak):
        runs = [json.loads(l) for l in open(peak) if l.startswith("{")]
        out["hbm_copy_peak_GBps"] = max(r_["hip_copy_GBps"] for r_ in runs)
        out["add_move_over_hbm_copy_peak"] = out["add_move_GBps"] / out["hbm_copy_peak_GBps"]
    out["add_host_table_share"] = out["add_host_tables_ms"]["median_ms"] / out["add_ms"]["median_ms"]
    out["add_kernel_share"] = (out["add_move_ms"]["median_ms"] + out["add_ingest_ms"]["median_ms"]) \
        / out["add_ms"]["median_ms"]
    out["rebuild_over_add"] = out["rebuild_from_host_ms"]["median_ms"] / out["add_ms"]["median_ms"]
    tag = a.tag or str(n)
    path = a.out or os.path.join(ROOT, "profiles", f"index_update_{tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("n", "add_move_GBps", "remove_move_GBps", "clone_GBps",
                                          "add_move_over_clone", "add_host_table_share",
                                          "rebuild_over_add")}
                     | {"add_ms": out["add_ms"]["median_ms"], "remove_ms": out["remove_ms"]["median_ms"],
                        "rebuild_ms": out["rebuild_from_host_ms"]["median_ms"], "out": path}))


if __name__ == "__main__":
    main()
