#!/usr/bin/env python3
"""Index re-bucket against a rebuild (K8: csrc/lmi_rebucket.hip), on one GPU:

    python tools/index_rebucket_bench.py --n 10000000 --tag 10M
    python tools/index_rebucket_bench.py --n 300000 --tag 300K

An n x 768 fp16 corpus is generated in HBM (li.synth.torch_mixture), labelled
by a router fitted on a k-means of its navigation vectors and indexed as
DeviceIndex.empty().add(all rows).  Two new label sets are measured:

  recluster  the labels of a re-cluster: a new k-means (another seed) and a
             router fitted on it, over the same rows
  random     uniformly random labels (no source locality at all)

In one process, after a warm-up of each, --reps rounds alternate, per label set

  (a) the sort: lmi_bucket_sort_labels (its four launches, device events),
      torch.sort(stable=True) on the device, and (--host-sorts times: it takes
      a second at 10M) np.argsort(kind="stable") on the host
  (b) the gather kernel (device events; bytes/s under the 2 n (2 d_pad + 4)
      byte model) beside the K7 move kernel over the same corpus,
      corpus.clone(), and corpus.index_select(0, src) + inv_norm.index_select
  (c) index.relabel from the call to its return (host clock), and once more
      with its stage clock on: the sort, the device tables (with the uploads
      of the old order / pos_to_id), the gather, the host tables (with the
      downloads)
  (d) --rebuilds times (it takes seconds): DeviceIndex(host rows, labels)

and profiles/index_rebucket_<tag>.json receives every time as median [min,
max], the rates, the ratios and whether the relabelled index equals (d)'s."""
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
from li.index import DeviceIndex, DeviceRouter  # noqa: E402

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


def router_labels(xn, n_buckets, seed):
    """Labels of a clustering: k-means on a 100K subsample of the navigation
    vectors, a short router fit on it (CPU: reproducible), the router's argmax
    over every row (li.synth.build_lmi_workload's steps)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sub = xn[torch.randperm(xn.shape[0], generator=g)[: min(xn.shape[0], 100_000)].to(xn.device)].cpu()
    with torch.random.fork_rng(devices=[]):
        cent = synth.kmeans(sub, n_buckets, iters=20, seed=seed)
        d2 = (sub * sub).sum(1, keepdim=True) - 2 * sub @ cent.T + (cent * cent).sum(1)[None]
        model = synth.train_router(sub, d2.argmin(1), synth.ARCHS["MLP"], n_buckets, steps=200,
                                   batch=2048, seed=seed)
    layers = [(m.weight.detach().cpu(), m.bias.detach().cpu()) for m in model
              if isinstance(m, torch.nn.Linear)]
    return DeviceRouter(layers, device=DEV).argmax(xn).to(torch.int64)


def sort_call(lab, n_buckets, order, off, status, ws):
    lib = _lib.load()
    _lib.check("lmi_bucket_sort_labels", lib.lmi_bucket_sort_labels(
        lab.data_ptr(), lab.element_size(), lab.numel(), n_buckets, off.data_ptr(), order.data_ptr(),
        status.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream_handle(DEV)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-sorts", type=int, default=3)
    ap.add_argument("--rebuilds", type=int, default=2)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("index_rebucket_bench needs a HIP device (no CPU path)")
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
    d_pad = index.d_pad
    row_b = 2 * d_pad + 4
    s = _lib.stream_handle(DEV)
    out = {"device": torch.cuda.get_device_name(0), "n": n, "d": d, "d_pad": d_pad, "buckets": C,
           "reps": a.reps, "chunk_rows": index.chunk_rows,
           "bytes_model": {"gather": 2 * n * row_b, "move": 2 * n * row_b, "clone": 2 * n * 2 * d_pad,
                           "index_select": 2 * n * row_b + 8 * n},
           "labels_moved_fraction": {k: float((v != lab_old).float().mean().item()) for k, v in sets.items()}}
    rate = lambda b, ms: b / (ms * 1e-3) / 1e9       # GB/s
    old_order = torch.from_numpy(index.layout.order).to(DEV)
    inv = torch.empty(n, dtype=torch.int64, device=DEV)
    inv[old_order] = torch.arange(n, dtype=torch.int64, device=DEV)
    del old_order
    order = torch.empty(n, dtype=torch.int64, device=DEV)
    off = torch.empty(C + 1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(lib.lmi_bucket_sort_labels_ws_bytes(n, C), 8) // 8, dtype=torch.int64, device=DEV)
    corpus = torch.empty((n, d_pad), dtype=torch.float16, device=DEV)
    inv_norm = torch.empty((n,), dtype=torch.float32, device=DEV)
    for name, lab in sets.items():
        t = {k: [] for k in ("sort_ms", "torch_sort_ms", "gather_ms", "move_ms", "clone_ms",
                             "index_select_ms", "relabel_ms")}
        sort_call(lab, C, order, off, status, ws)
        src_pos = inv[order]
        for rep in range(-1, a.reps):                # round -1: the warm-up
            got = {}
            got["sort_ms"] = events(lambda: sort_call(lab, C, order, off, status, ws))
            got["torch_sort_ms"] = events(lambda: torch.sort(lab, stable=True))
            got["gather_ms"] = events(lambda: _lib.check("lmi_index_gather_rows", lib.lmi_index_gather_rows(
                index.corpus.data_ptr(), index.inv_norm.data_ptr(), n, d_pad, src_pos.data_ptr(),
                corpus.data_ptr(), inv_norm.data_ptr(), n, status.data_ptr(), s)))
            # the K7 move kernel over the same corpus: every row to where it is (no drops)
            got["move_ms"] = events(lambda: _lib.check("lmi_index_move_rows", lib.lmi_index_move_rows(
                index.corpus.data_ptr(), index.inv_norm.data_ptr(), n, d_pad,
                index.bucket_off_local.data_ptr(), index.bucket_off_local.data_ptr(), C, None, 0, None,
                corpus.data_ptr(), inv_norm.data_ptr(), n, status.data_ptr(), s)))
            got["clone_ms"] = events(lambda: index.corpus.clone())
            got["index_select_ms"] = events(lambda: (index.corpus.index_select(0, src_pos),
                                                     index.inv_norm.index_select(0, src_pos)))
            new, got["relabel_ms"] = wall(lambda: index.relabel(lab))
            del new
            if rep >= 0:
                for k, v in got.items():
                    t[k].append(v)
        assert int(status.item()) == 0
        parts = {}
        new = index.relabel(lab, timings=parts)
        lab_host = lab.cpu().numpy()
        host_sort = []
        for _ in range(a.host_sorts):
            t0 = time.perf_counter()
            want_order = np.argsort(lab_host, kind="stable")
            host_sort.append((time.perf_counter() - t0) * 1e3)
        r = {k: stats(v) for k, v in t.items()}
        r["np_argsort_ms"] = stats(host_sort)
        r["sort_equals_np_argsort"] = bool(np.array_equal(order.cpu().numpy(), want_order))
        r["relabel_stage_ms"] = {k: v * 1e3 for k, v in parts.items()}
        med = lambda k: r[k]["median_ms"]
        r["gather_GBps"] = rate(out["bytes_model"]["gather"], med("gather_ms"))
        r["move_GBps"] = rate(out["bytes_model"]["move"], med("move_ms"))
        r["clone_GBps"] = rate(out["bytes_model"]["clone"], med("clone_ms"))
        r["index_select_GBps"] = rate(out["bytes_model"]["index_select"], med("index_select_ms"))
        r["gather_over_move"] = r["gather_GBps"] / r["move_GBps"]
        r["gather_over_clone"] = r["gather_GBps"] / r["clone_GBps"]
        r["index_select_ms_over_gather_ms"] = med("index_select_ms") / med("gather_ms")
        r["torch_sort_over_sort"] = med("torch_sort_ms") / med("sort_ms")
        r["np_argsort_over_sort"] = med("np_argsort_ms") / med("sort_ms")
        total = sum(parts.values())
        r["relabel_host_share"] = (parts["host"] + parts["tables"]) / total
        r["relabel_kernel_share"] = (med("sort_ms") + med("gather_ms")) / med("relabel_ms")
        if name == "recluster":
            # (d) the rebuild from host arrays: the host copy is made outside the timer
            x_host = x.cpu()
            rebuild = []
            for _ in range(a.rebuilds):
                ref, ms = wall(lambda: DeviceIndex(x_host, lab_host, C, device=DEV))
                rebuild.append(ms)
            r["relabel_equals_rebuild"] = bool(
                torch.equal(ref.corpus, new.corpus) and torch.equal(ref.inv_norm, new.inv_norm)
                and np.array_equal(ref.pos_to_id, new.pos_to_id)
                and np.array_equal(ref.layout.order, new.layout.order)
                and torch.equal(ref.chunk_first, new.chunk_first))
            del ref, x_host
            out["rebuild_from_host_ms"] = stats(rebuild)
        r["rebuild_over_relabel"] = out["rebuild_from_host_ms"]["median_ms"] / med("relabel_ms")
        del new, src_pos
        out[name] = r
    tag = a.tag or str(n)
    path = a.out or os.path.join(ROOT, "profiles", f"index_rebucket_{tag}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"n": n, "out": path, "rebuild_ms": out["rebuild_from_host_ms"]["median_ms"]} | {
        name: {k: round(out[name][k], 3) for k in ("gather_GBps", "move_GBps", "clone_GBps",
                                                   "index_select_GBps", "gather_over_move",
                                                   "torch_sort_over_sort", "np_argsort_over_sort",
                                                   "relabel_host_share", "rebuild_over_relabel")}
        | {"sort_ms": out[name]["sort_ms"]["median_ms"], "relabel_ms": out[name]["relabel_ms"]["median_ms"]}
        for name in sets}))


if __name__ == "__main__":
    main()
