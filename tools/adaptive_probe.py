#!/usr/bin/env python3
"""Adaptive probing measured: the router's probability-mass stop rule
(Searcher.search(stop_mass=...), lmi_router_stop) against fixed probe counts,
at equal recall, on a TRAINED router (the random routers of the test workloads
are near uniform: top-1 probability about 1/C).

    python tools/adaptive_probe.py --n 300000 --cap 7 --out profiles/adaptive_probe_300K.json
    python tools/adaptive_probe.py --n 10000000 --cap 4 --out profiles/adaptive_probe_10M.json

The corpus and the queries are the bench's synthetic mixture (li.synth); the
index is built by LearnedIndex.build(train_mode='minibatch') on the pca96 rows;
recall@10 is against the exact brute force over the whole corpus (the corpus as
one bucket of the scan, li.Baseline's form).

Settings: fixed R = 1 .. cap, and R = cap with every --stop-mass.  Each gets
  mean_probes  probes per query (the router's kept classes)
  recall_at_10
  scan_ms      the scan kernels' time per eager step (HIP events of
               lmi_timing_enable, summed per step, mean over --steps steps)
  stream_ms    ms per launch of the batch stream (Searcher.streamed), wall clock
               over --steps launches after a warm-up
  stream_scan_ms  the scan graph alone inside those launches (HIP events)
measured --reps times, the settings alternating inside every repetition (the
repetitions are the spread: median and max - min are reported).  For each stop
mass `equal_recall` names the cheapest fixed R (by stream_ms median) whose
recall is at least as high, and the time ratios against it; "not measured"
where a figure could not be taken."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import math  # noqa: E402

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from li import _lib, synth  # noqa: E402
from li.index import DeviceIndex, Searcher, default_chunk_rows  # noqa: E402
from li.LearnedIndex import LearnedIndex  # noqa: E402

NM = "not measured"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def workload(a, dev):
    x, cen = synth.torch_mixture(a.n, 768, a.centres, seed=a.seed, device=dev)
    q, _ = synth.torch_mixture(a.nq, 768, a.centres, seed=a.seed + 2219, device=dev, centres=cen,
                               out_dtype=torch.float32)
    g = torch.Generator(device="cpu")
    g.manual_seed(96)
    P = (torch.randn((768, 96), generator=g) / math.sqrt(768)).to(dev)
    return x, q, synth.torch_nav(x, P), synth.torch_nav(q, P)


def brute_force(x, q, k, dev):
    ix = DeviceIndex(x, torch.zeros(x.shape[0], dtype=torch.int32, device=dev), 1, device=dev)
    cls = torch.zeros((q.shape[0], 1), dtype=torch.int32, device=dev)
    _, d, pos, st = Searcher(ix, None, exchange=False).lists(None, q, 1, k, classes=cls)
    assert not int(st.item()) & _lib.LMI_STATUS_INTERNAL
    return ix.pos_to_id[np.maximum(pos[:, 0].cpu().numpy(), 0)]


def recall(anns, truth):
    k = truth.shape[1]
    hit = [np.intersect1d(anns[i][anns[i] > 0], truth[i]).size for i in range(truth.shape[0])]
    return float(np.sum(hit)) / (k * truth.shape[0])


def summary(v):
    v = [x for x in v if x is not None]
    if not v:
        return dict(median=NM, spread=NM)
    return dict(median=round(float(np.median(v)), 4), spread=round(float(max(v) - min(v)), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=300_000)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--buckets", type=int, default=122)
    ap.add_argument("--cap", type=int, default=7)
    ap.add_argument("--arch", default="MLP-5")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=0.009)
    ap.add_argument("--centres", type=int, default=400)
    ap.add_argument("--stop-mass", type=float, nargs="+", default=[0.5, 0.8, 0.9, 0.95, 0.99])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--extra", default=None, help="a JSON file merged into the result under 'extra'")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    K = 10
    t0 = time.time()
    x, q, xn, qn = workload(a, dev)
    truth = brute_force(x, q, K, dev)
    torch.cuda.empty_cache()
    log(f"[adaptive] workload and brute force in {time.time() - t0:.1f} s")
    data = pd.DataFrame(xn.cpu().numpy())
    data.index += 1
    del xn
    torch.manual_seed(a.seed)
    li = LearnedIndex()
    labels, build_s = li.build(data, n_categories=a.buckets, epochs=a.epochs, lr=a.lr,
                               model_type=a.arch, train_mode="minibatch")
    del data
    router = li.model.router()
    ix = DeviceIndex(x, np.asarray(labels), a.buckets, device=dev,
                     chunk_rows=default_chunk_rows(1, a.n))
    s = Searcher(ix, router, exchange=False)
    _, p = router.topr(qn, a.cap, with_probs=True)
    p = p.cpu().numpy()
    log(f"[adaptive] built in {build_s:.1f} s; mean top-1 probability {p[:, 0].mean():.3f}, "
        f"mean mass of the top {a.cap}: {p.sum(1).mean():.3f}")
    qn_h, q_h = qn.cpu().numpy(), q.cpu().numpy()

    settings = [dict(kind="fixed", R=r, stop_mass=None) for r in range(1, a.cap + 1)]
    settings += [dict(kind="stop", R=a.cap, stop_mass=m) for m in a.stop_mass]
    for st in settings:
        rule = {} if st["stop_mass"] is None else dict(stop_mass=st["stop_mass"])
        st["rule"] = rule
        cls = s.route(qn, st["R"], **rule)
        st["mean_probes"] = round(float((cls >= 0).sum().item()) / a.nq, 4)
        d, ann = s.search(qn, q, st["R"], k=K, **rule)
        st["recall_at_10"] = round(recall(ann, truth), 5)
        st["scan"], st["stream"], st["stream_scan"] = [], [], []
        log(f"[adaptive] {st['kind']} R={st['R']} stop={st['stop_mass']}: "
            f"{st['mean_probes']} probes, recall {st['recall_at_10']}")

    def scan_ms(st):
        for _ in range(2):
            s.search(qn, q, st["R"], k=K, **st["rule"])
        torch.cuda.synchronize()
        lib.lmi_timing_read(None, 0)
        lib.lmi_timing_enable(1)
        for _ in range(a.steps):
            s.search(qn, q, st["R"], k=K, **st["rule"])
        torch.cuda.synchronize()
        lib.lmi_timing_enable(0)
        cap = 8 * a.steps
        ms = (_lib.C.c_float * cap)()
        n_ev = lib.lmi_timing_read(ms, cap)
        return float(np.sum(list(ms)[:n_ev])) / a.steps if n_ev > 0 else None

    def stream_ms(st):
        with s.streamed(qn_h, q_h, st["R"], k=K, **st["rule"]) as ss:
            for _ in range(a.warmup):
                ss.step()
            ss.time_scans = True
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                ss.step()
            torch.cuda.synchronize()
            el = (time.perf_counter() - t) * 1e3 / a.steps
            scans = ss.scan_ms()
        return el, (float(np.mean(scans)) if scans else None)

    for rep in range(a.reps):
        for st in settings:
            st["scan"].append(scan_ms(st))
            try:
                el, sc = stream_ms(st)
            except Exception as e:  # noqa: BLE001 (recorded)
                log(f"[adaptive] stream failed for {st['kind']} R={st['R']}: {e!r}")
                st["stream_error"] = repr(e)[:200]
                el, sc = None, None
            st["stream"].append(el)
            st["stream_scan"].append(sc)
        log(f"[adaptive] repetition {rep + 1}/{a.reps} done")

    rows = []
    for st in settings:
        row = {k: st[k] for k in ("kind", "R", "stop_mass", "mean_probes", "recall_at_10")}
        for key in ("scan", "stream", "stream_scan"):
            row[f"{key}_ms"] = [NM if v is None else round(v, 4) for v in st[key]]
            sm = summary(st[key])
            row[f"{key}_ms_median"], row[f"{key}_ms_spread"] = sm["median"], sm["spread"]
        if "stream_error" in st:
            row["stream_error"] = st["stream_error"]
        rows.append(row)
    fixed = [r for r in rows if r["kind"] == "fixed"]

    def ratio(x, y):
        return round(x / y, 4) if isinstance(x, float) and isinstance(y, float) and y > 0 else NM

    equal = []
    for r in (r for r in rows if r["kind"] == "stop"):
        ok = [f for f in fixed if f["recall_at_10"] >= r["recall_at_10"]
              and isinstance(f["stream_ms_median"], float)]
        if not ok:
            equal.append(dict(stop_mass=r["stop_mass"], recall_at_10=r["recall_at_10"],
                              mean_probes=r["mean_probes"], cheapest_fixed_R=NM))
            continue
        f = min(ok, key=lambda f: f["stream_ms_median"])
        equal.append(dict(stop_mass=r["stop_mass"], recall_at_10=r["recall_at_10"],
                          mean_probes=r["mean_probes"], cheapest_fixed_R=f["R"],
                          fixed_recall_at_10=f["recall_at_10"],
                          stream_ms=r["stream_ms_median"], fixed_stream_ms=f["stream_ms_median"],
                          stream_ratio=ratio(r["stream_ms_median"], f["stream_ms_median"]),
                          scan_ms=r["scan_ms_median"], fixed_scan_ms=f["scan_ms_median"],
                          scan_ratio=ratio(r["scan_ms_median"], f["scan_ms_median"]),
                          spreads_ms=dict(stream=r["stream_ms_spread"],
                                          fixed_stream=f["stream_ms_spread"])))
    out = dict(n=a.n, nq=a.nq, buckets=a.buckets, cap=a.cap, arch=a.arch, epochs=a.epochs, k=K,
               device=torch.cuda.get_device_name(0), build_seconds=round(build_s, 2),
               train_mode="minibatch", reps=a.reps, steps=a.steps, warmup=a.warmup,
               mean_top1_probability=round(float(p[:, 0].mean()), 4),
               mean_mass_of_cap=round(float(p.sum(1).mean()), 4),
               bucket_rows_min_median_max=[int(ix.bucket_size.min()), int(np.median(ix.bucket_size)),
                                           int(ix.bucket_size.max())],
               settings=rows, equal_recall=equal)
    if a.extra:
        with open(a.extra) as f:
            out["extra"] = json.load(f)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "settings"}))


if __name__ == "__main__":
    main()
