#!/usr/bin/env python3
"""Timing of the index build (LearnedIndex.build, LearnedIndex.py:197-240) on
synthetic blobs, phase by phase, one JSON line:

    python tools/build_bench.py --n 300000 --d 96 --k 122 --epochs 20 --arch MLP \
        --verbatim-epochs 1

  cluster   LearnedIndex.cluster: k-means training (K5, 25 iterations on the
            k*256-row sample) and the labelling of every row
  train     what build does between the labels and the trained router: the
            LIDataset, the DataLoader over a SubsetRandomSampler of the frame's
            ids, the NeuralNetwork and train_batch (each epoch's last minibatch)
            (`train_batch`: that call alone)
  predict   NeuralNetwork.predict of every row (K1, argmax)
  total     their sum

--verbatim-epochs E also runs E epochs of the reference's loop
(LMI_TRAIN_VERBATIM=1) on the same loader with a fresh network and reports
`verbatim_epoch`, the seconds per epoch; the tool then fails (exit status 1)
unless the whole `train` phase took less time than one verbatim epoch.

--label-only times the labelling alone, `kmeans.index.search(X, 1)`
(LearnedIndex.py:282) with k random rows as centroids, on rows generated in
HBM (10M x 768 x fp32 is 30.7 GB; the host copy of X is not part of it):
`label` seconds for the call (kernel + the labels and distances to the host)
and `assign_ms`, the kernel by HIP events.

--train-mode minibatch times the training mode that steps on every minibatch
(NeuralNetwork.train_minibatch's kernels, lmi_mlp_train_steps) over one epoch
of the k-means labels, by HIP events around the enqueued epoch, beside a plain
torch loop that takes the same steps on the same device-resident rows (index
gather, forward, CrossEntropyLoss, backward, Adam.step): --reps repetitions of
each, alternating, every one from the same initial weights and the same order,
after a warm-up of both.  `fused_step_us` / `torch_step_us` hold each
repetition's time per step, `*_median` and `*_spread` (max - min) summarise
them; the tool fails (exit status 1) unless the fused median is below the torch
median by more than the two spreads combined.

A tiny Linear step and a tiny k-means run first, outside the timers, so that
no phase carries the process's first kernel launch and BLAS start-up."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from li import kmeans as K  # noqa: E402
from li.LearnedIndex import LearnedIndex  # noqa: E402
from li.model import LIDataset, NeuralNetwork, data_X_to_torch  # noqa: E402


def blobs_device(n, d, c, seed, spread=0.15, chunk=1 << 20):
    """[n, d] fp32 in HBM: c Gaussian centres, rows centre + spread * N(0, 1)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    centres = torch.randn(c, d, device="cuda", generator=g)
    x = torch.empty(n, d, device="cuda")
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        lab = torch.randint(0, c, (b - a,), device="cuda", generator=g)
        x[a:b] = centres[lab] + spread * torch.randn(b - a, d, device="cuda", generator=g)
    return x


def timed(fn, what=None):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter() - t
    if what:
        print(f"{what}: {t:.3f} s", file=sys.stderr, flush=True)
    return out, t


def warm_up(d, k):
    nn = NeuralNetwork(input_dim=d, output_dim=k, lr=0.01, model_type="MLP")
    x = torch.randn(512, d)
    nn.train_batch([(x, torch.randint(0, k, (512,)))], epochs=2)
    nn.predict(x)
    km = K.Kmeans(d, 2, niter=2)
    km.train(x.numpy())
    km.index.search(x.numpy(), 1)


def minibatch(a, x_dev, out):
    """One epoch of minibatch training: the fused kernels against torch eager."""
    import ctypes as C

    from li import _lib
    batch = 256
    x_host = x_dev.cpu().numpy()
    (_, labels), out["cluster"] = timed(lambda: LearnedIndex().cluster(x_host, a.k), "cluster")
    y64 = torch.from_numpy(np.asarray(labels).astype(np.int64)).cuda()
    y32 = y64.to(torch.int32)
    order = torch.randperm(a.n, generator=torch.Generator().manual_seed(a.seed)).cuda()
    steps = -(-a.n // batch)
    first = NeuralNetwork(input_dim=a.d, output_dim=a.k, lr=a.lr, model_type=a.arch)
    init = {k: v.clone() for k, v in first.model.state_dict().items()}
    lib = _lib.load()

    def fresh():
        nn = NeuralNetwork(input_dim=a.d, output_dim=a.k, lr=a.lr, model_type=a.arch)
        nn.model.load_state_dict(init)
        return nn

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3          # us

    def fused(n_steps):
        nn = fresh()
        desc, t0 = nn._minibatch_desc(nn._minibatch_linears())
        need = lib.lmi_mlp_train_workspace_bytes(C.byref(desc), batch)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        loss = torch.empty(n_steps, device="cuda")
        us = events(lambda: _lib.check("lmi_mlp_train_steps", lib.lmi_mlp_train_steps(
            C.byref(desc), x_dev.data_ptr(), a.n, x_dev.stride(0), y32.data_ptr(), order.data_ptr(),
            a.n, batch, 0, n_steps, t0, a.lr, 0.9, 0.999, 1e-8, loss.data_ptr(), ws.data_ptr(), need,
            _lib.stream_handle("cuda"))))
        nn._router = None
        return us / n_steps, nn, float(loss.double().mean())

    def eager(n_steps):
        nn = fresh()
        model, opt, lossf = nn.model, nn.optimizer, nn.loss
        last = [None]

        def loop():
            for s in range(n_steps):
                idx = order[s * batch:(s + 1) * batch]
                loss = lossf(model(x_dev[idx]), y64[idx])
                model.zero_grad()
                loss.backward()
                opt.step()
            last[0] = loss
        us = events(loop)
        return us / n_steps, nn, float(last[0].detach())

    warm = min(steps, 50)
    fused(warm), eager(warm)
    f_us, t_us = [], []
    for _ in range(a.reps):
        us, f_nn, f_loss = fused(steps)
        f_us.append(us)
        us, t_nn, t_loss = eager(steps)
        t_us.append(us)
    X = x_dev
    out.update(train_mode="minibatch", arch=a.arch, batch=batch, steps_per_epoch=steps, reps=a.reps,
               fused_step_us=f_us, torch_step_us=t_us,
               fused_step_us_median=float(np.median(f_us)), fused_step_us_spread=max(f_us) - min(f_us),
               torch_step_us_median=float(np.median(t_us)), torch_step_us_spread=max(t_us) - min(t_us),
               fused_epoch_mean_loss=f_loss, torch_last_step_loss=t_loss,
               fused_label_agreement=float((f_nn.predict(X) == labels).mean()),
               torch_label_agreement=float((t_nn.predict(X) == labels).mean()))
    out["speedup"] = out["torch_step_us_median"] / out["fused_step_us_median"]
    for key in ("fused_step_us", "torch_step_us"):
        out[key] = [round(v, 3) for v in out[key]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=300_000)
    ap.add_argument("--d", type=int, default=96)
    ap.add_argument("--k", type=int, default=122)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--arch", default="MLP")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--verbatim-epochs", type=int, default=0)
    ap.add_argument("--label-only", action="store_true")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--train-mode", default="reference", choices=["reference", "minibatch"])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    os.environ.pop("LMI_TRAIN_VERBATIM", None)
    torch.manual_seed(a.seed)
    out = {"n": a.n, "d": a.d, "k": a.k, "device": torch.cuda.get_device_name(0)}
    warm_up(a.d, a.k)
    x_dev = blobs_device(a.n, a.d, a.k, a.seed)

    if a.label_only:
        pick = torch.from_numpy(np.random.RandomState(a.seed).permutation(a.n)[: a.k]).cuda()
        index = K._FlatL2(x_dev[pick].contiguous())
        index.search(x_dev[: 1 << 16], 1)
        (_, labels), out["label"] = timed(lambda: index.search(x_dev, 1), "label")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.assign(x_dev, index.cent)
        e1.record()
        torch.cuda.synchronize()
        out["assign_ms"] = e0.elapsed_time(e1)
        out["assign_valu_Tops"] = 3.0 * a.n * a.k * a.d / out["assign_ms"] / 1e9
        out["buckets_used"] = int(np.unique(labels).size)
    elif a.train_mode == "minibatch":
        minibatch(a, x_dev, out)
    else:
        out.update(epochs=a.epochs, arch=a.arch)
        data = pd.DataFrame(x_dev.cpu().numpy())
        data.index += 1                                        # search.py:71-72
        del x_dev
        li = LearnedIndex()
        (_, labels), out["cluster"] = timed(lambda: li.cluster(data, a.k), "cluster")
        made = {}

        def train():                                           # LearnedIndex.py:223-237
            dataset = LIDataset(data, labels)
            made["loader"] = torch.utils.data.DataLoader(
                dataset, batch_size=256,
                sampler=torch.utils.data.SubsetRandomSampler(data.index.values.tolist()))
            made["nn"] = NeuralNetwork(input_dim=data.shape[1], output_dim=a.k, lr=a.lr,
                                       model_type=a.arch)
            _, made["train_batch"] = timed(
                lambda: made["nn"].train_batch(made["loader"], epochs=a.epochs), "train_batch")

        _, out["train"] = timed(train, "train")
        out["train_batch"] = made["train_batch"]
        pred, out["predict"] = timed(lambda: made["nn"].predict(data_X_to_torch(data)), "predict")
        out["total"] = out["cluster"] + out["train"] + out["predict"]
        out["label_agreement"] = float((pred == labels).mean())
        if a.verbatim_epochs > 0:
            os.environ["LMI_TRAIN_VERBATIM"] = "1"
            other = NeuralNetwork(input_dim=data.shape[1], output_dim=a.k, lr=a.lr, model_type=a.arch)
            _, t = timed(lambda: other.train_batch(made["loader"], epochs=a.verbatim_epochs),
                         "verbatim")
            out["verbatim_epochs"] = a.verbatim_epochs
            out["verbatim_epoch"] = t / a.verbatim_epochs
            out["forwards_per_verbatim_epoch"] = -(-a.n // 256)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))
    if "fused_step_us_median" in out and not (
            out["torch_step_us_median"] - out["fused_step_us_median"]
            > out["torch_step_us_spread"] + out["fused_step_us_spread"]):
        sys.exit("the fused step is not faster than the torch step by more than the two spreads")
    if "verbatim_epoch" in out and not out["train"] < out["verbatim_epoch"]:
        sys.exit(f"train phase {out['train']:.3f} s is not below one verbatim epoch "
                 f"{out['verbatim_epoch']:.3f} s")


if __name__ == "__main__":
    main()
