"""Router (K1) timing: topr / argmax for 10k queries on a few synthetic
architectures, torch events around the launches (diagnostic).

--stop-mass P also times topr with the stop rule (lmi_router_stop, the same
launch as topr), `--reps` rounds of every mode one after another: the rounds'
median and spread (max - min) per mode."""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"))
import torch
from li.index import DeviceRouter

ap = argparse.ArgumentParser()
ap.add_argument("--stop-mass", type=float, default=None)
ap.add_argument("--reps", type=int, default=1)
a = ap.parse_args()

dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
for arch, hidden in [("MLP-5", (256, 128)), ("MLP", (128,)), ("MLP-8", (8,))]:
    dims = (96,) + hidden + (122,)
    layers = [((torch.randn(dims[i + 1], dims[i], generator=g) * 0.1).numpy(),
               (torch.randn(dims[i + 1], generator=g) * 0.1).numpy()) for i in range(len(dims) - 1)]
    router = DeviceRouter(layers)
    x = torch.nn.functional.normalize(torch.randn(10000, 96, generator=g), dim=1).to(dev)
    fns = {"topr": lambda: router.topr(x, 4), "argmax": lambda: router.argmax(x)}
    if a.stop_mass is not None:
        fns["stop"] = lambda: router.topr(x, 4, stop_mass=a.stop_mass)
    us = {m: [] for m in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    for _ in range(a.reps):
        for mode, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[mode].append(e0.elapsed_time(e1) / 20 * 1e3)
    for mode, v in us.items():
        v = sorted(v)
        print(f"{arch:6s} {mode:6s} {v[len(v) // 2]:8.1f} us"
              + (f"  (spread {v[-1] - v[0]:.1f} us over {len(v)} rounds)" if len(v) > 1 else ""),
              flush=True)
