"""Shapes and inputs of the router checks (tests/test_oracle_router64.py on the
CPU, tests/test_gpu_router.py on the device): Linear/ReLU stacks by their
widths, torch-like weights (uniform +-1/sqrt(in), seeded), unit-norm rows, the
float64 oracle of each case computed once and shared read-only."""
import functools
import zlib

import numpy as np

import lmi_oracle as O

N = 257

# name -> widths (input, hidden ..., classes) and the K1 code each reaches,
# read from lmi_router's dispatch (csrc/lmi_router.hip):
#   MFMA  = router_mfma_kernel (input and hidden widths multiples of 16)
#   FMA32 / FMA16 = router_kernel<32> / <16> (16 once the widest layer > 576)
#   vec4 / scalar = the weight staging branch; blocks = more than one column block
SHAPES = {
    "MLP": (96, 128, 122),            # MFMA
    "MLP-5": (96, 256, 128, 122),     # MFMA, two hidden layers
    "MLP-4": (96, 512, 122),          # MFMA, 32 output tiles: two passes per wave
    "MLP-7": (96, 16, 122),           # MFMA, one output tile
    "MLP-8": (96, 8, 122),            # FMA32 vec4
    "MLP-2": (96, 64, 122),           # MFMA (the remaining model types)
    "MLP-3": (96, 256, 122),          # MFMA
    "MLP-6": (96, 32, 122),           # MFMA
    "odd": (20, 8, 5),                # FMA32 vec4 (20 and 8 are multiples of 4), C < 8
    "linear": (33, 7),                # FMA32 scalar, one layer, no ReLU
    "one": (1, 1, 1),                 # FMA32 scalar, C = 1
    "c3": (32, 16, 3),                # MFMA, C < 4 lane groups
    "c64": (96, 100, 64),             # FMA32 vec4, one wave of classes
    "c65": (96, 100, 65),             # FMA32 vec4, one class past the wave
    "nav768": (768, 128, 1000),       # MFMA, 1000 classes
    "deep16": (16,) * 8 + (10,),      # MFMA, LMI_MAX_LAYERS layers
    "deep12": (12,) * 8 + (10,),      # FMA32 vec4, LMI_MAX_LAYERS layers
    "max": (1024, 1024, 3),           # MFMA at LMI_ROUTER_MAX_DIM
    "wide-in-narrow": (768, 8, 122),  # FMA16 vec4, blocks
    "many-classes": (96, 8, 1000),    # FMA16 vec4, blocks
    "wide": (1000, 3, 1024),          # FMA16 scalar, blocks
    "mis768": (768, 128, 122),        # (misaligned weights: FMA16 scalar, blocks)
}
TABLE = [k for k in SHAPES if k != "mis768"]


def make_layers(dims, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    layers = []
    for a, b in zip(dims, dims[1:]):
        bound = 1.0 / np.sqrt(a)
        layers.append((rng.uniform(-bound, bound, (b, a)).astype(np.float32),
                       rng.uniform(-bound, bound, (b,)).astype(np.float32)))
    return layers


def make_rows(n, d, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


class Case:
    def __init__(self, name, dims, n, layers=None):
        seed = zlib.crc32(name.encode())
        self.name, self.dims, self.n = name, tuple(dims), n
        self.layers = layers if layers is not None else make_layers(dims, seed)
        self.x = make_rows(n, dims[0], seed + 1)
        self.l64, self.err = O.mlp_forward64(self.x, self.layers)
        self.clear, self.top64 = O.router_clear_rows(self.l64, self.err)
        self.C = dims[-1]
        for a in (self.x, self.l64, self.err, self.clear, self.top64):
            a.setflags(write=False)

    def Rs(self):
        return sorted({1, min(8, self.C), min(9, self.C), self.C})


@functools.lru_cache(maxsize=None)
def case(name, n=N):
    return Case(name, SHAPES[name], n)


def torch32_forward(x, layers):
    """torch's own CPU float32 Linear/ReLU forward."""
    import torch
    h = torch.from_numpy(np.array(x, np.float32))
    for i, (w, b) in enumerate(layers):
        h = torch.nn.functional.linear(h, torch.from_numpy(np.ascontiguousarray(w, np.float32)),
                                       torch.from_numpy(np.ascontiguousarray(b, np.float32)))
        if i + 1 < len(layers):
            h = torch.relu(h)
    return h.numpy()


def chain32_forward(x, layers):
    """The FMA kernel's arithmetic: b[o], then one float32 fma per term in
    ascending i (the float64 product of two float32 values is exact, so a
    float64 add rounded to float32 is the fma)."""
    h = np.asarray(x, np.float32)
    for li, (w, b) in enumerate(layers):
        w = np.asarray(w, np.float32).astype(np.float64)
        acc = np.broadcast_to(np.asarray(b, np.float32), (h.shape[0], w.shape[0])).copy()
        h64 = h.astype(np.float64)
        for k in range(w.shape[1]):
            acc = (acc.astype(np.float64) + h64[:, k, None] * w[None, :, k]).astype(np.float32)
        h = np.maximum(acc, np.float32(0)) if li + 1 < len(layers) else acc
    return h


def answer32(logits32, R):
    """(classes, probs) as a float32 router gives them from its logits:
    descending logit, ties to the lower class, float32 softmax."""
    logits32 = np.asarray(logits32, np.float32)
    cls = O.rank_classes(logits32)[:, :R]
    return cls, np.take_along_axis(O.softmax(logits32), cls, axis=1)
