"""K6, the fused training step (lmi_mlp_train_steps, csrc/lmi_train.hip), and
what stands on it: NeuralNetwork.train_minibatch and
LearnedIndex.build(train_mode='minibatch').

The oracle is torch itself on the CPU in float64 -- the same Linear/ReLU
stack, CrossEntropyLoss() and torch.optim.Adam, fed the same initial weights
(cast up) and the same `order`, batch by batch.  The tolerance is relative to
torch's own float32 CPU training on the same order:

    max|kernel - f64| <= F * max(max|torch32 - f64|, 4 ulp of the tensor's
                                 largest magnitude)          per tensor,

for the loss, every W and b and every exp_avg / exp_avg_sq.

Ratios seen on an MI355X over 5 seeds and every shape and row count below
(each test prints its own before it asserts; DESIGN.md §3 K6 has the table):
loss 0.89, exp_avg 2.93, exp_avg_sq 2.20 -- F = 8 for these, twice the largest
rounded up to a power of two.  The parameters reached 22.5 (MLP, n = 40,
one step; MLP-5 11.8): not a kernel error but the conditioning of Adam's
update, -lr * g / (|g| + eps), whose slope at a gradient within a few eps = 1e-8
of zero is lr / eps = 1e6.  Every worst parameter is such an element; a 1e-11
difference in its gradient sum (a different but fixed summation order) moves it
by 1e-5, for torch's float32 as for the kernel: the two have the same rms error
per tensor, either may hold the larger maximum (torch32 5x the kernel's on some
seeds), and the moments, i.e. the gradient itself, agree within 3x.  So the
parameters are held to F_PARAM = 64 by the same rule (2 * 22.5 rounded up), and,
after one step, also to F = 8 on every parameter whose gradient is at least
100 eps away from zero ("param_wc", largest ratio seen 3.66)."""
import ctypes as C
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

from li import _lib
from li.index import DeviceIndex, DeviceRouter, Searcher
from li.LearnedIndex import LearnedIndex, dist_dtype
from li.model import Model, NeuralNetwork, data_X_to_torch
from li.utils import save_as_pickle

pytestmark = pytest.mark.gpu

F = 8.0
F_PARAM = 64.0
LR = 0.01
SHAPES = {
    "MLP": (96, 128, 122),
    "MLP-5": (96, 256, 128, 122),
    "MLP-8": (20, 8, 5),            # nothing a multiple of 4
    "MLP-6": (768, 32, 10),         # wide input
    "linear": (33, 7),              # one Linear, no hidden layer
}
ROWS = {"n700": (700, 256), "n257": (257, 256), "n40": (40, 256)}
# the widest rows the kernel takes (its largest LDS image), on the smallest batch
EXTRA = [("wide", (1000, 3, 1024), "n40")]
CASES = [(s, SHAPES[s], r) for s in SHAPES for r in ROWS] + EXTRA


def make_case(dims, n, seed):
    """(layers [(W, b)] float32 numpy, x [n, d] f32, y [n] int64, order int64)."""
    g = torch.Generator().manual_seed(1000 + seed)
    layers = []
    for a, b in zip(dims, dims[1:]):
        bound = 1.0 / np.sqrt(a)                                  # nn.Linear's default init
        w = (torch.rand(b, a, generator=g) * 2 - 1) * bound
        bb = (torch.rand(b, generator=g) * 2 - 1) * bound
        layers.append((w.numpy(), bb.numpy()))
    C_ = dims[-1]
    y = torch.randint(0, C_, (n,), generator=g)
    centres = torch.randn(C_, dims[0], generator=g)
    x = centres[y] + 0.5 * torch.randn(n, dims[0], generator=g)
    order = torch.randperm(n, generator=g)
    return layers, x.numpy().astype(np.float32), y.numpy(), order.numpy()


def torch_train(layers, x, y, order, batch, n_steps, dtype, first_step=0, state=None):
    """torch on the CPU: n_steps optimizer steps over order's minibatches.
    Returns (losses, params, exp_avg, exp_avg_sq), each a list of float64 numpy."""
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        lin.weight.data = torch.from_numpy(np.array(w)).to(dtype)
        lin.bias.data = torch.from_numpy(np.array(b)).to(dtype)
        mods.append(lin)
        if i + 1 < len(layers):
            mods.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*mods).to(dtype)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    lossf = torch.nn.CrossEntropyLoss()
    X, Y, O = torch.from_numpy(x).to(dtype), torch.from_numpy(y), torch.from_numpy(order)
    losses = []
    for s in range(first_step, first_step + n_steps):
        idx = O[s * batch:(s + 1) * batch]
        loss = lossf(net(X[idx]), Y[idx])
        losses.append(loss.item())
        net.zero_grad()
        loss.backward()
        opt.step()
    ps = list(net.parameters())
    out = lambda ts: [t.detach().double().numpy() for t in ts]
    return (np.array(losses, dtype=np.float64), out(ps), out([opt.state[p]["exp_avg"] for p in ps]),
            out([opt.state[p]["exp_avg_sq"] for p in ps]))


class KernelNet:
    """Parameters and moments in HBM, driven through the C ABI."""

    def __init__(self, layers, batch):
        self.dev = torch.device("cuda")
        self.p, self.m, self.v = [], [], []
        d = _lib.MlpTrainDesc()
        d.n_layers = len(layers)
        d.dims[0] = layers[0][0].shape[1]
        for i, (w, b) in enumerate(layers):
            d.dims[i + 1] = w.shape[0]
            for arr, names in ((w, ("W", "W_exp_avg", "W_exp_avg_sq")), (b, ("b", "b_exp_avg", "b_exp_avg_sq"))):
                p = torch.from_numpy(np.array(arr, dtype=np.float32)).to(self.dev)
                m, v = torch.zeros_like(p), torch.zeros_like(p)
                self.p.append(p), self.m.append(m), self.v.append(v)
                for name, t in zip(names, (p, m, v)):
                    getattr(d, name)[i] = t.data_ptr()
        self.desc, self.batch = d, batch
        self.need = _lib.load().lmi_mlp_train_workspace_bytes(C.byref(d), batch)
        assert self.need > 0
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=self.dev)

    def steps(self, x, y, order, first_step, n_steps, t0):
        """x, y, order: device tensors (f32 rows, int32 labels, int64 order)."""
        loss = torch.full((n_steps,), float("nan"), device=self.dev)
        _lib.check("lmi_mlp_train_steps", _lib.load().lmi_mlp_train_steps(
            C.byref(self.desc), x.data_ptr(), x.shape[0], x.stride(0), y.data_ptr(), order.data_ptr(),
            order.numel(), self.batch, first_step, n_steps, t0, LR, 0.9, 0.999, 1e-8, loss.data_ptr(),
            self.ws.data_ptr(), self.need, _lib.stream_handle(self.dev)))
        torch.cuda.synchronize()
        return loss.cpu().numpy()

    def tensors(self):
        cp = lambda ts: [t.cpu().numpy() for t in ts]
        return cp(self.p), cp(self.m), cp(self.v)


def upload(x, y, order):
    return (torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(),
            torch.from_numpy(order.astype(np.int64)).cuda())


def kernel_train(layers, x, y, order, batch, n_steps, first_step=0, t0=0):
    net = KernelNet(layers, batch)
    losses = net.steps(*upload(x, y, order), first_step, n_steps, t0)
    return (losses.astype(np.float64),) + net.tensors()


def ratios(kern, t32, t64, one_step=False):
    """Per tensor kind: the largest max|kernel - f64| / max(max|torch32 - f64|, 4 ulp).
    After one step also "param_wc": the same over the parameters whose gradient is at
    least 100 eps away from zero (the first step's gradient is exp_avg / (1 - beta1))."""
    worst = {}
    for kind, k, a, b in zip(("loss", "param", "exp_avg", "exp_avg_sq"), kern, t32, t64):
        ks, as_, bs = ([k], [a], [b]) if kind == "loss" else (k, a, b)
        for i, (kt, at, bt) in enumerate(zip(ks, as_, bs)):
            floor = 4.0 * float(np.spacing(np.float32(np.abs(bt).max())))
            err_k = np.abs(kt.astype(np.float64) - bt)
            err_t = np.abs(at - bt)
            worst[kind] = max(worst.get(kind, 0.0), float(err_k.max()) / max(float(err_t.max()), floor))
            if kind == "param" and one_step:
                wc = np.abs(t64[2][i]) / 0.1 >= 100 * 1e-8
                if wc.any():
                    worst["param_wc"] = max(worst.get("param_wc", 0.0),
                                            float(err_k[wc].max()) / max(float(err_t[wc].max()), floor))
    return worst


def check_case(dims, n, batch, seed, n_steps):
    layers, x, y, order = make_case(dims, n, seed)
    kern = kernel_train(layers, x, y, order, batch, n_steps)
    t64 = torch_train(layers, x, y, order, batch, n_steps, torch.float64)
    t32 = torch_train(layers, x, y, order, batch, n_steps, torch.float32)
    for ts in kern[1:]:
        assert all(np.isfinite(t).all() for t in ts)
    return ratios(kern, t32, t64, one_step=n_steps == 1)


@pytest.mark.parametrize("name,dims,rows", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_step_and_epoch_match_the_float64_oracle(name, dims, rows):
    n, batch = ROWS[rows]
    epoch = -(-n // batch)
    for n_steps in sorted({1, epoch}):
        r = check_case(dims, n, batch, seed=0, n_steps=n_steps)
        print(f"{name} {rows} steps={n_steps}: ratios "
              + ", ".join(f"{k} {v:.2f}" for k, v in r.items()))
        for kind, v in r.items():
            assert v <= (F_PARAM if kind == "param" else F), (name, rows, n_steps, kind, v)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_two_runs_are_bitwise_equal():
    layers, x, y, order = make_case(SHAPES["MLP-5"], 700, 3)
    a = kernel_train(layers, x, y, order, 256, 3)
    b = kernel_train(layers, x, y, order, 256, 3)
    assert np.array_equal(a[0], b[0])
    for ta, tb in zip(a[1:], b[1:]):
        assert _same(ta, tb)


@pytest.mark.parametrize("name", ["MLP-5", "MLP-8"])
def test_one_call_of_three_steps_is_three_calls_of_one(name):
    layers, x, y, order = make_case(SHAPES[name], 700, 4)
    whole = kernel_train(layers, x, y, order, 256, 3)
    net = KernelNet(layers, 256)
    dev = upload(x, y, order)
    losses = np.concatenate([net.steps(*dev, s, 1, s) for s in range(3)])
    assert np.array_equal(whole[0], losses.astype(np.float64))
    for ta, tb in zip(whole[1:], net.tensors()):
        assert _same(ta, tb)


def test_rows_outside_order_are_never_read():
    layers, x, y, _ = make_case(SHAPES["MLP"], 700, 5)
    order = np.random.default_rng(5).permutation(np.arange(0, 700, 2))       # even rows only
    poisoned = x.copy()
    poisoned[1::2] = np.nan
    clean = kernel_train(layers, x, y, order, 256, 2)
    dirty = kernel_train(layers, poisoned, y, order, 256, 2)
    assert np.isfinite(dirty[0]).all() and np.array_equal(clean[0], dirty[0])
    for ta, tb in zip(clean[1:], dirty[1:]):
        assert all(np.isfinite(t).all() for t in tb) and _same(ta, tb)


def _frame(n, d, c, seed=9, spread=0.15):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((c, d)).astype(np.float32)
    lab = rng.integers(0, c, n)
    df = pd.DataFrame((centres[lab] + spread * rng.standard_normal((n, d))).astype(np.float32))
    df.index += 1                                   # search.py:71-72
    return df, lab


def test_predict_after_training_uses_the_new_weights():
    df, lab = _frame(2000, 96, 12)
    X = data_X_to_torch(df)
    torch.manual_seed(11)
    nn = NeuralNetwork(input_dim=96, output_dim=12, lr=LR, model_type="MLP")
    before = nn.predict(X)
    assert nn._router is not None
    losses = nn.train_minibatch(X, torch.from_numpy(lab), epochs=2,
                                generator=torch.Generator().manual_seed(1))
    assert len(losses) == 2 and losses[1] < losses[0]
    after = nn.predict(X)
    fresh = DeviceRouter.from_module(nn.model, device=nn.device).argmax(X.to(nn.device)).cpu().numpy()
    assert np.array_equal(after, fresh)
    assert not np.array_equal(after, before)
    assert (after == lab).mean() > (before == lab).mean()


def test_train_batch_continues_from_the_minibatch_steps():
    n, batch = 700, 256
    layers, x, y, _ = make_case(SHAPES["MLP"], n, 6)
    nn = NeuralNetwork(input_dim=96, output_dim=122, lr=LR, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (w, b) in zip(lin, layers):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    nn.train_minibatch(X, Y, epochs=1, batch_size=batch, generator=torch.Generator().manual_seed(2))
    p0 = lin[0].weight
    assert int(nn.optimizer.state[p0]["step"]) == 3
    assert set(nn.optimizer.state[p0]) == {"step", "exp_avg", "exp_avg_sq"}
    nn.train_batch([(X, Y)], epochs=1)              # one full-batch step: Adam step 4
    assert int(nn.optimizer.state[p0]["step"]) == 4
    got = p0.detach().cpu().double().numpy()

    order = torch.randperm(n, generator=torch.Generator().manual_seed(2)).numpy()
    order = np.concatenate([order, np.arange(n)])   # steps 0..2 of 256/256/188 rows, then all rows

    def continued(dtype):
        # the same three minibatch steps, then the full batch as a fourth step
        mods = []
        for i, (w, b) in enumerate(layers):
            l_ = torch.nn.Linear(w.shape[1], w.shape[0])
            l_.weight.data, l_.bias.data = torch.from_numpy(w.copy()).to(dtype), torch.from_numpy(b.copy()).to(dtype)
            mods += [l_] + ([torch.nn.ReLU()] if i + 1 < len(layers) else [])
        net = torch.nn.Sequential(*mods)
        opt = torch.optim.Adam(net.parameters(), lr=LR)
        Xd = X.to(dtype)
        for idx in (order[:256], order[256:512], order[512:700], order[700:]):
            loss = torch.nn.CrossEntropyLoss()(net(Xd[idx]), Y[idx])
            net.zero_grad()
            loss.backward()
            opt.step()
        return net[0].weight.detach().double().numpy()

    w64, w32 = continued(torch.float64), continued(torch.float32)
    floor = 4.0 * float(np.spacing(np.float32(np.abs(w64).max())))
    ratio = np.abs(got - w64).max() / max(np.abs(w32 - w64).max(), floor)
    print(f"train_minibatch + train_batch: ratio {ratio:.2f}")
    assert ratio <= F_PARAM                         # a parameter tensor: check 1's bound for those


_BUILT = {}
N, D, NC = 6000, 96, 30


def _build(mode):
    if mode not in _BUILT:
        df, _ = _frame(N, D, NC)
        cpu_rng = torch.get_rng_state()
        torch.manual_seed(2023)
        li = LearnedIndex()
        pred, seconds = li.build(df, n_categories=NC, epochs=2, lr=LR, model_type="MLP", train_mode=mode)
        torch.set_rng_state(cpu_rng)
        _BUILT[mode] = (df, li, pred)
    return _BUILT[mode]


def _oracle_share(df, labels):
    """The float64 oracle of the minibatch build: the same seed, hence the same
    initial weights and epoch orders as _build draws them."""
    cpu_rng = torch.get_rng_state()
    torch.manual_seed(2023)
    net = Model(D, NC, model_type="MLP")
    layers = [(m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy())
              for m in net.layers if isinstance(m, torch.nn.Linear)]
    orders = [torch.randperm(N).numpy(), torch.randperm(N).numpy()]
    torch.set_rng_state(cpu_rng)
    W = [torch.from_numpy(p) for p in _oracle_epochs(layers, df.to_numpy(), labels, orders)]
    h = torch.from_numpy(df.to_numpy()).double()
    for i in range(0, len(W), 2):
        h = h @ W[i].T + W[i + 1]
        if i + 2 < len(W):
            h = torch.relu(h)
    return float((h.argmax(1).numpy() == labels).mean())


def _oracle_epochs(layers, x, y, orders):
    mods = []
    for i, (w, b) in enumerate(layers):
        l_ = torch.nn.Linear(w.shape[1], w.shape[0])
        l_.weight.data, l_.bias.data = torch.from_numpy(w).double(), torch.from_numpy(b).double()
        mods += [l_] + ([torch.nn.ReLU()] if i + 1 < len(layers) else [])
    net = torch.nn.Sequential(*mods)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    X, Y = torch.from_numpy(x).double(), torch.from_numpy(y)
    for o in orders:
        o = torch.from_numpy(o)
        for s in range(0, len(o), 256):
            idx = o[s:s + 256]
            loss = torch.nn.CrossEntropyLoss()(net(X[idx]), Y[idx])
            net.zero_grad()
            loss.backward()
            opt.step()
    return [p.detach().numpy() for p in net.parameters()]


def test_minibatch_build_end_to_end():
    df, li, pred = _build("minibatch")
    _, ref, ref_pred = _build("reference")
    assert isinstance(pred, np.ndarray) and pred.dtype == np.int64 and pred.shape == (N,)
    assert np.array_equal(pred, li.model.predict(data_X_to_torch(df)))
    _, labels = LearnedIndex().cluster(df, NC)
    share, ref_share = float((pred == labels).mean()), float((ref_pred == labels).mean())
    print(f"router label == k-means label: minibatch {share:.4f} (48 steps), reference "
          f"{ref_share:.4f} (2 steps), float64 oracle of the minibatch build "
          f"{_oracle_share(df, labels):.4f}")
    assert share > ref_share
    # LearnedIndex.search over the built labels == Searcher.search with the same router and labels
    x = df.to_numpy().astype(np.float16).astype(np.float32)
    data_search = pd.DataFrame(x)
    data_search.index += 1
    rng = np.random.default_rng(3)
    rows = rng.choice(N, 64, replace=False)
    q = (x[rows] + 0.05 * rng.standard_normal((64, D))).astype(np.float16).astype(np.float32)
    q_nav = df.to_numpy()[rows]
    dists, anns = li.search(df.copy(), q_nav, data_search, q, pred, n_buckets=2, k=10)
    s = Searcher(DeviceIndex(x, pred, NC, ids=np.asarray(df.index)), li.model.router())
    rd, ra = s.search(torch.from_numpy(q_nav).cuda(), torch.from_numpy(q).cuda(), 2, k=10, k_round=10,
                      use_threshold=False, dist=dist_dtype(data_search, q))
    assert np.array_equal(anns, ra) and np.array_equal(dists, rd)


def test_minibatch_built_index_pickles_like_a_reference_build(tmp_path):
    _, li, pred = _build("minibatch")
    _, ref, _ = _build("reference")
    loaded = {}
    for name, obj in (("minibatch", li), ("reference", ref)):
        path = str(tmp_path / f"{name}.pkl")
        save_as_pickle(path, obj)
        with open(path, "rb") as f:
            loaded[name] = pickle.load(f)
    a, b = loaded["minibatch"], loaded["reference"]
    assert set(vars(a)) == set(vars(b))
    assert set(vars(a.model)) == set(vars(b.model))
    assert set(vars(a.model)) == set(ref.model.__getstate__())
    sa, sb = a.model.optimizer.state_dict()["state"], b.model.optimizer.state_dict()["state"]
    assert sa.keys() == sb.keys() and all(set(sa[k]) == set(sb[k]) for k in sa)
    df = _BUILT["minibatch"][0]
    assert np.array_equal(a.model.predict(data_X_to_torch(df)), pred)
