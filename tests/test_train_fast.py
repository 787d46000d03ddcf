"""NeuralNetwork.train_batch's last-batch path (li/model.py) against the
reference's loop, on the CPU.

The reference (model.py:174-199) runs a forward over every minibatch of an
epoch and steps once on the last one's loss; the drop-in computes that last
minibatch alone.  Pinned here: bitwise the same weights, losses, logger lines
and final RNG state as the verbatim loop (LMI_TRAIN_VERBATIM=1) from equal
seeds; which arguments take which loop (a forward counter); and, against a
run of the reference itself (tests/golden/gen_golden_train.py ->
reference_train.npz), the ids of every epoch's last minibatch exactly, and the
weights and losses bitwise where torch and the CPU's instruction set are the
recorded ones."""
import os

import numpy as np
import pandas as pd
import pytest
import torch
import torch.utils.data as D

import li.model as M

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                            "reference_train.npz"))
DIM, CLASSES, EPOCHS, SEED = 24, 7, 12, 2023


@pytest.fixture(autouse=True)
def _cpu_and_rng(monkeypatch):
    """Train on the CPU whatever the host has, and leave the process's RNG
    state and thread count as they were."""
    monkeypatch.setattr(M, "get_device", lambda: torch.device("cpu"))
    monkeypatch.delenv("LMI_TRAIN_VERBATIM", raising=False)
    state, threads = torch.get_rng_state(), torch.get_num_threads()
    yield
    torch.set_rng_state(state)
    torch.set_num_threads(threads)


class _Lines:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _frame(n):
    rng = np.random.default_rng(n)
    df = pd.DataFrame(rng.standard_normal((n, DIM)).astype(np.float32))
    df.index += 1
    return df, rng.integers(0, CLASSES, n).astype(np.int64)


def _loader(df, labels, **kw):
    kw.setdefault("sampler", D.SubsetRandomSampler(df.index.values.tolist()))
    return D.DataLoader(M.LIDataset(df, labels), batch_size=256, **kw)   # LearnedIndex.build


def _train(make_batches, arch, epochs=EPOCHS, init=None, lr=0.01):
    """(state_dict, losses, logger lines, RNG state after, forwards) of one
    seeded run; make_batches() -> train_batch's argument."""
    torch.manual_seed(SEED)
    batches = make_batches()
    nn = M.NeuralNetwork(input_dim=DIM, output_dim=CLASSES, lr=lr, model_type=arch)
    if init is not None:
        nn.model.load_state_dict(init)
    forwards = [0]
    inner = nn.model.forward

    def counting(x):
        forwards[0] += 1
        return inner(x)

    nn.model.forward = counting
    log = _Lines()
    losses = nn.train_batch(batches, epochs=epochs, logger=log)
    state = {k: v.detach().clone() for k, v in nn.model.state_dict().items()}
    return state, losses, log.lines, torch.get_rng_state(), forwards[0]


@pytest.mark.parametrize("n,arch", [(100, "MLP"), (512, "MLP-5"), (1000, "MLP"), (1001, "MLP-5")])
def test_fast_path_is_the_verbatim_loop_bitwise(n, arch, monkeypatch):
    """A lone short batch (100), a full last batch (512), a 232-row tail (1000)
    and a one-row tail (1001)."""
    df, labels = _frame(n)
    fast = _train(lambda: _loader(df, labels), arch)
    monkeypatch.setenv("LMI_TRAIN_VERBATIM", "1")
    slow = _train(lambda: _loader(df, labels), arch)
    assert fast[4] == EPOCHS and slow[4] == EPOCHS * -(-n // 256)
    assert fast[0].keys() == slow[0].keys()
    for key in fast[0]:
        assert torch.equal(fast[0][key], slow[0][key]), key
    assert fast[1] == slow[1] and len(fast[1]) == EPOCHS
    assert fast[2] == slow[2] and len(fast[2]) == EPOCHS      # "Epochs: ..." + epochs 1..11
    assert torch.equal(fast[3], slow[3])
    # and it trained: not the initial weights
    torch.manual_seed(SEED)
    init = M.NeuralNetwork(input_dim=DIM, output_dim=CLASSES, lr=0.01, model_type=arch).model
    assert not torch.equal(init.state_dict()["layers.0.weight"], fast[0]["layers.0.weight"])


def test_other_arguments_take_the_verbatim_loop():
    n = 600                                                    # 3 minibatches
    df, labels = _frame(n)
    assert _train(lambda: _loader(df, labels), "MLP", epochs=4)[4] == 4
    # another sampler
    ds = M.LIDataset(df, labels)
    seq = lambda: D.DataLoader(ds, batch_size=256, sampler=D.SequentialSampler(range(1, n + 1)))
    assert _train(seq, "MLP", epochs=4)[4] == 4 * 3
    # a plain list of (X, y) batches
    x, y = ds.dataset_x, ds.dataset_y
    batches = [(x[i:i + 256], y[i:i + 256]) for i in range(0, n, 256)]
    assert _train(lambda: batches, "MLP", epochs=4)[4] == 4 * 3
    # drop_last, a collate function of the caller's, a Dataset subclass with its own __getitem__
    assert _train(lambda: _loader(df, labels, drop_last=True), "MLP", epochs=2)[4] == 2 * 2
    assert _train(lambda: _loader(df, labels, collate_fn=lambda b: D.default_collate(b)), "MLP",
                  epochs=2)[4] == 2 * 3

    class Other(M.LIDataset):
        def __getitem__(self, idx):
            return super().__getitem__(idx)

    other = lambda: D.DataLoader(Other(df, labels), batch_size=256,
                                 sampler=D.SubsetRandomSampler(df.index.values.tolist()))
    assert _train(other, "MLP", epochs=2)[4] == 2 * 3


def test_model_with_other_modules_takes_the_verbatim_loop(monkeypatch):
    """Only Linear/ReLU stacks have forwards without side effects (a Dropout
    would draw from the generator, a BatchNorm would move its statistics)."""
    df, labels = _frame(600)
    real = M.Model

    class WithDropout(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.layers = torch.nn.Sequential(*self.layers, torch.nn.Dropout(0.0))

    monkeypatch.setattr(M, "Model", WithDropout)
    assert _train(lambda: _loader(df, labels), "MLP", epochs=2)[4] == 2 * 3


def test_last_batch_indices_wraps_like_getitem(monkeypatch):
    """A sampler over 0-based ids: id 0 reads row -1, as LIDataset.__getitem__
    (idx - 1) does in the verbatim loop."""
    n = 300
    df, labels = _frame(n)
    zero_based = lambda: _loader(df, labels, sampler=D.SubsetRandomSampler(list(range(n))))
    fast = _train(zero_based, "MLP", epochs=6)
    monkeypatch.setenv("LMI_TRAIN_VERBATIM", "1")
    slow = _train(zero_based, "MLP", epochs=6)
    assert (fast[4], slow[4]) == (6, 12)
    assert fast[1] == slow[1] and all(torch.equal(fast[0][k], slow[0][k]) for k in fast[0])
    ids = M.last_batch_indices(torch.arange(n), 256, None, None)
    assert ids.dtype == torch.int64 and ids.shape == (n - 256,)


def _golden_frame():
    df = pd.DataFrame(GOLD["x16"].astype(np.float32))
    df.index += 1
    return df, GOLD["labels"].astype(np.int64)


def test_last_batch_ids_are_the_reference_samplers():
    """The ids the reference's DataLoader asked its dataset for in the last
    minibatch of each of its 12 epochs: integers of the CPU generator, equal
    on every machine."""
    n, d, c, epochs, batch, seed = (int(v) for v in GOLD["meta"])
    assert (n, d, c, epochs, seed) == (1000, DIM, CLASSES, EPOCHS, SEED)
    df, labels = _golden_frame()
    torch.manual_seed(seed)
    _loader(df, labels)
    M.NeuralNetwork(input_dim=d, output_dim=c, lr=float(GOLD["lr"]), model_type=str(GOLD["arch"]))
    indices = torch.tensor(df.index.values.tolist())
    for ep in range(epochs):
        got = M.last_batch_indices(indices, batch, None, None)
        assert got.tolist() == GOLD["last_ids"][ep].tolist(), f"epoch {ep}"


def test_training_is_the_references_bitwise():
    same = (str(GOLD["torch_version"]) == torch.__version__
            and str(GOLD["cpu_capability"]) == torch.backends.cpu.get_cpu_capability())
    if not same:
        pytest.skip(f"fixture floats are torch {GOLD['torch_version']} / {GOLD['cpu_capability']}'s; "
                    f"here {torch.__version__} / {torch.backends.cpu.get_cpu_capability()}")
    torch.set_num_threads(1)                                   # as the fixture was made
    df, labels = _golden_frame()
    keys = [k[len("init__"):] for k in GOLD.files if k.startswith("init__")]
    init = {k: torch.from_numpy(GOLD[f"init__{k}"]) for k in keys}
    # (the reference's Model draws the same initial weights from the seed)
    torch.manual_seed(SEED)
    fresh = M.NeuralNetwork(input_dim=DIM, output_dim=CLASSES, model_type=str(GOLD["arch"])).model
    for k in keys:
        assert torch.equal(fresh.state_dict()[k], init[k]), k
    state, losses, _, _, forwards = _train(lambda: _loader(df, labels), str(GOLD["arch"]), init=init,
                                           lr=float(GOLD["lr"]))
    assert forwards == EPOCHS
    assert losses == GOLD["losses"].tolist()
    for k in keys:
        assert torch.equal(state[k], torch.from_numpy(GOLD[f"final__{k}"])), k
