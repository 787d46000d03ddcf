"""LearnedIndex.build end to end on the GPU (LearnedIndex.py:197-240): k-means
labels (K5), the router trained on each epoch's last minibatch
(NeuralNetwork.train_batch), labels from the router kernel's argmax (K1) --
and a search on the index it made.  Two frames: 96-wide navigation (the pca96
shape, narrow k-means kernel) and 192-wide (the wide k-means kernel and a
router input wider than 128).  The last-batch path is held to the verbatim
loop (LMI_TRAIN_VERBATIM=1) from the same seeds, bitwise: both issue the same
torch calls on the same shapes, on the minibatch the reference steps on."""
import numpy as np
import pandas as pd
import pytest
import torch

from li.index import DeviceIndex, Searcher
from li.LearnedIndex import LearnedIndex, dist_dtype
from li.model import data_X_to_torch

pytestmark = pytest.mark.gpu

EPOCHS = 8
CASES = {"nav96": (6000, 96, 30, "MLP"), "nav192": (3000, 192, 12, "MLP-5")}
_BUILT = {}


def _frame(n, d, c, seed=9, spread=0.15):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((c, d)).astype(np.float32)
    lab = rng.integers(0, c, n)
    df = pd.DataFrame((centres[lab] + spread * rng.standard_normal((n, d))).astype(np.float32))
    df.index += 1                                   # search.py:71-72
    return df


def _build(name, verbatim=False):
    """One seeded build per (case, loop), shared by the tests."""
    key = (name, verbatim)
    if key not in _BUILT:
        n, d, c, arch = CASES[name]
        df = _frame(n, d, c)
        mp = pytest.MonkeyPatch()
        try:
            if verbatim:
                mp.setenv("LMI_TRAIN_VERBATIM", "1")
            else:
                mp.delenv("LMI_TRAIN_VERBATIM", raising=False)
            cpu_rng = torch.get_rng_state()
            torch.manual_seed(2023)
            li = LearnedIndex()
            pred, seconds = li.build(df, n_categories=c, epochs=EPOCHS, lr=0.01, model_type=arch)
            torch.set_rng_state(cpu_rng)
        finally:
            mp.undo()
        _BUILT[key] = (df, li, pred, seconds)
    return _BUILT[key]


@pytest.mark.parametrize("name", list(CASES))
def test_build_labels_are_the_routers(name):
    n, d, c, arch = CASES[name]
    df, li, pred, seconds = _build(name)
    assert li.model is not None and seconds > 0
    assert isinstance(pred, np.ndarray) and pred.dtype == np.int64 and pred.shape == (n,)
    assert pred.min() >= 0 and pred.max() < c
    assert (pred == li.model.predict(data_X_to_torch(df))).all()
    # the router learned something of the clustering in 8 steps: more than one bucket in use
    assert np.unique(pred).size > 1


@pytest.mark.parametrize("name", list(CASES))
def test_search_on_the_built_index(name):
    """LearnedIndex.search over the built labels == Searcher.search with the
    same router and labels."""
    n, d, c, arch = CASES[name]
    df, li, pred, _ = _build(name)
    x = df.to_numpy().astype(np.float16).astype(np.float32)     # fp16-exact search vectors
    data_search = pd.DataFrame(x)
    data_search.index += 1                                      # search.py:83-84
    rng = np.random.default_rng(3)
    rows = rng.choice(n, 64, replace=False)
    q = (x[rows] + 0.05 * rng.standard_normal((64, d))).astype(np.float16).astype(np.float32)
    q_nav = df.to_numpy()[rows]
    data = df.copy()
    dists, anns = li.search(data, q_nav, data_search, q, pred, n_buckets=2, k=10)
    assert dists.shape == (64, 10) and anns.dtype == np.uint32
    assert (np.asarray(data["category"]) == pred).all()         # LearnedIndex.py:67
    s = Searcher(DeviceIndex(x, pred, c, ids=np.asarray(df.index)), li.model.router())
    rd, ra = s.search(torch.from_numpy(q_nav).cuda(), torch.from_numpy(q).cuda(), 2, k=10, k_round=10,
                      use_threshold=False, dist=dist_dtype(data_search, q))
    assert np.array_equal(anns, ra) and np.array_equal(dists, rd)
    # answers are ids of the frame (1-based), the fill id 0 aside
    assert anns.max() <= n


@pytest.mark.parametrize("name", list(CASES))
def test_last_batch_build_is_the_verbatim_build_bitwise(name):
    _, fast, fast_pred, _ = _build(name)
    _, slow, slow_pred, _ = _build(name, verbatim=True)
    fs, ss = fast.model.model.state_dict(), slow.model.model.state_dict()
    assert fs.keys() == ss.keys()
    for key in fs:
        diff = (fs[key].double() - ss[key].double()).abs().max().item()
        print(f"{name} {key}: max |fast - verbatim| = {diff:.3e}")
    for key in fs:
        assert torch.equal(fs[key], ss[key]), key
    assert np.array_equal(fast_pred, slow_pred)
