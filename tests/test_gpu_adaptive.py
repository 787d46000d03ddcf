"""Adaptive probing end to end: Searcher.search / the batch stream / the step
graph / LearnedIndex.search with the router's stop rule (stop_mass) against the
CPU oracle given the kernel's masked classes.

The test workloads' routers have random weights and are near uniform (top-1
probability about 1/C), so the last layer's weights and bias are multiplied by
100: at R = 4, stop mass 0.8 the rule then keeps 1, 2, 3 and 4 probes on
66, 78, 45 and 11 of the 200 queries (CPU oracle, float32 softmax), and the
cumulative mass nearest to 0.8 is 5.9e-4 away -- far above float32 softmax
rounding, so the kernel's mask is that mask.

A dropped probe's class is -1: the plan, the lists, the float64 refinement,
the split mode and both replays treat it as a probe with no bucket, and the
oracle (bucket_lists, replay, search_direct, search_exact) as a round whose
category matches no bucket.  Comparator and tolerances are those of
tests/test_gpu_parity.py for the same workloads (O.compare_lists: defaults in
float32, atol = tie = 1e-12 in float64)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import lmi_oracle as O
import workloads
from li.index import DeviceIndex, DeviceRouter, Searcher, probe_stop_mask

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R, K, STOP = 4, 10, 0.8
MODES = ("skewed", "near")
T = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the shared arrays are read-only)


def _sharpen(layers):
    out = [(w.copy(), b.copy()) for w, b in layers]
    out[-1] = (out[-1][0] * np.float32(100), out[-1][1] * np.float32(100))
    return out


@functools.lru_cache(maxsize=None)
def setup(mode):
    """The workload, its Searcher and the kernel's masked classes (shared, read-only)."""
    w = workloads.clustered(n=6000, d=768, nq=200, C=16, arch="MLP", label_mode=mode)
    w["layers"] = _sharpen(w["layers"])
    router = DeviceRouter(w["layers"], device="cuda")
    s = Searcher(DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=512, device="cuda"), router)
    qn = T(w["qn"])
    cls, probs = router.topr(qn, R, with_probs=True, stop_mass=STOP)
    cls, probs = cls.cpu().numpy(), probs.cpu().numpy()
    plain = router.topr(qn, R)[0].cpu().numpy()
    for a in (cls, probs, plain, w["x"], w["q"], w["qn"], w["labels"]):
        a.setflags(write=False)
    return w, s, cls, probs, plain


def _inputs(w, dist):
    # float16 operands make the oracle compute in float64 (sklearn's rule), as
    # dist="f64" does; the values are fp16-exact
    if dist == "f64":
        return w["x"].astype(np.float16), w["q"].astype(np.float16)
    return w["x"], w["q"]


def _tol(dist):
    return {} if dist == "f32" else dict(atol=1e-12, tie=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_kernel_mask_has_every_probe_count(mode):
    w, s, cls, probs, plain = setup(mode)
    keep = cls >= 0
    counts = np.bincount(keep.sum(1), minlength=R + 1)
    print(f"{mode}: probe-count histogram {counts[1:].tolist()}, nearest mass to {STOP}: "
          f"{np.abs(np.cumsum(probs, axis=1, dtype=np.float32) - np.float32(STOP)).min():.2e}")
    assert counts[0] == 0 and (counts[1:] > 0).all(), counts
    assert np.array_equal(keep, probe_stop_mask(probs, STOP, 1))
    assert np.array_equal(cls[keep], plain[keep]) and (cls[~keep] == -1).all()
    # Searcher.route is the same call
    assert np.array_equal(s.route(T(w["qn"]), R, stop_mass=STOP).cpu().numpy(), cls)


@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
def test_search_matches_oracle_given_the_masked_classes(mode, dist):
    w, s, cls, _, _ = setup(mode)
    ids = np.arange(1, w["x"].shape[0] + 1)
    x, q = _inputs(w, dist)
    qn, qs = T(w["qn"]), T(w["q"])
    fixed = s.search(qn, qs, R, k=K, dist=dist)
    for thr in (False, True):
        d, a = s.search(qn, qs, R, k=K, use_threshold=thr, dist=dist, stop_mass=STOP)
        rd, ra = O.search_direct(w["labels"], ids, x, q, cls, n_buckets=R, k=K, use_threshold=thr)
        assert d.shape == rd.shape and a.dtype == np.uint32
        assert O.compare_lists(rd, ra, d, a, **_tol(dist)) == 0, (mode, dist, thr)
        # the rule is the router's alone: the same answer from the masked classes
        d2, a2 = s.search(qn, qs, R, k=K, use_threshold=thr, dist=dist, classes=T(cls))
        assert np.array_equal(d, d2) and np.array_equal(a, a2)
        # the host replay agrees with the device replay on -1 classes
        d3, a3 = s.search(qn, qs, R, k=K, use_threshold=thr, dist=dist, stop_mass=STOP,
                          replay_on="host")
        assert np.array_equal(d, d3) and np.array_equal(a, a3)
    # (thr = True is the default): the mask is not ignored
    differ = int(((fixed[1] != a) | (fixed[0] != d)).any(axis=1).sum())
    print(f"{mode} {dist}: {differ} of 200 rows differ from the fixed R = {R} answer")
    assert differ >= 100
    d, a = s.search(qn, qs, R, k=K, semantics="exact", dist=dist, stop_mass=STOP)
    rd, ra = O.search_exact(w["labels"], ids, x, q, cls, w["C"], R, K)
    assert O.compare_lists(rd, ra, d, a, **_tol(dist)) == 0, (mode, dist, "exact")
    d2, a2 = s.search(qn, qs, R, k=K, semantics="exact", dist=dist, classes=T(cls))
    assert np.array_equal(d, d2) and np.array_equal(a, a2)


def test_min_probes_and_timings():
    w, s, cls, probs, _ = setup("skewed")
    qn, qs = T(w["qn"]), T(w["q"])
    keep2 = probe_stop_mask(probs, STOP, 2)
    got = s.route(qn, R, stop_mass=STOP, min_probes=2).cpu().numpy()
    assert np.array_equal(got >= 0, keep2) and (keep2.sum(1) >= 2).all()
    tm = {}
    d, a = s.search(qn, qs, R, k=K, stop_mass=STOP, timings=tm)
    assert tm["mean_probes"] == pytest.approx((cls >= 0).sum() / 200.0, abs=1e-12)
    d0, a0 = s.search(qn, qs, R, k=K, stop_mass=STOP)
    assert np.array_equal(d, d0) and np.array_equal(a, a0)
    tm = {}
    s.search(qn, qs, R, k=K, timings=tm)
    assert "mean_probes" not in tm
    # one probe: nothing to stop
    d1, a1 = s.search(qn, qs, 1, k=K, stop_mass=STOP)
    d1p, a1p = s.search(qn, qs, 1, k=K)
    assert np.array_equal(d1, d1p) and np.array_equal(a1, a1p)


def _two_batches(w):
    p = np.random.Generator(np.random.PCG64(99)).permutation(w["q"].shape[0])
    return [(w["qn"], w["q"]), (w["qn"][p], w["q"][p])]


@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
def test_stream_and_graph_equal_search(mode, dist):
    """Six steps over two distinct batches (the four-slot pipeline wraps): the
    captured router call carries the rule."""
    w, s, cls, _, _ = setup(mode)
    two = _two_batches(w)
    ref = [s.search(T(a), T(b), R, k=K, dist=dist, stop_mass=STOP) for a, b in two]
    assert not np.array_equal(ref[0][1], ref[1][1])
    plain0 = s.search(T(two[0][0]), T(two[0][1]), R, k=K, dist=dist)
    assert not np.array_equal(ref[0][1], plain0[1])
    batches = [two[i % 2] for i in range(6)]
    with s.streamed(w["qn"], w["q"], R, k=K, dist=dist, stop_mass=STOP) as st:
        got = list(st.stream(batches))
        assert st.launches >= 3
    assert len(got) == 6
    for i, (d, a) in enumerate(got):
        assert np.array_equal(d, ref[i % 2][0]) and np.array_equal(a, ref[i % 2][1]), (i, "stream")
    g = s.graph(w["qn"], w["q"], R, k=K, dist=dist, stop_mass=STOP)
    assert g.graph is not None
    for i, (a, b) in enumerate(batches):
        d, an = g.run(a, b)
        assert np.array_equal(d, ref[i % 2][0]) and np.array_equal(an, ref[i % 2][1]), (i, "graph")
    g.close()


def test_split_mode():
    """Float32 data that is not fp16-exact (storage f32x), thresholds on."""
    w, _, _, _, _ = setup("near")
    x32, q32 = workloads.float32_inputs(w, 7)
    ix = DeviceIndex(x32, w["labels"], w["C"], chunk_rows=512, device="cuda")
    assert ix.storage == "f32x"
    s = Searcher(ix, DeviceRouter(w["layers"], device="cuda"))
    qn, qs = T(w["qn"]), T(q32)
    cls = s.route(qn, R, stop_mass=STOP)
    assert np.array_equal(cls.cpu().numpy(), setup("near")[2])
    ids = np.arange(1, x32.shape[0] + 1)
    d, a = s.search(qn, qs, R, k=K, use_threshold=True, stop_mass=STOP)
    rd, ra = O.search_direct(w["labels"], ids, x32, q32, cls.cpu().numpy(), n_buckets=R, k=K,
                             use_threshold=True)
    assert O.compare_lists(rd, ra, d, a, atol=1e-5, tie=1e-6) == 0
    d2, a2 = s.search(qn, qs, R, k=K, use_threshold=True, classes=cls)
    assert np.array_equal(d, d2) and np.array_equal(a, a2)
    with s.streamed(w["qn"], q32, R, k=K, stop_mass=STOP) as st:
        assert st.split
        for _ in range(2):
            d3, a3 = st.step()
            assert np.array_equal(d3, d) and np.array_equal(a3, a)


def test_learned_index_search_on_frames():
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    w, s, cls, _, _ = setup("skewed")
    nn = NeuralNetwork(input_dim=96, output_dim=w["C"], lr=0.009, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    li = LearnedIndex()
    li.model = nn
    data = pd.DataFrame(np.array(w["xn"]))
    data.index += 1
    data_search = pd.DataFrame(w["x"].astype(np.float16))
    data_search.index += 1
    q16 = w["q"].astype(np.float16)
    labels = np.array(w["labels"])
    args = (data, np.array(w["qn"]), data_search, q16, labels)
    qn, qs = T(w["qn"]), T(w["q"])
    for thr in (False, True):
        d, a = li.search(*args, n_buckets=R, k=K, use_threshold=thr, stop_mass=STOP)
        rd, ra = s.search(qn, qs, R, k=K, use_threshold=thr, dist="f64", stop_mass=STOP)
        assert np.array_equal(d, rd) and np.array_equal(a, ra), thr
    d2, a2 = li.search(*args, n_buckets=R, k=K, use_threshold=True, stop_mass=STOP, min_buckets=R)
    p, pa = li.search(*args, n_buckets=R, k=K, use_threshold=True)
    n, na = li.search(*args, n_buckets=R, k=K, use_threshold=True, stop_mass=None)
    assert np.array_equal(p, n) and np.array_equal(pa, na)
    assert np.array_equal(p, d2) and np.array_equal(pa, a2)       # min_buckets = the cap: off
    assert not np.array_equal(pa, a)
    mean = li.mean_probes(data, np.array(w["qn"]), data_search, labels, R, STOP)
    assert mean == pytest.approx((cls >= 0).sum() / 200.0, abs=1e-12)


@pytest.mark.timeout(300)
def test_exchange_branch_in_a_one_rank_group():
    env = dict(os.environ, LMI_FORCE_EXCHANGE="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               LMI_DIST_TIMEOUT_S="120")
    env.pop("MASTER_PORT", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "adaptive_rccl_worker.py")], env=env,
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "adaptive forced exchange OK" in p.stdout
