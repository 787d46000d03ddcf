"""Search by squared Euclidean distance and by inner product (metric="l2" /
"ip": lmi_bucket_topk_metric) against a plain float64 numpy reference per
(query, probed bucket): d64 by the definition, ordered by (distance, position).

Workload: test_gpu_scan_widths.py's shape (3000 rows, 8 skewed buckets, chunks
of 256 rows, 96 queries, 3 probes) with every row scaled by a seeded factor in
[0.5, 4] and every query by one in [0.5, 2], rounded to fp16 -- without the
norm spread all three metrics rank alike and the cosine kernel would pass.
Widths: 768 (the 8-wave ring for k <= 10, the general kernel's 16-entry lists
above), 96 (one full 64-wide block + the trailing half block), 30 (d % 4 != 0,
d_pad 32: the trailing block alone, scalar word loads).

bound = 2 * (a proven bound on |d32 - d64|), DESIGN.md §3 "K2 by another
metric": with eps = refine_eps(d_pad, f16math) >= the accumulator's error
relative to |q||y|, and u = 2^-24, ip: eps |q||y|; l2: 2 eps |q||y| + 4u (qq +
yy) (the roundings of qq, yy, their sum and the fma).  Every returned distance
is held to bound / 2 of its own pair; the gap rule of a list takes the bound
at the largest |y| of the corpus, an upper bound of every pair's.
SEEDS: picked on the CPU so that both reference-only conditions hold for every
case (96: seed 996 put 10.4 % of the k = 16 l2 lists inside the bound)."""
import functools

import numpy as np
import pytest
import torch

import workloads
from li import _lib
from li.Baseline import Baseline
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_topk, refine_eps
from li.layout import BucketLayout

pytestmark = pytest.mark.gpu

N, NQ, C, R, CHUNK = 3000, 96, 8, 3, 256
SEEDS = {768: 1668, 96: 1996, 30: 930}
F16, F32 = _lib.LMI_Q_F16, _lib.LMI_Q_F32
CLASSES = (("f16", F16, 1), ("f16", F16, 10), ("f16", F16, 12), ("f16", F16, 16), ("f16", F32, 10),
           ("f32", F32, 10))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def _dist64(metric, q, x):
    """[nq, n] float64 distances by the definition."""
    acc = q @ x.T
    if metric == "ip":
        return -acc
    if metric == "l2":
        return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * acc
    return 1.0 - acc / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :])


@functools.lru_cache(maxsize=None)
def _workload(d):
    """Rows in bucket-sorted (position) order, float64; queries; probed classes."""
    import lmi_oracle as O
    w = workloads.clustered(n=N, d=d, nq=NQ, C=C, seed=SEEDS[d], label_mode="skewed")
    rng = np.random.Generator(np.random.PCG64(SEEDS[d] + 17))
    x = (w["x"] * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float16).astype(np.float32)
    q = (w["q"] * rng.uniform(0.5, 2.0, (NQ, 1))).astype(np.float16).astype(np.float32)
    classes = np.ascontiguousarray(O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))[:, :R]).astype(np.int32)
    lay = BucketLayout.from_labels(w["labels"], C)
    return dict(w, x=x, q=q, classes=classes, xs=x[lay.order].astype(np.float64), off=lay.bucket_off)


@functools.lru_cache(maxsize=None)
def _reference(d, metric, depth=17):
    """(d64 of every (query, position) [NQ, N]; ref_d, ref_p [NQ, R, depth], (inf, -1) padded)."""
    w = _workload(d)
    D = _dist64(metric, w["q"].astype(np.float64), w["xs"])
    rd = np.full((NQ, R, depth), np.inf)
    rp = np.full((NQ, R, depth), -1, np.int64)
    for i in range(NQ):
        for r in range(R):
            a, b = w["off"][w["classes"][i, r]], w["off"][w["classes"][i, r] + 1]
            o = np.argsort(D[i, a:b], kind="stable")[:depth]  # (positions ascend: ties by position)
            rd[i, r, :o.size], rp[i, r, :o.size] = D[i, a:b][o], a + o
    return D, rd, rp


def _err(d, metric, f16math, qn, yn):
    """The proven bound on |d32 - d64| of pairs with norms qn, yn (broadcast)."""
    u, eps = 2.0 ** -24, refine_eps((d + 31) // 32 * 32, f16math)
    return eps * qn * yn if metric == "ip" else 2 * eps * qn * yn + 4 * u * (qn * qn + yn * yn)


def _norms(w, xs=None):
    return np.linalg.norm(w["q"].astype(np.float64), axis=1), np.linalg.norm(w["xs"] if xs is None else xs, axis=1)


@functools.lru_cache(maxsize=None)
def _index(d, metric, storage):
    w = _workload(d)
    ix = DeviceIndex(w["x"], w["labels"], C, storage=storage, chunk_rows=CHUNK, device="cuda", metric=metric)
    assert ix.metric == metric and ix.storage == storage
    return ix


def _check(D, rd, rp, got_d, got_p, k, err, allowed, cap=None):
    """Lists [NQ, L, k] of (float32 distance, position; -1 = none) against the
    reference's [NQ, L, k + 1].  err(qn, yn): _err of the case; a list's bound
    is 2 err at the corpus' largest |y| (an upper bound of every pair's), each
    distance is held to its own pair's err.  allowed [NQ, L, N]: the rows a
    list may name.  `cap`: the reference-only condition, first."""
    w_qn, w_yn = err.norms
    bound = 2.0 * err(w_qn, w_yn.max())[:, None, None]
    with np.errstate(invalid="ignore"):  # (inf - inf between empty slots)
        gaps = np.diff(rd[..., :k + 1], axis=-1)
    gaps[np.isnan(gaps)] = np.inf
    clear = np.all(gaps > bound, axis=-1)
    if cap is not None:
        assert 1.0 - clear.mean() <= cap, f"the strict-id rule exempts {1 - clear.mean():.1%} (cap {cap:.0%})"
    got_p = got_p.astype(np.int64)
    assert got_d.dtype == np.float32 and got_d.shape == rd[..., :k].shape
    assert np.array_equal(got_p < 0, rp[..., :k] < 0) and np.all(np.isinf(got_d[got_p < 0]))
    live, pc = got_p >= 0, np.maximum(got_p, 0)
    assert np.all(np.take_along_axis(allowed, pc, axis=2)[live]), "a row from outside the probed buckets"
    srt = np.sort(np.where(live, got_p, -1 - np.arange(k)), axis=-1)
    assert np.all(srt[..., 1:] != srt[..., :-1]), "a list names a row twice"
    own = np.take_along_axis(np.broadcast_to(D[:, None, :], allowed.shape), pc, axis=2)  # d64 of the returned rows
    pair = err(w_qn[:, None, None], w_yn[pc])                                            # = its bound / 2
    assert np.all(np.abs(got_d - own)[live] <= pair[live]), "a distance off its d64 by more than its pair's bound / 2"
    assert np.all(np.abs(own - rd[..., :k])[live] <= np.broadcast_to(bound, own.shape)[live]), \
        "ids differ beyond the bound"
    same = np.all(got_p == rp[..., :k], axis=-1)
    assert np.all(same[clear]), f"ids differ in {int((~same & clear).sum())} clear lists"


def _errfn(d, metric, f16math, w, xs=None):
    fn = functools.partial(_err, d, metric, f16math)
    fn.norms = _norms(w, xs)
    return fn


def _bucket_mask(w, classes):
    """[NQ, L, N]: position p lies in the bucket classes[i, l] names."""
    pos = np.arange(N)[None, None, :]
    return (pos >= w["off"][classes][..., None]) & (pos < w["off"][classes + 1][..., None])


def _lists(got):
    d, p, st = got
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    return d.cpu().numpy(), p.cpu().numpy()


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"{c[0]}-q{'f16' if c[1] == F16 else 'f32'}-k{c[2]}")
@pytest.mark.parametrize("d", [768, 96, 30])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_lists_match_float64(metric, d, cls):
    storage, qmode, k = cls
    w, f16math = _workload(d), cls[:2] == ("f16", F16)
    D, rd, rp = _reference(d, metric)
    # from the reference alone: the metric's lists are not the cosine's
    _, _, cp = _reference(d, "cosine")
    full = rp[..., 9] >= 0
    differ = np.any(np.sort(rp[..., :10], -1) != np.sort(cp[..., :10], -1), axis=-1)
    assert differ[full].mean() >= 0.90, f"only {differ[full].mean():.1%} of the top-10 lists differ from cosine"
    got = bucket_topk(_index(d, metric, storage), T(w["q"]), T(w["classes"]), k, qmode=qmode)
    _check(D, rd, rp, *_lists(got), k, _errfn(d, metric, f16math, w), _bucket_mask(w, w["classes"]),
           cap=0.10 if f16math else 0.50)


def test_ring_ties_across_a_chunk_boundary():
    """d = 768, l2, k = 10: 20 equal rows, 6 at the end of a bucket's first
    chunk and 14 at the start of its second; for the query equal to them all 20
    tie at the smallest distance, and positions decide: the lane bound keeps
    ties, the chunk merge orders them."""
    w = _workload(768)
    c = int(np.argmax(np.diff(w["off"])))
    a = int(w["off"][c]) + CHUNK - 6
    assert w["off"][c + 1] - w["off"][c] >= 2 * CHUNK
    lay = BucketLayout.from_labels(w["labels"], C)
    x, q = w["x"].copy(), w["q"].copy()
    x[lay.order[a:a + 20]] = q[0]
    ix = DeviceIndex(x, w["labels"], C, storage="f16", chunk_rows=CHUNK, device="cuda", metric="l2")
    cls = np.full((NQ, 1), c, np.int32)
    d, p = _lists(bucket_topk(ix, T(q), T(cls), 10, qmode=F16))
    assert p[0, 0].tolist() == list(range(a, a + 10)) and len(set(d[0, 0].tolist())) == 1
    xs = x[lay.order].astype(np.float64)
    D = _dist64("l2", q.astype(np.float64), xs)
    rows = slice(int(w["off"][c]), int(w["off"][c + 1]))
    o = np.argsort(D[:, rows], axis=1, kind="stable")[:, :11]
    rd = np.take_along_axis(D[:, rows], o, 1)[:, None, :]
    _check(D, rd, (o + rows.start)[:, None, :], d, p, 10, _errfn(768, "l2", True, w, xs), _bucket_mask(w, cls))


@pytest.mark.parametrize("d", [768, 96])
def test_phases_compose(d):
    w = _workload(d)
    ix, q, cls = _index(d, "l2", "f16"), T(w["q"]), T(w["classes"])
    d0, p0, st0 = bucket_topk(ix, q, cls, 10, qmode=F16)
    ws = torch.empty_like(ix._ws["buf"])
    out = (torch.empty_like(d0), torch.empty_like(p0), torch.zeros_like(st0))
    for ph in (_lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_MERGE):
        bucket_topk(ix, q, cls, 10, qmode=F16, out=out, ws=ws, phases=ph)
    assert torch.equal(out[0], d0) and torch.equal(out[1], p0) and int(out[2].item()) == 0 == int(st0.item())


def _merged(D, rp, depth=11):
    """The (distance, position) top of the union of each query's probed lists, [NQ, 1, depth]."""
    md, mp = np.full((NQ, 1, depth), np.inf), np.full((NQ, 1, depth), -1, np.int64)
    for i in range(NQ):
        cand = np.unique(rp[i][rp[i] >= 0])
        o = cand[np.lexsort((cand, D[i, cand]))][:depth]
        md[i, 0, :o.size], mp[i, 0, :o.size] = D[i, o], o
    return md, mp


def _answer(ix, dists, anns):
    """search()'s (float64 distances, ids; (10000, 0) = none) as (float32, positions; (inf, -1))."""
    inv = np.full(N + 1, -1, np.int64)
    inv[ix.pos_to_id] = np.arange(N)
    p = inv[anns.astype(np.int64)]
    return np.where(p < 0, np.inf, dists).astype(np.float32)[:, None, :], p[:, None, :]


@pytest.mark.parametrize("d", [768, 96])
def test_search_exact_end_to_end(d):
    """Searcher.search(semantics="exact"), l2: the merged top-10 of the three
    probed buckets, under the lists' tie rule; LearnedIndex.attach(metric=)
    answers the same through the public class."""
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    w = _workload(d)
    ix = _index(d, "l2", "f16")
    s = Searcher(ix, DeviceRouter(w["layers"], device="cuda"))
    dists, anns = s.search(T(w["qn"]), T(w["q"]), R, k=10, semantics="exact")
    D, _, rp = _reference(d, "l2")
    md, mp = _merged(D, rp)
    _check(D, md, mp, *_answer(ix, dists, anns), 10, _errfn(d, "l2", True, w),
           _bucket_mask(w, w["classes"]).any(axis=1, keepdims=True))
    # the reference replay on such lists: the device replay is the host replay
    ref = [s.search(T(w["qn"]), T(w["q"]), R, k=10, use_threshold=True, replay_on=on) for on in ("device", "host")]
    assert np.array_equal(ref[0][0], ref[1][0]) and np.array_equal(ref[0][1], ref[1][1])
    if d != 96:
        return
    nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=C, lr=0.009, model_type="MLP")
    with torch.no_grad():
        for m, (wt, b) in zip([m for m in nn.model.layers if isinstance(m, torch.nn.Linear)], w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    nav, ds = pd.DataFrame(w["xn"]), pd.DataFrame(w["x"].astype(np.float16))
    nav.index += 1
    ds.index += 1
    li_ = LearnedIndex()
    li_.model = nn
    assert li_.attach(nav, ds, w["labels"], metric="l2").metric == "l2"
    got = li_.search(nav, w["qn"], ds, w["q"], w["labels"], n_buckets=R, k=10, semantics="exact")
    assert np.array_equal(got[0], dists) and np.array_equal(got[1], anns)
    with pytest.raises(ValueError, match="metric 'l2'"):
        li_.range_search(nav, w["qn"], ds, w["q"], w["labels"], 1.0, n_buckets=R)


def test_stop_mass_drops_probes_of_a_metric_index():
    w = _workload(96)
    s = Searcher(_index(96, "ip", "f16"), DeviceRouter(w["layers"], device="cuda"))
    # (this router's top probabilities lie in 0.132 .. 0.143: 0.14 stops some queries after one probe, the rest after two)
    cls, d, p, st = s.lists(T(w["qn"]), T(w["q"]), R, 10, stop_mass=0.14)
    full = bucket_topk(s.index, T(w["q"]), T(w["classes"]), 10, qmode=F16)
    cls = cls.cpu().numpy()
    assert int(st.item()) == 0 and (cls < 0).any() and np.array_equal(cls[cls >= 0], w["classes"][cls >= 0])
    keep = torch.from_numpy(cls >= 0).cuda()
    assert torch.equal(d[keep], full[0][keep]) and torch.equal(p[keep], full[1][keep])
    assert bool(torch.isinf(d[~keep]).all()) and bool((p[~keep] == -1).all())


def test_baseline_ip_is_the_brute_force():
    w = _workload(96)
    dists, nns, _ = Baseline(metric="ip").search(w["q"], w["x"], k=10)
    x64 = w["x"].astype(np.float64)
    D = _dist64("ip", w["q"].astype(np.float64), x64)
    o = np.argsort(D, axis=1, kind="stable")[:, :11]
    assert dists.dtype == np.float32
    _check(D, np.take_along_axis(D, o, 1)[:, None, :], o[:, None, :], dists[:, None, :], (nns - 1)[:, None, :], 10,
           _errfn(96, "ip", True, w, x64), np.ones((NQ, 1, N), bool))


def test_cosine_argument_changes_nothing():
    w = _workload(96)
    args = (w["x"], w["labels"], C)
    a = bucket_topk(DeviceIndex(*args, chunk_rows=CHUNK, device="cuda"), T(w["q"]), T(w["classes"]), 10)
    b = bucket_topk(DeviceIndex(*args, chunk_rows=CHUNK, device="cuda", metric="cosine"), T(w["q"]),
                    T(w["classes"]), 10)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
