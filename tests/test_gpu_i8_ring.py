"""The 8-wave ring of the 8-bit storage (scan3_i8_kernel: storage "i8", d_pad ==
768, k <= 10) on the smallest shapes at which a ring can go wrong.  Every list
is compared twice, bit for bit in distances and positions over every pair:
against the numpy restatement of tests/i8_cases.py and against the general i8
kernel (scan_i8_kernel) run in the same process under LMI_SCAN_V1=1.  The
integer sums are exact, so there is no tolerance anywhere.

The common fixture: chunk_rows = 64, R = 2, nine buckets of
(1, 31, 32, 33, 64, 65, 97, 0, 300) rows -- a one-row chunk, a block one short,
exactly one block, one row over, exactly one chunk, a one-row tail chunk, a
chunk plus a partial block, an empty bucket, five chunks -- and 564 queries
whose `classes` are written out so that the buckets receive
(1, 31, 32, 33, 255, 256, 257, 4, 258) probing pairs: one live lane, a partial
wave, one full wave, a wave plus one, a tile one short, a full tile, a tile plus
a one-pair tile, a few probes of the empty bucket, and on the 300-row bucket a
full tile plus a two-pair tile; one class lies outside [0, C)."""
import functools
import os

import numpy as np
import pytest
import torch

import i8_cases as I8
import workloads
from li import _lib
from li.index import DeviceIndex, DeviceRouter, Searcher, scan_family
from test_gpu_i8 import PAIRS as I8_PAIRS

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 64, 65, 97, 0, 300)
PROBES = (1, 31, 32, 33, 255, 256, 257, 4, 258)
N, C, CHUNK, R = sum(SIZES), len(SIZES), 64, 2
NQ = (sum(PROBES) + 1) // R
# the i8 test's predicates and a wanted bit no row carries
PAIRS = tuple(I8_PAIRS) + ((1 << 28, 0),)
SEED = 7681
DEV = "cuda"


def _ok(tags, w, a):
    tags = np.asarray(tags, np.uint32)
    return ((tags & np.uint32(w)) == np.uint32(w)) & ((tags & np.uint32(a)) == 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _classes():
    """[NQ, 2]: the pairs' buckets bucket after bucket, then the class outside
    [0, C); query i probes entries i and NQ + i (never one bucket twice)."""
    flat = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(PROBES)] + [np.array([C + 3], np.int32)])
    assert flat.size == NQ * R
    cls = np.stack([flat[:NQ], flat[NQ:]], axis=1)
    assert (cls[:, 0] != cls[:, 1]).all()
    return np.ascontiguousarray(cls)


@functools.lru_cache(maxsize=None)
def _fixture(d):
    rng = np.random.default_rng(SEED + d)
    x = rng.standard_normal((N, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    tags = rng.integers(0, 8, N).astype(np.uint32)
    tags[labels == 6] |= np.uint32(1 << 30)                    # avoid bit 30: nothing left in bucket 6
    b8 = np.flatnonzero(labels == 8)
    tags[b8[[3, 70, 140, 299]]] |= np.uint32(1 << 31)          # want bit 31: four rows, all in bucket 8
    classes = _classes()
    pair = rng.integers(0, len(PAIRS), NQ)
    pair[:len(PAIRS)] = np.arange(len(PAIRS))
    # every predicate on the buckets where it is short or empty
    on8 = np.flatnonzero(classes[:, 1] == 8)
    on6 = np.flatnonzero(classes[:, 1] == 6)
    pair[on8[:4]] = [PAIRS.index((1 << 31, 1)), PAIRS.index((1 << 28, 0)), 0, PAIRS.index((0, 1 << 30))]
    pair[on6[:3]] = [PAIRS.index((0, 1 << 30)), PAIRS.index((1 << 31, 1)), 0]
    pw = np.array(PAIRS, np.int64)[pair]
    f = dict(x=x, q=q, labels=labels, ids=ids, tags=tags, classes=classes, pair=pair, want=pw[:, 0].copy(),
             avoid=pw[:, 1].copy())
    # the planted properties, on the CPU
    got = np.bincount(classes[(classes >= 0) & (classes < C)], minlength=C)
    assert tuple(got) == PROBES and ((classes < 0) | (classes >= C)).sum() == 1
    assert np.array_equal(np.bincount(labels, minlength=C), SIZES)
    return f


@functools.lru_cache(maxsize=None)
def _searcher(d):
    f = _fixture(d)
    return Searcher(DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV, storage="i8",
                                tags=f["tags"]), None)


def _restate(x, q, ix):
    cx, invx = I8.quantize(x[ix.layout.order])
    cq, invq = I8.quantize(q)
    dist = I8.distances(cq, invq, cx, invx)
    dist.setflags(write=False)
    return cq, cx, dist


@functools.lru_cache(maxsize=None)
def _restated(d):
    """The restatement of width d, computed once and left unchanged."""
    f = _fixture(d)
    return _restate(f["x"], f["q"], _searcher(d).index)[2]


def _lists(s, q, classes, k, **kw):
    _, d, pos, st = s.lists(None, _T(q), R, k, classes=_T(classes), **kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    return d.cpu().numpy(), pos.cpu().numpy()


def _lists_general(s, q, classes, k, **kw):
    """The same call on scan_i8_kernel (LMI_SCAN_V1=1), the switch then put back."""
    lib = _lib.load()
    saved = os.environ.get("LMI_SCAN_V1")
    os.environ["LMI_SCAN_V1"] = "1"
    lib.lmi_config_reload()
    try:
        assert scan_family(s.index, k, tagged=bool(kw)) == "general"
        return _lists(s, q, classes, k, **kw)
    finally:
        os.environ.pop("LMI_SCAN_V1", None)
        if saved is not None:
            os.environ["LMI_SCAN_V1"] = saved
        lib.lmi_config_reload()


def _same(got, ref, what):
    assert np.array_equal(_bits(got[0]), _bits(ref[0])), what
    assert np.array_equal(got[1], ref[1]), what


def _both(s, q, classes, k, dist, **kw):
    """The ring's lists, checked against the restatement and the general kernel."""
    tagged = bool(kw)
    assert scan_family(s.index, k, tagged=tagged) == "ring8-i8"
    got = _lists(s, q, classes, k, **kw)
    elig = None
    if tagged:
        t = s.index.tags.cpu().numpy().view(np.uint32)
        elig = np.stack([_ok(t, kw["want"][i], kw["avoid"][i]) for i in range(q.shape[0])])
    ref = I8.bucket_lists(dist, s.index.layout.bucket_off, classes, k, eligible=elig)
    _same(got, ref, "ring vs restatement")
    _same(got, _lists_general(s, q, classes, k, **kw), "ring vs general i8 kernel")
    assert scan_family(s.index, k, tagged=tagged) == "ring8-i8"
    return got


# ---- 1. shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [768, 750])
def test_shapes(d, k):
    f, s = _fixture(d), _searcher(d)
    assert s.index.storage == "i8" and s.index.d_pad == 768
    if d == 750:
        assert not s.index.corpus[:, d:].any().item()              # zero pad columns
    got_d, got_p = _both(s, f["q"], f["classes"], k, _restated(d))
    cls = f["classes"]
    # padded lists: the empty bucket, the class outside [0, C), the one-row bucket past its row
    for sel in (cls == 7, cls >= C):
        assert sel.any() and np.isinf(got_d[sel]).all() and (got_p[sel] == -1).all()
    one = cls == 0
    assert np.isfinite(got_d[one][:, 0]).all() and np.isinf(got_d[one][:, 1:]).all() and (got_p[one][:, 1:] == -1).all()
    assert np.isfinite(got_d[cls == 8]).all()


# ---- 2. pruning and cross-chunk ties -----------------------------------------------------------
def test_pruning_and_cross_chunk_ties():
    d, k, nq = 768, 10, 257
    sizes = (6000, 40, 3, 70, 0)
    rng = np.random.default_rng(SEED + 2)
    n = sum(sizes)
    x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    dup = b0[[10, 700, 2500, 4100, 5990]]                       # chunks 0, 1, 4, 8, 11 of the 12
    x[dup] = x[dup[0]]
    q[5] = x[dup[0]]
    classes = np.empty((nq, R), np.int32)
    classes[:, 0], classes[:, 1] = 0, 1 + np.arange(nq) % 4
    ix = DeviceIndex(x, labels, len(sizes), chunk_rows=512, device=DEV, storage="i8")
    assert ix.max_chunks == 12
    s = Searcher(ix, None)
    dist = _restate(x, q, ix)[2]
    dup_pos = np.sort(np.flatnonzero(np.isin(ix.layout.order, dup)))
    assert np.unique(dup_pos // 512).size == 5                  # (bucket 0 is first: positions = rows of it)
    ref_d, ref_p = I8.bucket_lists(dist, ix.layout.bucket_off, classes, k)
    assert np.isin(ref_p[5, 0], dup_pos).sum() >= 2, "no list holds two duplicates"
    got_d, got_p = _both(s, q, classes, k, dist)
    at = np.flatnonzero(np.isin(got_p[5, 0], dup_pos))
    assert at.size == 5 and np.array_equal(at, np.arange(5))
    assert np.unique(_bits(got_d[5, 0, at])).size == 1 and np.array_equal(got_p[5, 0, at], dup_pos)


# ---- 3. accumulator extremes -------------------------------------------------------------------
def test_accumulator_extremes():
    d, k = 768, 10
    sizes = (45, 20)
    rng = np.random.default_rng(SEED + 3)
    n = sum(sizes)
    x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(2), sizes)).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    ones, neg, zero = b0[[2, 33, 44]]
    x[ones], x[neg], x[zero] = 1.0, -1.0, 0.0
    q = rng.standard_normal((40, d)).astype(np.float16).astype(np.float32)
    q[0], q[1] = 1.0, -1.0
    classes = np.empty((40, R), np.int32)
    classes[:, 0], classes[:, 1] = 0, 1
    ix = DeviceIndex(x, labels, 2, chunk_rows=CHUNK, device=DEV, storage="i8")
    s = Searcher(ix, None)
    cq, cx, dist = _restate(x, q, ix)
    acc = cq.astype(np.int64) @ cx.astype(np.int64).T
    pos = {name: int(np.flatnonzero(ix.layout.order == r)[0]) for name, r in (("ones", ones), ("neg", neg), ("zero", zero))}
    top = 768 * 127 * 127
    assert top == 12387072 and acc.max() == top and acc.min() == -top
    assert acc[0, pos["ones"]] == top and acc[0, pos["neg"]] == -top and acc[1, pos["neg"]] == top
    assert dist[0, pos["zero"]] == 1.0 and dist[1, pos["zero"]] == 1.0
    got_d, got_p = _both(s, q, classes, k, dist)
    assert got_p[0, 0, 0] == pos["ones"] and got_p[1, 0, 0] == pos["neg"]
    assert _bits(got_d[0, 0, 0]) == _bits(dist[0, pos["ones"]])
    # the most negative sum is the largest distance of the bucket: listed by neither query, present in k = all
    assert pos["neg"] not in got_p[0, 0] and pos["ones"] not in got_p[1, 0]


# ---- 4. tagged ---------------------------------------------------------------------------------
def test_tagged():
    d, k = 768, 10
    f, s = _fixture(d), _searcher(d)
    t = f["tags"][s.index.layout.order]
    off = s.index.layout.bucket_off
    # the planted properties: (0, 0) takes every row; bit 31 leaves 1..9 rows of bucket 8 and none
    # elsewhere; bit 28 none anywhere; avoiding bit 30 none of bucket 6
    assert _ok(t, 0, 0).all() and not _ok(t, 1 << 28, 0).any()
    assert 1 <= _ok(t[off[8]:off[9]], 1 << 31, 1).sum() <= 9 and not _ok(t[:off[8]], 1 << 31, 0).any()
    assert not _ok(t[off[6]:off[7]], 0, 1 << 30).any()
    used = {(int(f["want"][i]), int(f["avoid"][i]), int(f["classes"][i, 1])) for i in range(NQ)}
    assert {(1 << 31, 1, 8), (1 << 28, 0, 8), (0, 1 << 30, 6), (0, 0, 8)} <= used
    assert set(f["pair"]) == set(range(len(PAIRS)))
    assert scan_family(s.index, 10, tagged=True) == "ring8-i8"
    got_d, got_p = _both(s, f["q"], f["classes"], k, _restated(d), want=f["want"], avoid=f["avoid"])
    i = int(np.flatnonzero((f["want"] == 1 << 31) & (f["classes"][:, 1] == 8))[0])
    n31 = int(_ok(t[off[8]:off[9]], 1 << 31, 1).sum())
    assert np.isfinite(got_d[i, 1, :n31]).all() and np.isinf(got_d[i, 1, n31:]).all() and (got_p[i, 1, n31:] == -1).all()
    i = int(np.flatnonzero((f["avoid"] == 1 << 30) & (f["classes"][:, 1] == 6))[0])
    assert np.isinf(got_d[i, 1]).all() and (got_p[i, 1] == -1).all()


# ---- 5. one workgroup --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [768, 750])
def test_one_workgroup(d, k):
    f, s = _fixture(d), _searcher(d)
    assert scan_family(s.index, k) == "ring8-i8"
    ref = I8.bucket_lists(_restated(d), s.index.layout.bucket_off, f["classes"], k)
    lib = _lib.load()
    prev = lib.lmi_scan_set_workgroups(1)
    try:
        got = _lists(s, f["q"], f["classes"], k)
    finally:
        assert lib.lmi_scan_set_workgroups(prev) == 1
    _same(got, ref, "one workgroup vs restatement")
    _same(got, _lists(s, f["q"], f["classes"], k), "one workgroup vs the whole grid")
    _same(got, _lists_general(s, f["q"], f["classes"], k), "one workgroup vs general i8 kernel")


# ---- 6. through the public interface -----------------------------------------------------------
def test_search_exact_equals_the_merged_restated_lists():
    d = 768
    f, s = _fixture(d), _searcher(d)
    ix = s.index
    assert scan_family(ix, 10) == "ring8-i8"
    lists = I8.bucket_lists(_restated(d), ix.layout.bucket_off, f["classes"], 10)
    want = I8.merged_topk(*lists, 10, ix.pos_to_id)
    got = s.search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact")
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))


def test_learned_index_attach_storage_i8_answers_through_the_ring():
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    Cw = 8
    w = workloads.clustered(n=2000, nq=64, C=Cw, seed=11, label_mode="router")
    assert w["x"].shape[1] == 768
    nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=Cw, lr=0.009, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    nav, ds = pd.DataFrame(w["xn"]), pd.DataFrame(w["x"].astype(np.float16))
    nav.index += 1
    ds.index += 1
    li_ = LearnedIndex()
    li_.model = nn
    index = li_.attach(nav, ds, w["labels"], storage="i8")
    assert index.storage == "i8" and scan_family(index, 10) == "ring8-i8"
    got = li_.search(nav, w["qn"], ds, w["q"], w["labels"], n_buckets=3, k=10, use_threshold=True)
    # the restated lists of the router's own classes, replayed
    s = Searcher(index, DeviceRouter(w["layers"], device=DEV))
    classes, d_l, p_l, st = s.lists(_T(w["qn"]), _T(w["q"]), 3, 10)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    classes = classes.cpu().numpy()
    dist = _restate(w["x"], w["q"], index)[2]
    ref = I8.bucket_lists(dist, index.layout.bucket_off, classes, 10)
    _same((d_l.cpu().numpy(), p_l.cpu().numpy()), ref, "attach: ring vs restatement")
    from li.index import replay
    want = replay(classes, ref[0], ref[1], k_round=10, k_final=10, bucket_size=index.bucket_size,
                  pos_to_id=index.pos_to_id, use_threshold=True)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
