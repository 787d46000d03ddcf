"""Re-ranking 16-entry lists of the 8-bit storage from kept fp16 rows: the i8
ring's 16-entry lists (scan3_i8_kernel<16, TAG>), the re-rank kernel alone
(lmi_rerank_f64) and Searcher / LearnedIndex with `rerank`.

No tolerance anywhere.  The 8-bit lists are compared bit for bit with the numpy
restatement of tests/i8_cases.py and with scan_i8_kernel; the re-ranked float64
distances with the bits lmi_bucket_topk_f64 gives the same (query, row), read
from range_search(dist="f64", radius=2.0) of an fp16 index over the same rows
(every row of a probed bucket, each with those bits).

Where a test compares a re-ranked answer with the fp16 index's own float64
answer, it does so on the pairs whose numpy float64 top-10 lies inside the
restated 8-bit top-16 (elsewhere the two differ by design), and numpy alone
asserts the fixture's conditions first: how many pairs those are, and that no
two candidates of a pair lie within 1e-10 of each other (numpy's and the
device's float64 distances differ by a few ulp of 1, which must not reorder)."""
import functools

import numpy as np
import pytest
import torch

import i8_cases as I8
import test_gpu_i8_ring as RING
import test_gpu_range as RANGE
import workloads
from li import _lib
from li.index import (DeviceIndex, DeviceRouter, RowSource, Searcher, bucket_topk, i8_lists16, rerank_f64,
                      scan_family)

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 2
_T = RING._T


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same64(got, ref, what, sel=None):
    gd, gp = np.asarray(got[0]), np.asarray(got[1])
    rd, rp = np.asarray(ref[0]), np.asarray(ref[1])
    if sel is not None:
        gd, gp, rd, rp = gd[sel], gp[sel], rd[sel], rp[sel]
    assert gd.dtype == np.float64 and rd.dtype == np.float64
    assert np.array_equal(gp, rp), what
    assert np.array_equal(_bits64(gd), _bits64(rd)), what


# ---- numpy alone ----------------------------------------------------------------------------------
def numpy_d64(x_sorted, q):
    """float64 [nq, n]: 1 - cosine of every query and every row, numpy alone."""
    x = np.asarray(x_sorted, np.float64)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    qn = np.asarray(q, np.float64)
    qn = qn / np.linalg.norm(qn, axis=1, keepdims=True)
    return 1.0 - qn @ xn.T


def containment(Dnp, d8, bucket_off, classes, eligible=None, k=10, k2=16):
    """Per pair: (numpy's float64 top-k of the bucket lies inside the restated
    8-bit top-k2, the bucket has >= k2 candidates, the smallest float64 gap
    between two of the pair's k2 candidates)."""
    classes = np.asarray(classes)
    nq, Rr = classes.shape
    p2 = I8.bucket_lists(d8, bucket_off, classes, k2, eligible=eligible)[1]
    inside = np.ones((nq, Rr), bool)
    big = np.zeros((nq, Rr), bool)
    gap = np.full((nq, Rr), np.inf)
    C = len(bucket_off) - 1
    for i in range(nq):
        for r in range(Rr):
            c = int(classes[i, r])
            if not 0 <= c < C:
                continue
            p = np.arange(bucket_off[c], bucket_off[c + 1])
            if eligible is not None:
                p = p[eligible[i, p]]
            best = p[np.lexsort((p, Dnp[i, p]))][:k]
            cand = p2[i, r][p2[i, r] >= 0]
            inside[i, r] = np.isin(best, cand).all()
            big[i, r] = p.size >= k2
            if cand.size > 1:
                gap[i, r] = np.diff(np.sort(Dnp[i, cand])).min()
    return inside, big, gap


def expected_rerank(D, pos_in, k, n_rows):
    """The k smallest of every pair's live candidates by (D, position), padded
    (+inf, -1); a position twice is listed twice; positions >= n_rows are skipped."""
    nq, Rr, _ = pos_in.shape
    out_d = np.full((nq, Rr, k), np.inf, np.float64)
    out_p = np.full((nq, Rr, k), -1, np.int32)
    for i in range(nq):
        for r in range(Rr):
            p = pos_in[i, r]
            p = p[(p >= 0) & (p < n_rows)]
            dd = D[i, p]
            assert not np.isnan(dd).any(), "a candidate outside the query's probed buckets"
            o = np.lexsort((p, dd))[:k]
            out_d[i, r, :o.size], out_p[i, r, :o.size] = dd[o], p[o]
    return out_d, out_p


# ---- the device's float64 bits of every (query, probed row) ----------------------------------------
def d64_table(s16, q, classes):
    """float64 [nq, n] by position, NaN off the query's probed buckets: the
    distances of range_search(dist="f64", radius=2.0) of the fp16 index --
    lmi_bucket_topk_f64's bits for that (query, row)."""
    ix = s16.index
    cls = np.where((classes >= 0) & (classes < ix.n_buckets), classes, -1).astype(np.int32)
    lims, dists, anns = s16.range_search(None, _T(q), cls.shape[1], 2.0, classes=_T(cls), dist="f64")
    assert int(lims[-1]) == int(ix.bucket_size[cls[cls >= 0]].sum())     # every row of every probed bucket
    inv = np.full(int(ix.pos_to_id.max()) + 1, -1, np.int64)
    inv[ix.pos_to_id] = np.arange(ix.pos_to_id.size)
    D = np.full((cls.shape[0], ix.n_total), np.nan, np.float64)
    D[np.repeat(np.arange(cls.shape[0]), np.diff(lims)), inv[anns.astype(np.int64)]] = dists
    D.setflags(write=False)
    return D


def _lists64(s, q, classes, k, **kw):
    _, d, pos, st = s.lists(None, _T(q), classes.shape[1], k, classes=_T(classes), dist="f64", **kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    return d.cpu().numpy(), pos.cpu().numpy()


# ---- 1. the ring at KL = 16 ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 16])
@pytest.mark.parametrize("d", [768, 750])
def test_ring_16_entry_lists_plain_and_tagged(d, k):
    f, s = RING._fixture(d), RING._searcher(d)
    # the 16-entry lists are the plan of a thread that asked for them (the re-rank's scan does);
    # every other call keeps the plan it had
    assert scan_family(s.index, k) == "general" and scan_family(s.index, k, tagged=True) == "general"
    assert scan_family(s.index, k, lists16=True) == "ring8-i8"
    assert scan_family(s.index, k, tagged=True, lists16=True) == "ring8-i8"
    with i8_lists16():
        assert scan_family(s.index, k) == "ring8-i8" and scan_family(s.index, k, tagged=True) == "ring8-i8"
        got_d, got_p = RING._both(s, f["q"], f["classes"], k, RING._restated(d))
        cls = f["classes"]
        assert np.isfinite(got_d[cls == 8]).all() and (got_p[cls == 7] == -1).all()
        assert np.isfinite(got_d[cls == 0][:, 0]).all() and np.isinf(got_d[cls == 0][:, 1:]).all()
        RING._both(s, f["q"], f["classes"], k, RING._restated(d), want=f["want"], avoid=f["avoid"])
    assert scan_family(s.index, k) == "general"
    # bucket_topk(..., lists16=True), the re-rank's own call, against the default kernel's lists
    a = bucket_topk(s.index, RING._T(f["q"]), RING._T(f["classes"]), k, lists16=True)
    b = bucket_topk(s.index, RING._T(f["q"]), RING._T(f["classes"]), k)
    torch.cuda.synchronize()
    RING._same((a[0].cpu().numpy(), a[1].cpu().numpy()), (b[0].cpu().numpy(), b[1].cpu().numpy()),
               "lists16 vs default")


def test_ring_16_one_workgroup():
    d, k = 768, 16
    f, s = RING._fixture(d), RING._searcher(d)
    ref = I8.bucket_lists(RING._restated(d), s.index.layout.bucket_off, f["classes"], k)
    lib = _lib.load()
    with i8_lists16():
        assert scan_family(s.index, k) == "ring8-i8"
        prev = lib.lmi_scan_set_workgroups(1)
        try:
            got = RING._lists(s, f["q"], f["classes"], k)
        finally:
            assert lib.lmi_scan_set_workgroups(prev) == 1
        RING._same(got, ref, "one workgroup vs restatement")
        RING._same(got, RING._lists_general(s, f["q"], f["classes"], k), "one workgroup vs general i8 kernel")


def test_ring_16_more_than_16_tied_rows_across_chunks():
    d, nq = 768, 257
    sizes = (3000, 40, 3, 70, 0)
    rng = np.random.default_rng(RING.SEED + 16)
    n = sum(sizes)
    x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    # 20 copies of one row: chunks 0, 1, 3, 5, 8, 11 of the 12, up to six in one chunk
    at = [10, 11, 12, 200, 255, 256, 300, 800, 801, 1290, 1300, 1310, 1320, 1330, 1340, 2100, 2101, 2900, 2990, 2999]
    dup = b0[at]
    x[dup] = x[dup[0]]
    q[5] = x[dup[0]]
    classes = np.empty((nq, R), np.int32)
    classes[:, 0], classes[:, 1] = 0, 1 + np.arange(nq) % 4
    ix = DeviceIndex(x, labels, len(sizes), chunk_rows=256, device=DEV, storage="i8")
    assert ix.max_chunks == 12
    s = Searcher(ix, None)
    dist = RING._restate(x, q, ix)[2]
    dup_pos = np.sort(np.flatnonzero(np.isin(ix.layout.order, dup)))
    assert dup_pos.size == 20 and np.unique(dup_pos // 256).size == 6
    assert np.unique(RING._bits(dist[5, dup_pos])).size == 1 and (dist[5, dup_pos] <= dist[5, :3000].min()).all()
    for k in (11, 16):
        with i8_lists16():
            got_d, got_p = RING._both(s, q, classes, k, dist)
        # the tie straddles the list's bound and the chunk merge: the k lowest positions win
        assert np.array_equal(got_p[5, 0], dup_pos[:k]) and np.unique(RING._bits(got_d[5, 0])).size == 1


# ---- 2. the re-rank kernel alone -------------------------------------------------------------------
ROWS2 = np.r_[0:24, 270:278]          # 32 of the range fixture's queries: bucket 0 in round 0 and in round 1
PATTERNS = 7


def _hand_made(f, ix, k_in, rng):
    """pos int32 [32, R, k_in] inside each pair's probed bucket; pair (i, r) takes pattern (i R + r) % 7:
    0 all live; 1 empty entries in the middle; 2 empty entries at the end; 3 one live entry (fewer than
    k), in the middle; 4 a whole empty list; 5 one row listed three times; 6 (on bucket 0) the fixture's
    five equal rows, highest position first."""
    off = ix.layout.bucket_off
    cls = f["classes"][ROWS2]
    b0 = np.flatnonzero(f["labels"] == 0)
    dup_pos = np.sort(np.flatnonzero(np.isin(ix.layout.order, b0[[10, 11, 900, 2060, 2090]])))
    pos = np.full((cls.shape[0], R, k_in), -1, np.int32)
    pat = np.empty((cls.shape[0], R), np.int32)
    for i in range(cls.shape[0]):
        for r in range(R):
            c = int(cls[i, r])
            p = rng.choice(np.arange(off[c], off[c + 1]), k_in, replace=False).astype(np.int32)
            t = pat[i, r] = (i * R + r) % PATTERNS
            if t == 1:
                p[1::3] = -1
            elif t == 2:
                p[k_in - k_in // 3:] = -1
            elif t == 3:
                keep = p[k_in // 2]
                p[:] = -1
                p[k_in // 2] = keep
            elif t == 4:
                p[:] = -1
            elif t == 5:
                p[-1] = p[k_in // 2] = p[0]
            elif t == 6 and c == 0:
                m = min(5, k_in)
                p[:m] = dup_pos[::-1][:m]
            pos[i, r] = p
    return pos, pat, cls, dup_pos


@pytest.mark.parametrize("d", [768, 200])
def test_rerank_kernel_on_hand_made_lists(d):
    f, s16 = RANGE._fixture(d), RANGE._tagged(d)
    ix = s16.index
    assert ix.storage == "f16" and tuple(ix.bucket_size) == RANGE.SIZES
    q = f["q"][ROWS2]
    D = d64_table(s16, q, f["classes"][ROWS2])
    rng = np.random.default_rng(5100 + d)
    for k_in in (1, 11, 16):
        pos, pat, cls, dup_pos = _hand_made(f, ix, k_in, rng)
        assert set(pat.ravel()) == set(range(PATTERNS)) and ((pat == 6) & (cls == 0)).any()
        i6 = int(np.argwhere((pat == 6) & (cls == 0))[0][0])
        assert np.unique(_bits64(D[i6, dup_pos])).size == 1           # five rows, one distance
        for k in sorted({1, min(10, k_in), k_in}):
            gd, gp, st = rerank_f64(ix, _T(q), _T(pos), k)
            torch.cuda.synchronize()
            assert int(st.item()) == 0
            got = gd.cpu().numpy(), gp.cpu().numpy()
            _same64(got, expected_rerank(D, pos, k, ix.n_rows), (d, k_in, k))
            if k_in >= 5 and k >= 5:
                j = np.argwhere((pat == 6) & (cls == 0))[0]
                assert np.array_equal(np.sort(got[1][j[0], j[1]][np.isin(got[1][j[0], j[1]], dup_pos)]),
                                      got[1][j[0], j[1]][np.isin(got[1][j[0], j[1]], dup_pos)])
            if k_in == 16 and k == 16:
                j = np.argwhere(pat == 5)[0]
                assert (got[1][j[0], j[1]] == pos[j[0], j[1], 0]).sum() == 3     # listed three times


def test_rerank_kernel_out_of_range_position_sets_the_status_and_is_skipped():
    d, k_in, k = 768, 16, 10
    f, s16 = RANGE._fixture(d), RANGE._tagged(d)
    ix = s16.index
    q = f["q"][ROWS2]
    D = d64_table(s16, q, f["classes"][ROWS2])
    pos, pat, _, _ = _hand_made(f, ix, k_in, np.random.default_rng(5200))
    assert pat[0, 0] == 0 and pos[0, 0, 3] >= 0
    pos[0, 0, 3] = ix.n_rows                                        # one past the last row
    gd, gp, st = rerank_f64(ix, _T(q), _T(pos), k)
    torch.cuda.synchronize()
    assert int(st.item()) & _lib.LMI_STATUS_INTERNAL
    _same64((gd.cpu().numpy(), gp.cpu().numpy()), expected_rerank(D, pos, k, ix.n_rows), "skipped")
    assert np.isfinite(gd.cpu().numpy()[0, 0]).all() and ix.n_rows not in gp.cpu().numpy()


# ---- 3. end to end, lists ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_of_indexes(d):
    f = RING._fixture(d)
    kw = dict(ids=f["ids"], chunk_rows=RING.CHUNK, device=DEV, tags=f["tags"])
    s8 = Searcher(DeviceIndex(f["x"], f["labels"], RING.C, storage="i8", keep_rows=True, **kw), None)
    s16 = Searcher(DeviceIndex(f["x"], f["labels"], RING.C, storage="f16", **kw), None)
    return s8, s16


@pytest.mark.parametrize("d", [768, 750])
def test_lists_reranked_from_16_entry_lists(d):
    f = RING._fixture(d)
    s8, s16 = _pair_of_indexes(d)
    ix = s8.index
    assert ix.storage == "i8" and ix.rows16 is not None and tuple(ix.rows16.shape) == (RING.N, 768)
    assert ix.rows16.dtype == torch.float16 and torch.equal(ix.rows16, s16.index.corpus)
    off, cls = ix.layout.bucket_off, f["classes"]
    d8 = RING._restated(d)
    # the fixture's conditions, from numpy
    inside, big, gap = containment(numpy_d64(f["x"][ix.layout.order], f["q"]), d8, off, cls)
    print(f"d={d}: pairs on buckets of >= 16 rows {big.sum()}, top-10 inside the i8 top-16 {inside[big].sum()}, "
          f"smallest gap {gap.min():.3g}")
    assert big.sum() >= 1000 and inside[big].sum() >= 0.95 * big.sum()
    assert gap.min() > 1e-10
    got = _lists64(s8, f["q"], cls, 10, rerank=16)
    # the re-rank of the restated 8-bit top-16, with the fp16 index's own float64 bits
    p16 = I8.bucket_lists(d8, off, cls, 16)[1]
    _same64(got, expected_rerank(d64_table(s16, f["q"], cls), p16, 10, ix.n_rows), "rerank of the restated top-16")
    # where the float64 top-10 is among the 16 candidates: the fp16 index's float64 lists
    _same64(got, _lists64(s16, f["q"], cls, 10), "the fp16 index's float64 lists", sel=inside)
    for sel in (cls == 7, cls >= RING.C):
        assert sel.any() and np.isinf(got[0][sel]).all() and (got[1][sel] == -1).all()


# ---- 4. end to end, answers --------------------------------------------------------------------------
RA = 3          # probes of the answers' fixture
WANT, AVOID = 1, 4


@functools.lru_cache(maxsize=None)
def _answers():
    Cw = 8
    w = workloads.clustered(n=2000, nq=64, C=Cw, seed=11, label_mode="router")
    x = w["x"].astype(np.float16).astype(np.float32)
    q = w["q"].astype(np.float16).astype(np.float32)
    n = x.shape[0]
    ids = np.arange(1, n + 1, dtype=np.int64)
    tags = np.random.default_rng(5400).integers(0, 8, n).astype(np.uint32)
    router = DeviceRouter(w["layers"], device=DEV)
    s16 = Searcher(DeviceIndex(x, w["labels"], Cw, ids=ids, device=DEV, storage="f16", tags=tags), router)
    s8 = Searcher(DeviceIndex(x, w["labels"], Cw, ids=ids, device=DEV, storage="i8", keep_rows=True, tags=tags),
                  router)
    m = ((tags & np.uint32(WANT)) == WANT) & ((tags & np.uint32(AVOID)) == 0)
    se = Searcher(DeviceIndex(x[m], w["labels"][m], Cw, ids=ids[m], device=DEV, storage="f16"), router)
    classes = s16.route(_T(w["qn"]), RA).cpu().numpy()
    ix = s8.index
    xs = x[ix.layout.order]
    d8 = RING._restate(x, q, ix)[2]
    Dnp = numpy_d64(xs, q)
    elig = np.broadcast_to(m[ix.layout.order], (q.shape[0], n))
    return dict(w=w, x=x, q=q, tags=tags, s8=s8, s16=s16, se=se, classes=classes, d8=d8, Dnp=Dnp, elig=elig)


def _search(s, a, **kw):
    return s.search(_T(a["w"]["qn"]), _T(a["q"]), RA, k=10, use_threshold=True, dist="f64", **kw)


def _same_answer(got, ref, what):
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(_bits64(got[0]), _bits64(ref[0])), what


# (this fixture's router is nearly flat: two picks hold 0.264 .. 0.278 of the mass, so at 0.272 about
# half of the queries stop after two probes -- asserted below)
@pytest.mark.parametrize("stop_mass", [None, 0.272])
@pytest.mark.parametrize("semantics", ["reference", "exact"])
def test_search_reranked_equals_the_fp16_float64_answer(semantics, stop_mass):
    a = _answers()
    s8, s16 = a["s8"], a["s16"]
    assert scan_family(s8.index, 16, lists16=True) == "ring8-i8"
    inside, big, gap = containment(a["Dnp"], a["d8"], s8.index.layout.bucket_off, a["classes"])
    assert big.sum() >= 150 and inside.all() and gap.min() > 1e-10      # every pair: the answers must be equal
    kw = dict(semantics=semantics)
    if stop_mass is not None:
        kw.update(stop_mass=stop_mass, min_probes=1)
        cls = s16.route(_T(a["w"]["qn"]), RA, stop_mass=stop_mass, min_probes=1).cpu().numpy()
        assert (cls[:, 1:] < 0).any() and (cls[:, -1] >= 0).any()     # some queries stop early, some do not
    _same_answer(_search(s8, a, rerank=16, **kw), _search(s16, a, **kw), (semantics, stop_mass))


def test_learned_index_attach_keep_rows_rerank():
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    a = _answers()
    w = a["w"]
    inside, _, gap = containment(a["Dnp"], a["d8"], a["s8"].index.layout.bucket_off, a["classes"])
    assert inside.all() and gap.min() > 1e-10
    nav, ds = pd.DataFrame(w["xn"]), pd.DataFrame(a["x"].astype(np.float16))
    nav.index += 1
    ds.index += 1

    def learned():
        nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=8, lr=0.009, model_type="MLP")
        lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for m, (wt, b) in zip(lin, w["layers"]):
                m.weight.copy_(torch.from_numpy(wt))
                m.bias.copy_(torch.from_numpy(b))
        li_ = LearnedIndex()
        li_.model = nn
        return li_
    l8, l16 = learned(), learned()
    i8 = l8.attach(nav, ds, w["labels"], storage="i8", keep_rows=True, rerank=16)
    i16 = l16.attach(nav, ds, w["labels"])
    assert i8.storage == "i8" and i8.rows16 is not None and i16.storage == "f16"
    args = (nav, w["qn"], ds, a["q"].astype(np.float16), w["labels"])
    for sem in ("reference", "exact"):
        _same_answer(l8.search(*args, n_buckets=RA, k=10, use_threshold=True, semantics=sem),
                     l16.search(*args, n_buckets=RA, k=10, use_threshold=True, semantics=sem), sem)
    # without `rerank` the same attach answers float32 lists, as it did
    l8b = learned()
    l8b.attach(nav, ds, w["labels"], storage="i8", keep_rows=True)
    plain = learned()
    plain.attach(nav, ds, w["labels"], storage="i8")
    _same_answer(l8b.search(*args, n_buckets=RA, k=10, use_threshold=True),
                 plain.search(*args, n_buckets=RA, k=10, use_threshold=True), "no rerank")


@pytest.mark.parametrize("semantics", ["reference", "exact"])
def test_tagged_search_reranked_equals_the_index_of_the_eligible_rows(semantics):
    a = _answers()
    s8, se = a["s8"], a["se"]
    assert scan_family(s8.index, 16, tagged=True, lists16=True) == "ring8-i8"
    inside, big, gap = containment(a["Dnp"], a["d8"], s8.index.layout.bucket_off, a["classes"], eligible=a["elig"])
    assert big.sum() >= 100 and inside.all() and gap.min() > 1e-10
    cls = _T(a["classes"])
    got = _search(s8, a, rerank=16, semantics=semantics, want=WANT, avoid=AVOID, classes=cls)
    _same_answer(got, _search(se, a, semantics=semantics, classes=cls), semantics)


# ---- 5. sharing and refusals ---------------------------------------------------------------------------
def test_quantized_keep_rows_shares_the_corpus():
    _, s16 = _pair_of_indexes(768)
    ix = s16.index
    q8 = ix.quantized(keep_rows=True)
    assert q8.storage == "i8" and q8.rows16.data_ptr() == ix.corpus.data_ptr() and q8.rows16 is ix.corpus
    assert ix.quantized().rows16 is None
    f = RING._fixture(768)
    s8, _ = _pair_of_indexes(768)
    assert torch.equal(q8.corpus, s8.index.corpus) and torch.equal(q8.inv_norm, s8.index.inv_norm)
    _same64(_lists64(Searcher(q8, None), f["q"], f["classes"], 10, rerank=16),
            _lists64(s8, f["q"], f["classes"], 10, rerank=16), "quantized(keep_rows=True) vs built with keep_rows")
    f32 = DeviceIndex(f["x"], f["labels"], RING.C, device=DEV, storage="f32")
    with pytest.raises(ValueError, match="keep_rows"):
        f32.quantized(keep_rows=True)


def test_refusals_before_any_launch():
    f = RING._fixture(768)
    s8, s16 = _pair_of_indexes(768)
    plain8 = RING._searcher(768)
    # (queries of None: a call that got as far as touching them would raise something else)
    for s, kw, what in ((plain8, dict(dist="f64", rerank=16), "keeps no fp16 rows"),
                        (s16, dict(dist="f64", rerank=16), "storage 'i8'"),
                        (s8, dict(dist="f64", rerank=10), "must lie in"),
                        (s8, dict(dist="f64", rerank=5), "must lie in"),
                        (s8, dict(dist="f64", rerank=17), "must lie in"),
                        (s8, dict(dist="f32", rerank=16), "float64"),
                        (s8, dict(rerank=16), "float64"),
                        (s8, dict(dist="f64"), "not offered on storage 'i8'")):
        with pytest.raises(ValueError, match=what):
            s.lists(None, None, R, 10, classes=None, **kw)
        with pytest.raises(ValueError, match=what):
            s.search(None, None, R, k=10, **kw)
    q, cls = _T(f["q"]), _T(f["classes"])
    for call in (lambda: s8.streamed(q, q, R), lambda: s8.graph(q, q, R),
                 lambda: s8.range_search(None, q, R, 0.5, classes=cls)):
        with pytest.raises(ValueError, match="i8"):
            call()
    with pytest.raises(ValueError, match="fp16-representable"):
        DeviceIndex(f["x"] * np.float32(1.0001), f["labels"], RING.C, device=DEV, storage="i8", keep_rows=True)
    with pytest.raises(ValueError, match="keep_rows"):
        DeviceIndex(f["x"], f["labels"], RING.C, device=DEV, storage="f16", keep_rows=True)
    src = RowSource(RING.N, 768, lambda a, b: torch.from_numpy(f["x"][a:b]).to(DEV).half())
    with pytest.raises(ValueError, match="RowSource"):
        DeviceIndex(src, f["labels"], RING.C, device=DEV, storage="i8", keep_rows=True)


@pytest.mark.parametrize("k", [10, 16])
def test_calls_without_rerank_are_what_they_were(k):
    f = RING._fixture(768)
    s8, _ = _pair_of_indexes(768)
    plain8 = RING._searcher(768)
    RING._same(RING._lists(s8, f["q"], f["classes"], k), RING._lists(plain8, f["q"], f["classes"], k), "plain")
    RING._same(RING._lists(s8, f["q"], f["classes"], k, want=f["want"], avoid=f["avoid"]),
               RING._lists(plain8, f["q"], f["classes"], k, want=f["want"], avoid=f["avoid"]), "tagged")
    a = s8.search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact")
    b = plain8.search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact")
    assert np.array_equal(a[1], b[1]) and np.array_equal(_bits64(a[0]), _bits64(b[0]))
