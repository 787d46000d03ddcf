"""Filtered search: per-query want words tested inside the scan kernels
(lmi_bucket_topk_tagged: scan3_kernel MODE 4 on the 8-wave ring, scan_kernel
TAG on the general kernel), against the same project's untagged scan over an
index built from the eligible rows alone -- the definition of a filtered list
-- and against numpy.

One seeded fixture per row width: 3 buckets of 2 100 / 37 / 700 rows with
chunk_rows = 1024 (bucket 0: three chunks, the last of 52 rows = one full
32-row block + a 20-row tail), 300 queries x 2 probes with bucket 0 probed by
270 queries in round 0 and by the other 30 in round 1 (300 pairs: two pair
blocks of the 8-wave ring, the second partly live).  Tags: bits 0-2 random
(want 1 keeps ~1/2, 7 ~1/8), bit 31 on exactly 4 rows of bucket 0 (fewer than
k eligible rows there, none elsewhere, and the top bit), bit 30 on every row of
bucket 1, and five exact duplicate rows in bucket 0 with different tags."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li import _lib
from li.index import (DeviceIndex, DeviceRouter, Searcher, bucket_topk, merge_topk,
                      want_words)

pytestmark = pytest.mark.gpu

SIZES = (2100, 37, 700)
N, C, CHUNK, NQ, R = sum(SIZES), 3, 1024, 300, 2
WANTS = (0, 1, 7, 1 << 31, 1 << 30, 5)
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _fixture(d, exact=True):
    rng = np.random.default_rng(4200 + d + (0 if exact else 1))
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    if exact:
        x, q = x.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    tags = rng.integers(0, 8, N).astype(np.uint32)
    tags[labels == 1] |= np.uint32(1 << 30)
    tags[b0[[3, 700, 1400, 2099]]] |= np.uint32(1 << 31)   # first, second and last chunk of bucket 0
    dup = b0[[10, 11, 900, 2060, 2090]]                     # five copies of one row, tags 0..4
    x[dup] = x[dup[0]]
    tags[dup] = (tags[dup] & ~np.uint32(7)) | np.arange(5, dtype=np.uint32)
    classes = np.empty((NQ, R), np.int32)
    i = np.arange(NQ)
    classes[:270, 0], classes[:270, 1] = 0, 1 + i[:270] % 2
    classes[270:, 0], classes[270:, 1] = 1 + i[270:] % 2, 0
    want = np.array(WANTS, np.uint32)[rng.integers(0, len(WANTS), NQ)]
    want[:len(WANTS)] = WANTS                               # every word is drawn
    return dict(x=x, q=q, labels=labels, ids=ids, tags=tags, classes=classes, want=want)


@functools.lru_cache(maxsize=None)
def _tagged(d, exact=True):
    f = _fixture(d, exact)
    ix = DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV,
                     storage="f16" if exact else "f32", tags=f["tags"])
    return Searcher(ix, None)


@functools.lru_cache(maxsize=None)
def _eligible(d, w, exact=True):
    """Searcher over the index built from the rows eligible under `w` alone."""
    f = _fixture(d, exact)
    m = (f["tags"] & np.uint32(w)) == np.uint32(w)
    ix = DeviceIndex(f["x"][m], f["labels"][m], C, ids=f["ids"][m], chunk_rows=CHUNK, device=DEV,
                     storage="f16" if exact else "f32")
    return Searcher(ix, None)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lists(s, f, k, rows=slice(None), want=None):
    """(d [n, R, k] float32, ids [n, R, k] int64 with -1 padding, positions)."""
    _, d, pos, st = s.lists(None, _T(f["q"][rows]), R, k, classes=_T(f["classes"][rows]), want=want)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    d, pos = d.cpu().numpy(), pos.cpu().numpy()
    ids = np.where(pos >= 0, s.index.pos_to_id[np.maximum(pos, 0)], -1)
    return d, ids, pos


def _bitwise(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- 1. lists, a want word per query --------------------------------------------
@pytest.mark.parametrize("d,k,exact", [(768, 10, True), (96, 10, True), (96, 16, True), (200, 10, True),
                                       (200, 16, True), (96, 10, False)])
def test_lists_per_query_want_equal_the_eligible_rows_index(d, k, exact):
    f = _fixture(d, exact)
    got_d, got_ids, _ = _lists(_tagged(d, exact), f, k, want=f["want"])
    for w in WANTS:
        rows = np.flatnonzero(f["want"] == w)
        assert rows.size
        ref_d, ref_ids, _ = _lists(_eligible(d, w, exact), f, k, rows=rows)
        assert _bitwise(got_d[rows], ref_d), (d, k, w)
        assert np.array_equal(got_ids[rows], ref_ids), (d, k, w)
    # (the fixture does what it is there for: short and empty lists, full ones)
    top = f["want"] == 1 << 31
    assert np.isinf(got_d[top]).any() and np.isfinite(got_d[top]).any()
    assert np.isfinite(got_d[f["want"] == 1]).all()


# ---- 2. k_list = 16 at d = 768: the general kernel against the 4-wave ring ---------
def test_lists_k16_at_768_match_the_eligible_rows_index():
    f = _fixture(768)
    got_d, got_ids, _ = _lists(_tagged(768), f, 16, want=f["want"])
    for w in WANTS:
        rows = np.flatnonzero(f["want"] == w)
        ref_d, ref_ids, _ = _lists(_eligible(768, w), f, 16, rows=rows)
        assert O.compare_lists(ref_d, ref_ids, got_d[rows], got_ids[rows]) == 0, w


# ---- 3. want = 0 -----------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(768, 10), (96, 10), (96, 16)])
def test_want_zero_is_the_untagged_scan(d, k):
    f, s = _fixture(d), _tagged(d)
    got_d, _, got_p = _lists(s, f, k, want=0)
    ref_d, _, ref_p = _lists(s, f, k)
    assert _bitwise(got_d, ref_d) and np.array_equal(got_p, ref_p)


# ---- 4. numpy ---------------------------------------------------------------------------
def test_lists_match_numpy_float64():
    f, s = _fixture(768), _tagged(768)
    k = 10
    got_d, _, got_p = _lists(s, f, k, want=f["want"])
    order, off = s.index.layout.order, s.index.layout.bucket_off
    x = f["x"][order].astype(np.float64)
    t = f["tags"][order]
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    qn = f["q"].astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    dist = 1.0 - qn @ xn.T                                     # [NQ, N] by position
    ref_d = np.full((NQ, R, k), np.inf)
    ref_p = np.full((NQ, R, k), -1, np.int64)
    for i in range(NQ):
        w = f["want"][i]
        for r in range(R):
            c = f["classes"][i, r]
            p = np.arange(off[c], off[c + 1])
            p = p[(t[p] & w) == w]
            best = p[np.lexsort((p, dist[i, p]))][:k]
            ref_d[i, r, :best.size], ref_p[i, r, :best.size] = dist[i, best], best
    assert O.compare_lists(ref_d, ref_p, got_d, got_p) == 0


# ---- 5. search, exact semantics, a word per query ---------------------------------------
@pytest.mark.parametrize("d", [768, 96])
def test_search_exact_per_query_want(d):
    f = _fixture(d)
    got = _tagged(d).search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact",
                            want=f["want"])
    for w in WANTS:
        rows = np.flatnonzero(f["want"] == w)
        ref = _eligible(d, w).search(None, _T(f["q"][rows]), R, k=10, classes=_T(f["classes"][rows]),
                                     semantics="exact")
        assert np.array_equal(got[0][rows].view(np.uint64), ref[0].view(np.uint64)), w
        assert np.array_equal(got[1][rows], ref[1]), w


# ---- 6. search, reference semantics, one word for the batch ------------------------------
@functools.lru_cache(maxsize=None)
def _reference_answer(d, w, thr):
    f = _fixture(d)
    return _eligible(d, w).search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), use_threshold=thr)


@pytest.mark.parametrize("thr", [True, False])
@pytest.mark.parametrize("w", [1, 7, 1 << 31])
def test_search_reference_one_want(w, thr):
    f, s = _fixture(768), _tagged(768)
    ref = _reference_answer(768, w, thr)
    for where in ("device", "host"):
        got = s.search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), use_threshold=thr,
                       replay_on=where, want=w)
        assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), (w, thr, where)
        assert np.array_equal(got[1], ref[1]), (w, thr, where)
    # (bit 31: 4 eligible rows in bucket 0 -- the < k quirk -- and none elsewhere)
    assert s.eligible_bucket_size(1 << 31).tolist() == [4, 0, 0]


# ---- 7. stripes ----------------------------------------------------------------------------
def test_striped_shards_merge_to_the_one_gpu_lists():
    f, k, G = _fixture(768), 10, 3
    one_d, _, one_p = _lists(_tagged(768), f, k, want=f["want"])
    q, cls = _T(f["q"]), _T(f["classes"])
    ds, ps = [], []
    for r in range(G):
        sh = DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV,
                         rank=r, world=G, tags=f["tags"])
        assert sh.tags.numel() == sh.n_rows < N
        d, p, st = bucket_topk(sh, q, cls, k, want=want_words(sh, f["want"], NQ, k))
        assert int(st.item()) == 0
        ds.append(d.view(NQ * R, k))
        ps.append(p.view(NQ * R, k))
    md, mp = merge_topk(torch.stack(ds), torch.stack(ps), k)
    torch.cuda.synchronize()
    assert _bitwise(md.cpu().numpy().reshape(NQ, R, k), one_d)
    assert np.array_equal(mp.cpu().numpy().reshape(NQ, R, k), one_p)


# ---- 8. updates carry the tags ----------------------------------------------------------------
def _same_index(a, b, f):
    assert torch.equal(a.corpus, b.corpus) and torch.equal(a.inv_norm, b.inv_norm)
    assert torch.equal(a.tags, b.tags) and np.array_equal(a.tags_by_pos, b.tags_by_pos)
    assert np.array_equal(a.pos_to_id, b.pos_to_id)
    la, lb = _lists(Searcher(a, None), f, 10, want=f["want"]), _lists(Searcher(b, None), f, 10, want=f["want"])
    assert _bitwise(la[0], lb[0]) and np.array_equal(la[2], lb[2])


@pytest.mark.parametrize("inplace", [False, True])
def test_add_remove_relabel_carry_the_tags(inplace):
    f = _fixture(768)
    x, lab, ids, tags = f["x"], f["labels"], f["ids"], f["tags"]
    n0, m = N - 50, 50

    def build(rows, labels=lab, **kw):
        return DeviceIndex(x[rows], labels[rows], C, ids=ids[rows], chunk_rows=CHUNK, device=DEV,
                           tags=tags[rows], **kw)

    kw = dict(capacity=N) if inplace else {}
    base = np.arange(n0)
    added = build(base, **kw).add(x[n0:], lab[n0:], ids=ids[n0:], tags=tags[n0:], inplace=inplace)
    _same_index(added, build(np.arange(N)), f)
    # (new rows default to tag 0)
    zero = build(base, **kw).add(x[n0:], lab[n0:], ids=ids[n0:], inplace=inplace)
    assert np.array_equal(np.sort(zero.tags_by_pos[np.isin(zero.pos_to_id, ids[n0:])]), np.zeros(m, np.uint32))

    gone = np.random.default_rng(5).choice(N, m, replace=False)
    keep = np.setdiff1d(np.arange(N), gone)
    removed = build(np.arange(N), **kw).remove(ids[gone], inplace=inplace)
    _same_index(removed, build(keep), f)

    lab2 = np.random.default_rng(6).permutation(lab)
    relabeled = build(np.arange(N), **kw).relabel(lab2, inplace=inplace)
    _same_index(relabeled, build(np.arange(N), labels=lab2), f)


# ---- 9. refusals, each before any launch ----------------------------------------------------------
def test_refusals_come_before_any_launch():
    f = _fixture(96)
    q, cls = _T(f["q"]), _T(f["classes"])

    def fresh(**kw):
        kw.setdefault("tags", f["tags"])
        return Searcher(DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV, **kw),
                        None)

    def refused(s, how, **kw):
        with pytest.raises(ValueError):
            if how == "lists":
                s.lists(None, q, R, kw.pop("k", 10), classes=cls, **kw)
            else:
                s.search(None, q, R, classes=cls, **kw)
        assert "buf" not in s.index._ws, "a workspace was allocated before the refusal"

    refused(fresh(tags=None), "lists", want=1)                      # an untagged index
    refused(fresh(tags=None), "search", want=1)
    s = fresh()
    refused(s, "lists", want=1, dist="f64")
    refused(s, "search", want=1, dist="f64")
    refused(s, "lists", want=1, k=17)                               # k_list > 16
    refused(s, "search", want=1, k=17, semantics="exact")
    refused(s, "lists", want=np.ones(NQ - 1, np.int64))             # shape
    refused(s, "lists", want=np.ones((NQ, 1), np.int64))
    refused(s, "lists", want=-1)                                    # range
    refused(s, "lists", want=1 << 32)
    refused(s, "lists", want=np.full(NQ, 1 << 32, np.int64))
    refused(s, "lists", want=np.ones(NQ, np.float32))               # not integers
    refused(s, "search", want=f["want"])                            # a word per query under "reference"
    # storage "f32x" (the split mode): float32 values that are not fp16-exact at d_pad 768
    g = _fixture(768, False)
    sx = Searcher(DeviceIndex(g["x"][:300], g["labels"][:300], C, chunk_rows=CHUNK, device=DEV,
                              tags=g["tags"][:300]), None)
    assert sx.index.storage == "f32x"
    with pytest.raises(ValueError):
        sx.lists(None, _T(g["q"]), R, 10, classes=_T(g["classes"]), want=1)
    assert "buf" not in sx.index._ws
    # construction and updates
    with pytest.raises(ValueError):
        fresh(subcluster=True)
    with pytest.raises(ValueError):
        fresh(tags=f["tags"][:-1])
    with pytest.raises(ValueError):
        fresh(tags=None).index.add(f["x"][:2], f["labels"][:2], ids=[1, 2], tags=[1, 2])
    # the index still answers
    d, _, _ = _lists(s, f, 10, want=1)
    assert np.isfinite(d).any()


# ---- 10. the drop-in class --------------------------------------------------------------------------
def test_learned_index_attach_tags_search_want():
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    Cw, w_ = 8, 1
    w = workloads.clustered(n=2000, nq=64, C=Cw, seed=11, label_mode="router")
    rng = np.random.default_rng(12)
    tags = rng.integers(0, 8, 2000).astype(np.uint32)
    nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=Cw, lr=0.009, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    nav, ds = pd.DataFrame(w["xn"]), pd.DataFrame(w["x"])
    nav.index += 1
    ds.index += 1
    li_ = LearnedIndex()
    li_.model = nn
    li_.attach(nav, ds, w["labels"], tags=tags)
    got = li_.search(nav, w["qn"], ds, w["q"], w["labels"], n_buckets=3, k=10, use_threshold=True, want=w_)
    # the Searcher's filtered answer, and the answer over the eligible objects alone
    s = li_._get_searcher(li_._index)
    mine = s.search(_T(w["qn"]), _T(w["q"]), 3, k=10, use_threshold=True, want=w_)
    m = (tags & w_) == w_
    ids = np.arange(1, 2001, dtype=np.int64)
    ref = Searcher(DeviceIndex(w["x"][m], w["labels"][m], s.index.n_buckets, ids=ids[m], device=DEV),
                   DeviceRouter(w["layers"], device=DEV)).search(_T(w["qn"]), _T(w["q"]), 3, k=10,
                                                                 use_threshold=True)
    for a in (mine, ref):
        assert np.array_equal(got[0].view(np.uint64), a[0].view(np.uint64))
        assert np.array_equal(got[1], a[1])
