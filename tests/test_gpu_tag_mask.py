"""Filtered search with all-of and none-of bits, tag edits in place and deletes
by tombstone: a row answers a query iff (tag & want) == want and
(tag & avoid) == 0, one test (tag & mask) == value inside the scan kernels
(lmi_bucket_topk_masked: scan3_kernel MODE 4 on the 8-wave ring, scan_kernel
TAG on the general kernel; lmi_bucket_range_masked: range_scan_kernel), and
DeviceIndex.edit_tags / set_tags / ids_with (lmi_index_edit_tags).  The
reference is this project's own untagged scan over an index built from the
eligible rows alone -- the definition of a filtered answer -- and numpy.

One seeded fixture per row width: 3 buckets of 2 100 / 37 / 700 rows with
chunk_rows = 1024 (bucket 0: three chunks, the last of 52 rows = one full
32-row block + a 20-row tail), 300 queries x 2 probes with bucket 0 probed by
270 queries in round 0 and by the other 30 in round 1 (300 pairs: two pair
blocks of the 8-wave ring, the second partly live).  Tags: bits 0-2 random,
bit 30 on every row of bucket 1, bit 31 on exactly 4 rows of bucket 0 (its
first, second and last chunk), and five exact duplicate rows in bucket 0 with
tags 0..4.  Every query draws one (want, avoid) pair of PAIRS."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li.index import DeviceIndex, DeviceRouter, Searcher

pytestmark = pytest.mark.gpu

SIZES = (2100, 37, 700)
N, C, CHUNK, NQ, R = sum(SIZES), 3, 1024, 300, 2
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 2), (0, 7), (1 << 31, 1), (0, 1 << 30), (4, 3))
TOMB = 1 << 29
SEED = 5302   # (chosen so that test_the_fixture_does_its_job holds at every width)
DEV = "cuda"


def _ok(tags, w, a):
    """The predicate, restated: every wanted bit and no avoided one."""
    tags = np.asarray(tags, np.uint32)
    return ((tags & np.uint32(w)) == np.uint32(w)) & ((tags & np.uint32(a)) == 0)


@functools.lru_cache(maxsize=None)
def _fixture(d, exact=True):
    rng = np.random.default_rng(SEED + d + (0 if exact else 1))
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    if exact:
        x, q = x.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    tags = rng.integers(0, 8, N).astype(np.uint32)
    tags[labels == 1] |= np.uint32(1 << 30)
    top = b0[[3, 700, 1400, 2099]]                          # first, second and last chunk of bucket 0
    tags[top] |= np.uint32(1 << 31)
    dup = b0[[10, 11, 900, 2060, 2090]]                     # five copies of one row, tags 0..4
    x[dup] = x[dup[0]]
    tags[dup] = (tags[dup] & ~np.uint32(7)) | np.arange(5, dtype=np.uint32)
    classes = np.empty((NQ, R), np.int32)
    i = np.arange(NQ)
    classes[:270, 0], classes[:270, 1] = 0, 1 + i[:270] % 2
    classes[270:, 0], classes[270:, 1] = 1 + i[270:] % 2, 0
    pair = rng.integers(0, len(PAIRS), NQ)
    pair[:len(PAIRS)] = np.arange(len(PAIRS))               # every pair is drawn
    pw = np.array(PAIRS, np.int64)[pair]
    return dict(x=x, q=q, labels=labels, ids=ids, tags=tags, classes=classes, pair=pair,
                want=pw[:, 0].copy(), avoid=pw[:, 1].copy(), top=top, dup=dup)


def test_the_fixture_does_its_job():
    for d, exact in ((768, True), (96, True), (200, True), (96, False)):
        f = _fixture(d, exact)
        assert sorted(set(f["pair"].tolist())) == list(range(len(PAIRS)))
        t, lab = f["tags"], f["labels"]
        assert not _ok(t[lab == 1], 0, 1 << 30).any()                   # bucket 1 empty
        assert _ok(t[lab != 1], 0, 1 << 30).all()
        n31 = int(_ok(t[lab == 0], 1 << 31, 1).sum())
        assert 1 <= n31 < 10 and not _ok(t[lab != 0], 1 << 31, 1).any()  # fewer than k in bucket 0, not none
        kept = _ok(t[f["dup"]], 0, 1)
        assert kept.any() and not kept.all()                            # the duplicate run is split


def _build(f, rows=slice(None), exact=True, tags="own", **kw):
    t = f["tags"][rows] if isinstance(tags, str) else tags
    return DeviceIndex(f["x"][rows], f["labels"][rows], C, ids=f["ids"][rows], chunk_rows=CHUNK, device=DEV,
                       storage="f16" if exact else "f32", tags=t, **kw)


@functools.lru_cache(maxsize=None)
def _tagged(d, exact=True):
    return Searcher(_build(_fixture(d, exact), exact=exact), None)


@functools.lru_cache(maxsize=None)
def _eligible(d, w, a, exact=True, tagged=False):
    """Searcher over the index built from the rows eligible under (w, a) alone
    (tagged: with their tag words, for calls that must run the tagged kernels)."""
    f = _fixture(d, exact)
    return Searcher(_build(f, _ok(f["tags"], w, a), exact, tags="own" if tagged else None), None)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lists(s, f, k, rows=slice(None), **kw):
    """(d [n, R, k] float32, ids [n, R, k] int64 with -1 padding, positions)."""
    _, d, pos, st = s.lists(None, _T(f["q"][rows]), R, k, classes=_T(f["classes"][rows]), **kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    d, pos = d.cpu().numpy(), pos.cpu().numpy()
    ids = np.where(pos >= 0, s.index.pos_to_id[np.maximum(pos, 0)], -1)
    return d, ids, pos


def _bitwise(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _same_answer(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def _pairs_rows(f):
    for p, (w, a) in enumerate(PAIRS):
        rows = np.flatnonzero(f["pair"] == p)
        assert rows.size
        yield w, a, rows


# ---- 1. lists against the eligible-rows index -------------------------------------------
@pytest.mark.parametrize("d,k,exact", [(768, 10, True), (96, 10, True), (96, 16, True), (200, 10, True),
                                       (200, 16, True), (96, 10, False)])
def test_lists_per_query_pairs_equal_the_eligible_rows_index(d, k, exact):
    f = _fixture(d, exact)
    got_d, got_ids, _ = _lists(_tagged(d, exact), f, k, want=f["want"], avoid=f["avoid"])
    for w, a, rows in _pairs_rows(f):
        ref_d, ref_ids, _ = _lists(_eligible(d, w, a, exact), f, k, rows=rows)
        assert _bitwise(got_d[rows], ref_d), (d, k, w, a)
        assert np.array_equal(got_ids[rows], ref_ids), (d, k, w, a)
    # (short, empty and full lists are all there)
    r31 = f["pair"] == PAIRS.index((1 << 31, 1))
    assert np.isinf(got_d[r31]).any() and np.isfinite(got_d[r31]).any()
    r30 = np.flatnonzero(f["pair"] == PAIRS.index((0, 1 << 30)))
    assert np.isinf(got_d[r30][f["classes"][r30] == 1]).all()
    r01 = np.flatnonzero(f["pair"] == PAIRS.index((0, 1)))
    assert np.isfinite(got_d[r01][f["classes"][r01] != 1]).all()


def test_lists_k16_at_768_match_the_eligible_rows_index():
    """(k_list = 16 at d = 768: the general kernel against the 4-wave ring, two
    kernel families, so lists are compared as the oracle compares them)"""
    f = _fixture(768)
    got_d, got_ids, _ = _lists(_tagged(768), f, 16, want=f["want"], avoid=f["avoid"])
    for w, a, rows in _pairs_rows(f):
        ref_d, ref_ids, _ = _lists(_eligible(768, w, a), f, 16, rows=rows)
        assert O.compare_lists(ref_d, ref_ids, got_d[rows], got_ids[rows]) == 0, (w, a)


# ---- 2. avoid = 0 is the want-only call ---------------------------------------------------
@pytest.mark.parametrize("d", [768, 96])
def test_avoid_zero_is_the_want_only_call(d):
    f, s = _fixture(d), _tagged(d)
    ref_d, _, ref_p = _lists(s, f, 10, want=f["want"])
    for avoid in (0, np.zeros(NQ, np.int64)):
        got_d, _, got_p = _lists(s, f, 10, want=f["want"], avoid=avoid)
        assert _bitwise(got_d, ref_d) and np.array_equal(got_p, ref_p)


# ---- 3. numpy -------------------------------------------------------------------------------
def test_lists_match_numpy_float64():
    f, s = _fixture(768), _tagged(768)
    k = 10
    got_d, _, got_p = _lists(s, f, k, want=f["want"], avoid=f["avoid"])
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
        for r in range(R):
            c = f["classes"][i, r]
            p = np.arange(off[c], off[c + 1])
            p = p[_ok(t[p], f["want"][i], f["avoid"][i])]
            best = p[np.lexsort((p, dist[i, p]))][:k]
            ref_d[i, r, :best.size], ref_p[i, r, :best.size] = dist[i, best], best
    assert O.compare_lists(ref_d, ref_p, got_d, got_p) == 0


# ---- 4. Searcher.search ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 96])
def test_search_exact_per_query_pairs(d):
    f = _fixture(d)
    got = _tagged(d).search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact",
                            want=f["want"], avoid=f["avoid"])
    for w, a, rows in _pairs_rows(f):
        ref = _eligible(d, w, a).search(None, _T(f["q"][rows]), R, k=10, classes=_T(f["classes"][rows]),
                                        semantics="exact")
        assert _same_answer((got[0][rows], got[1][rows]), ref), (w, a)


@pytest.mark.parametrize("thr", [True, False])
@pytest.mark.parametrize("w,a", [(1, 2), (0, 1 << 30), (1 << 31, 1)])
def test_search_reference_one_pair(w, a, thr):
    f, s = _fixture(768), _tagged(768)
    ref = _eligible(768, w, a).search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), use_threshold=thr)
    kw = dict(avoid=a) if w == 0 else dict(want=w, avoid=a)     # (avoid alone means want = 0)
    got = s.search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), use_threshold=thr, **kw)
    assert _same_answer(got, ref), (w, a, thr)
    lab_by_pos = f["labels"][s.index.layout.order]
    assert s.eligible_bucket_size(w, a).tolist() == \
        [int(_ok(s.index.tags_by_pos[lab_by_pos == c], w, a).sum()) for c in range(C)]


# ---- 5. range search ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _radius(d):
    """Each query's 10th unfiltered distance."""
    f = _fixture(d)
    got = _tagged(d).search(None, _T(f["q"]), R, k=10, classes=_T(f["classes"]), semantics="exact")
    return got[0][:, 9].astype(np.float64)


@pytest.mark.parametrize("d,dist", [(768, "f32"), (768, "f64"), (96, "f32"), (96, "f64")])
def test_range_search_per_query_pairs(d, dist):
    """(float32 at d = 768: a tagged call runs the general kernel's collect form
    and an untagged index the 8-wave ring's, two kernel families whose float32
    distances differ in the last bits, at a radius that is itself a distance.
    There the eligible-rows index keeps its rows' tag words and is searched with
    want = 0: the same rows, no row left to filter, the same kernel family.)"""
    f, s, radius = _fixture(d), _tagged(d), _radius(d)
    same_family = d == 768 and dist == "f32"

    def run(searcher, rows=slice(None), **kw):
        return searcher.range_search(None, _T(f["q"][rows]), R, radius[rows], classes=_T(f["classes"][rows]),
                                     dist=dist, **kw)

    lims, dists, anns = run(s, want=f["want"], avoid=f["avoid"])
    n = np.diff(lims)
    for w, a, rows in _pairs_rows(f):
        rl, rd, ra = run(_eligible(d, w, a, True, same_family), rows, **(dict(want=0) if same_family else {}))
        assert np.array_equal(n[rows], np.diff(rl)), (d, dist, w, a)
        sel = np.concatenate([np.arange(lims[i], lims[i + 1]) for i in rows] + [np.zeros(0, np.int64)])
        assert np.array_equal(anns[sel], ra), (d, dist, w, a)
        assert np.array_equal(dists[sel].view(np.uint64), rd.view(np.uint64)), (d, dist, w, a)
    assert n[f["pair"] == 0].min() >= 9 and n[f["pair"] == PAIRS.index((1 << 31, 1))].max() <= 4


# ---- 6. edits in place ----------------------------------------------------------------------
def _edit_case(f):
    """ids to edit (first and last row of bucket 0, a row of its 20-row tail,
    every row of the 37-row bucket, one of the duplicates), their set / clear
    words and the tag array after the edit (input order)."""
    rng = np.random.default_rng(77)
    lab = f["labels"]
    b0, b1 = np.flatnonzero(lab == 0), np.flatnonzero(lab == 1)
    rows = np.concatenate([b0[[0, 2099, 2085]], b1, f["dup"][2:3]])
    rows = rows[rng.permutation(rows.size)]
    st = rng.integers(0, 8, rows.size).astype(np.uint32)
    st[rng.random(rows.size) < 0.3] |= np.uint32(1 << 28)
    cl = rng.integers(0, 8, rows.size).astype(np.uint32)
    in_b1 = lab[rows] == 1
    st[in_b1], cl[in_b1] = 0, 1 | (1 << 30)                  # bucket 1 loses bit 0 (no row left under want = 1) and bit 30
    after = f["tags"].copy()
    after[rows] = (after[rows] & ~cl) | st
    return rows, st, cl, after


def test_edit_tags_equals_a_fresh_build_and_drops_the_cached_counts():
    f = _fixture(768)
    rows, st, cl, after = _edit_case(f)
    ix = _build(f)
    s = Searcher(ix, None)
    q, cls = _T(f["q"]), _T(f["classes"])
    before = ix.tags.clone()

    def ref_search(tags):
        return Searcher(_build(f, tags=tags), None).search(None, q, R, k=10, classes=cls, want=1)

    assert _same_answer(s.search(None, q, R, k=10, classes=cls, want=1), ref_search(f["tags"]))
    n1_before = s.eligible_bucket_size(1).tolist()
    v0 = ix.tags_version
    ix.edit_tags(f["ids"][rows], set_bits=st, clear_bits=cl)
    assert ix.tags_version == v0 + 1 and not ix.consumed
    fresh = _build(f, tags=after)
    assert torch.equal(ix.tags, fresh.tags) and not torch.equal(ix.tags, before)
    assert ix.tags_by_pos.dtype == np.uint32 and np.array_equal(ix.tags_by_pos, fresh.tags_by_pos)
    a = _lists(s, f, 10, want=f["want"], avoid=f["avoid"])
    b = _lists(Searcher(fresh, None), f, 10, want=f["want"], avoid=f["avoid"])
    assert _bitwise(a[0], b[0]) and np.array_equal(a[2], b[2])
    # the same Searcher after the edit: its cached eligible counts are gone
    assert _same_answer(s.search(None, q, R, k=10, classes=cls, want=1), ref_search(after))
    n1_after = s.eligible_bucket_size(1).tolist()
    assert n1_after[1] == 0 and n1_before[1] > 0
    # one word for all ids, then set_tags restores the original words exactly
    ix.edit_tags(f["ids"][rows], set_bits=TOMB)
    assert np.array_equal(np.sort(ix.ids_with(want=TOMB)), np.sort(f["ids"][rows]))
    ix.set_tags(f["ids"][rows], f["tags"][rows])
    assert torch.equal(ix.tags, before) and np.array_equal(ix.tags_by_pos, _build(f).tags_by_pos)


# ---- 7. deletes by tombstone ------------------------------------------------------------------
def _tomb_rows(f):
    rng = np.random.default_rng(78)
    lab = f["labels"]
    return np.concatenate([rng.choice(np.flatnonzero(lab == c), n, replace=False)
                           for c, n in ((0, 38), (1, 5), (2, 7))])


def test_tombstones_equal_remove():
    f = _fixture(768)
    gone = f["ids"][_tomb_rows(f)]
    ix = _build(f)
    ix.edit_tags(gone, set_bits=TOMB)
    s = Searcher(ix, None)
    removed = ix.remove(gone)
    compacted = ix.remove(ix.ids_with(want=TOMB))
    assert np.array_equal(compacted.pos_to_id, removed.pos_to_id)
    assert np.array_equal(compacted.tags_by_pos, removed.tags_by_pos) and torch.equal(compacted.tags, removed.tags)
    assert torch.equal(compacted.corpus, removed.corpus)
    q, cls = _T(f["q"]), _T(f["classes"])
    for kw in (dict(semantics="exact"), dict(use_threshold=True), dict(use_threshold=False)):
        got = s.search(None, q, R, k=10, classes=cls, avoid=TOMB, **kw)
        ref = Searcher(removed, None).search(None, q, R, k=10, classes=cls, **kw)
        assert _same_answer(got, ref), kw
        assert not np.isin(got[1], gone).any()


@pytest.mark.parametrize("inplace", [False, True])
def test_add_relabel_remove_carry_edited_tags(inplace):
    f = _fixture(768)
    rng = np.random.default_rng(79)
    rows, st, cl, after = _edit_case(f)
    m = 50
    ix = _build(f, capacity=N + m) if inplace else _build(f)
    ix.edit_tags(f["ids"][rows], set_bits=st, clear_bits=cl)
    new_x = rng.standard_normal((m, 768)).astype(np.float16).astype(np.float32)
    new_ids = np.arange(900001, 900001 + m, dtype=np.int64)
    new_tags = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) & ~np.uint32(TOMB)
    word = dict(zip(f["ids"].tolist() + new_ids.tolist(), after.tolist() + new_tags.tolist()))

    def carries(index):
        exp = np.array([word[i] for i in index.pos_to_id.tolist()], np.uint32)
        assert index.tags_by_pos.dtype == np.uint32 and np.array_equal(index.tags_by_pos, exp)
        assert np.array_equal(index.tags.cpu().numpy().view(np.uint32), exp)

    ix = ix.add(new_x, rng.integers(0, C, m), ids=new_ids, tags=new_tags, inplace=inplace)
    carries(ix)
    ix = ix.relabel(rng.integers(0, C, ix.n_rows), inplace=inplace)
    carries(ix)
    # an edit of the successor, then a removal of edited and unedited rows
    ix.edit_tags(new_ids[:5], set_bits=TOMB)
    for i in new_ids[:5].tolist():
        word[i] |= TOMB
    ix = ix.remove(np.concatenate([f["ids"][rows[:10]], new_ids[40:], f["ids"][_tomb_rows(f)[:5]]]), inplace=inplace)
    carries(ix)
    assert np.array_equal(np.sort(ix.ids_with(want=TOMB)), new_ids[:5])


# ---- 8. refusals, each before any launch ------------------------------------------------------
def test_refusals_come_before_any_launch():
    f = _fixture(96)
    q, cls = _T(f["q"]), _T(f["classes"])

    def fresh(**kw):
        return Searcher(_build(f, **kw), None)

    def refused(s, how, err=ValueError, **kw):
        t0 = None if s.index.tags is None else s.index.tags.clone()
        with pytest.raises(err):
            if how == "lists":
                s.lists(None, q, R, kw.pop("k", 10), classes=cls, **kw)
            elif how == "search":
                s.search(None, q, R, classes=cls, **kw)
            elif how == "range":
                s.range_search(None, q, R, 0.5, classes=cls, **kw)
            else:
                s.index.edit_tags(**kw)
        assert "buf" not in s.index._ws and "range" not in s.index._ws, "a workspace was allocated before the refusal"
        assert t0 is None or s.index.consumed or torch.equal(s.index.tags, t0)

    for how in ("lists", "search", "range"):
        refused(fresh(tags=None), how, avoid=1)                        # an untagged index
    s = fresh()
    both = np.zeros(NQ, np.int64)
    both[NQ - 1] = 4
    for how in ("lists", "range"):
        refused(s, how, want=5, avoid=4)                                # a bit both wanted and avoided
        refused(s, how, want=both, avoid=both)                          # ... in one query of the batch
        refused(s, how, want=both, avoid=4)
        refused(s, how, avoid=np.ones(NQ - 1, np.int64))                # shape
        refused(s, how, avoid=np.ones((NQ, 1), np.int64))
        refused(s, how, avoid=-1)                                       # range
        refused(s, how, avoid=1 << 32)
        refused(s, how, avoid=np.full(NQ, 1 << 32, np.int64))
        refused(s, how, avoid=np.full(NQ, -1, np.int64))
        refused(s, how, avoid=np.ones(NQ, np.float32))                  # not integers
    refused(s, "search", want=5, avoid=4)
    refused(s, "search", want=3, avoid=1, semantics="exact")
    refused(s, "search", avoid=f["avoid"])                              # a word per query under "reference"
    refused(s, "search", want=1, avoid=f["avoid"])
    refused(s, "lists", avoid=1, dist="f64")
    refused(s, "search", avoid=1, dist="f64")
    refused(s, "search", avoid=1, dist="f64", semantics="exact")
    refused(s, "lists", avoid=1, k=17)                                  # k_list > 16
    # edit_tags
    ids = f["ids"]
    refused(s, "edit", ids=[int(ids[0]), int(ids[1]), int(ids[0])], set_bits=1)      # duplicate ids
    refused(s, "edit", ids=[int(ids[0]), 7], set_bits=1)                             # an id the index does not hold
    refused(s, "edit", err=KeyError, ids=[7], set_bits=1)                            # (as remove reports it)
    refused(s, "edit", ids=ids[:3], set_bits=1 << 32)                                # words outside [0, 2^32)
    refused(s, "edit", ids=ids[:3], clear_bits=-1)
    refused(s, "edit", ids=ids[:3], set_bits=[1, 2])                                 # one word per id
    refused(s, "edit", ids=ids[:3], set_bits=np.ones(3, np.float32))
    refused(fresh(tags=None), "edit", ids=ids[:3], set_bits=1)                       # an untagged index
    with pytest.raises(ValueError):
        fresh(tags=None).index.ids_with(want=1)
    with pytest.raises(ValueError):
        s.index.ids_with(want=1, avoid=1)
    shard = Searcher(_build(f, rank=0, world=2), None)
    refused(shard, "edit", ids=shard.index.pos_to_id[:1], set_bits=1)                # a stripe of a sharded index
    old = fresh(capacity=N)
    new = old.index.remove(ids[:1], inplace=True)
    refused(old, "edit", err=RuntimeError, ids=ids[1:2], set_bits=1)                 # a consumed index
    assert np.array_equal(new.tags_by_pos[np.isin(new.pos_to_id, ids[1:2])], f["tags"][1:2])
    # nothing changed, and the index still answers
    assert s.index.tags_version == 0 and np.array_equal(s.index.tags_by_pos, _build(f).tags_by_pos)
    d, _, _ = _lists(s, f, 10, avoid=1)
    assert np.isfinite(d).any()


# ---- 9. the drop-in class ----------------------------------------------------------------------
def test_learned_index_retag_search_want_avoid():
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    Cw, w_, a_ = 8, 1, TOMB
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
    ids = np.arange(1, 2001, dtype=np.int64)
    li_ = LearnedIndex()
    li_.model = nn
    index = li_.attach(nav, ds, w["labels"], tags=tags)
    hide = rng.choice(ids, 300, replace=False)
    li_.retag(hide, set_bits=TOMB)
    flip = rng.choice(ids, 100, replace=False)
    li_.retag(flip, tags=np.full(100, 6))
    after = tags.copy()
    after[hide - 1] |= np.uint32(TOMB)
    after[flip - 1] = 6
    got = li_.search(nav, w["qn"], ds, w["q"], w["labels"], n_buckets=3, k=10, use_threshold=True,
                     want=w_, avoid=a_)
    assert li_._index is index                                # the attached index, edited in place
    # the Searcher's filtered answer, and the answer over the eligible objects alone
    s = li_._get_searcher(li_._index)
    mine = s.search(_T(w["qn"]), _T(w["q"]), 3, k=10, use_threshold=True, want=w_, avoid=a_)
    m = _ok(after, w_, a_)
    ref = Searcher(DeviceIndex(w["x"][m], w["labels"][m], s.index.n_buckets, ids=ids[m], device=DEV),
                   DeviceRouter(w["layers"], device=DEV)).search(_T(w["qn"]), _T(w["q"]), 3, k=10,
                                                                 use_threshold=True)
    for a in (mine, ref):
        assert _same_answer(got, a)
    # an attach with the old words does not take the edited index for its own
    assert li_.attach(nav, ds, w["labels"], tags=tags) is not index
