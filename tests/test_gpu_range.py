"""Range search (K11): every object of a query's probed buckets within its
radius -- the 8-wave ring's collect scan (scan3_kernel MODE 2) at d = 768, the
general kernel's collect form (range_scan_kernel: fp16 math, fp32 math over
fp16 and over float32 rows, each with and without tags) everywhere else, the
float64 re-score and the pack -- against numpy float64, against the project's
own top-k lists (bitwise) and against the index built from the eligible rows.

The fixture has test_gpu_tagged's shape: 3 buckets of 2 100 / 37 / 700 rows
with chunk_rows = 1024 (bucket 0: three chunks, the last of 52 rows = one full
32-row block + a 20-row tail; bucket 1 under one chunk), 300 queries x 2 probes
with bucket 0 probed by 270 queries in round 0 and by the other 30 in round 1,
and its tag layout.  Radii cycle per query through -1 (nothing), 2 (everything)
and the float32 midpoint between the query's m-th and (m+1)-th smallest float64
distance over its probed rows, m = 1, 10, 200.

Tolerances.  eps = refine_eps(d_pad, f16math) bounds |d32 - d64| for every
(query, row) (its docstring derives it), so in float32 a row with D64 < r - eps
must come, one with D64 > r + eps must not, and rows in between may go either
way; numpy alone counts those and the fixture is accepted only if they are at
most 1 % of the must-have rows.  In float64 the device and numpy differ by the
summation order of a d-term dot product, a few ulp of 1: 1e-12."""
import functools

import numpy as np
import pytest
import torch

import workloads
from li import _lib
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_range, refine_eps

pytestmark = pytest.mark.gpu

SIZES = (2100, 37, 700)
N, C, CHUNK, NQ, R = sum(SIZES), 3, 1024, 300, 2
WANTS = (0, 1, 7, 1 << 31, 1 << 30, 5)
DEV = "cuda"
CASES = [(768, True), (96, True), (200, True), (96, False)]   # (d, fp16-exact values / storage f16)


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


@functools.lru_cache(maxsize=None)
def _numpy64(d, exact=True):
    """(D64 [NQ, N] by position, probed [NQ, N] bool, radius float32 [NQ]) -- numpy alone."""
    f, s = _fixture(d, exact), _tagged(d, exact)
    order, off = s.index.layout.order, s.index.layout.bucket_off
    x = f["x"][order].astype(np.float64)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    qn = f["q"].astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    dist = 1.0 - qn @ xn.T
    probed = np.zeros((NQ, N), bool)
    for c in range(C):
        probed[np.ix_((f["classes"] == c).any(axis=1), np.arange(off[c], off[c + 1]))] = True
    radius = np.empty(NQ, np.float32)
    for i in range(NQ):
        kind = i % 5
        if kind == 0:
            radius[i] = -1.0
        elif kind == 1:
            radius[i] = 2.0
        else:
            m = (1, 10, 200)[kind - 2]
            v = np.sort(dist[i, probed[i]])
            radius[i] = np.float32(0.5 * (v[m - 1] + v[m]))
    for a in (dist, probed, radius):
        a.setflags(write=False)
    return dist, probed, radius


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _range(s, f, radius, rows=slice(None), **kw):
    kw.setdefault("classes", _T(f["classes"][rows]))
    return s.range_search(None, _T(f["q"][rows]), R, radius, **kw)


def _pos_of(s, anns):
    """global positions of returned ids (the ids are unique)."""
    inv = np.full(int(s.index.pos_to_id.max()) + 1, -1, np.int64)
    inv[s.index.pos_to_id] = np.arange(s.index.pos_to_id.size)
    return inv[anns.astype(np.int64)]


def _check_order(lims, dists, pos):
    assert lims[0] == 0 and lims[-1] == dists.size == pos.size and np.all(np.diff(lims) >= 0)
    for i in range(lims.size - 1):
        dd, pp = dists[lims[i]:lims[i + 1]], pos[lims[i]:lims[i + 1]]
        assert np.array_equal(np.lexsort((pp, dd)), np.arange(dd.size)), i
        assert np.unique(pp).size == pp.size, i


def _f32_bits(a):
    return np.asarray(a, np.float64).astype(np.float32).view(np.uint32)


# ---- 1. against numpy float64 ----------------------------------------------------------
@pytest.mark.parametrize("d,exact", CASES)
def test_f32_result_against_numpy_float64(d, exact):
    f, s = _fixture(d, exact), _tagged(d, exact)
    D, probed, radius = _numpy64(d, exact)
    eps = refine_eps(s.index.d_pad, exact)
    must = probed & (D < radius[:, None].astype(np.float64) - eps)
    never = ~probed | (D > radius[:, None].astype(np.float64) + eps)
    either = probed & ~must & ~never
    print(f"d={d} exact={exact}: eps={eps:g} must={must.sum()} either={either.sum()}")
    assert either.sum() <= 0.01 * must.sum()                  # (a condition of the fixture)
    lims, dists, anns = _range(s, f, radius)
    pos = _pos_of(s, anns)
    _check_order(lims, dists, pos)
    got = np.zeros((NQ, N), bool)
    qi = np.repeat(np.arange(NQ), np.diff(lims))
    got[qi, pos] = True
    assert not (must & ~got).any(), "a row inside r - eps is missing"
    assert not (never & got).any(), "a row outside r + eps (or of an unprobed bucket) is returned"
    assert np.abs(dists - D[qi, pos]).max() <= eps
    assert np.all(dists <= radius[qi].astype(np.float64))     # (inclusive, and never above)
    # (the radii do what they are there for)
    n = np.diff(lims)
    assert (n[0::5] == 0).all() and (n[2::5] >= 1).all() and (n[4::5] >= 190).all()


@pytest.mark.parametrize("d,exact", CASES)
def test_f64_result_against_numpy_float64(d, exact):
    f, s = _fixture(d, exact), _tagged(d, exact)
    D, probed, radius = _numpy64(d, exact)
    r = radius.astype(np.float64)[:, None]
    close = probed & (np.abs(D - r) <= 1e-12)
    assert close.sum() <= 3
    lims, dists, anns = _range(s, f, radius.astype(np.float64), dist="f64")
    pos = _pos_of(s, anns)
    _check_order(lims, dists, pos)
    got = np.zeros((NQ, N), bool)
    qi = np.repeat(np.arange(NQ), np.diff(lims))
    got[qi, pos] = True
    want = probed & (D <= r)
    assert np.array_equal(got | close, want | close)
    assert np.abs(dists - D[qi, pos]).max() <= 1e-12
    assert np.all(dists <= r[qi, 0])


# ---- 2. whole buckets -------------------------------------------------------------------
@pytest.mark.parametrize("d,exact", CASES)
def test_whole_buckets_and_nothing(d, exact):
    f, s = _fixture(d, exact), _tagged(d, exact)
    size = s.index.bucket_size
    lims, dists, anns = _range(s, f, 2.0)
    assert np.array_equal(np.diff(lims), size[f["classes"]].sum(axis=1))
    _check_order(lims, dists, _pos_of(s, anns))
    for w in WANTS[1:]:
        lims, dists, anns = _range(s, f, 2.0, want=w)
        assert np.array_equal(np.diff(lims), s.eligible_bucket_size(w)[f["classes"]].sum(axis=1)), w
        t = s.index.tags_by_pos[_pos_of(s, anns)]
        assert np.all((t & np.uint32(w)) == np.uint32(w))
    for dist in ("f32", "f64"):
        lims, dists, anns = _range(s, f, -1.0, dist=dist)
        assert not lims.any() and lims.shape == (NQ + 1,) and dists.size == 0 and anns.size == 0
        assert lims.dtype == np.int64 and dists.dtype == np.float64 and anns.dtype == np.uint32


# ---- 3. round trip with the top-k scan, bitwise -------------------------------------------
@pytest.mark.parametrize("d,exact", [(768, True), (96, True), (96, False)])
def test_round_trip_with_the_lists_bitwise(d, exact):
    f, s = _fixture(d, exact), _tagged(d, exact)
    q, cls = _T(f["q"]), _T(f["classes"][:, :1])
    _, ld, lpos, st = s.lists(None, q, 1, 10, classes=cls)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    ld, lpos = ld.cpu().numpy()[:, 0], lpos.cpu().numpy()[:, 0]
    assert np.isfinite(ld).all()
    lims, dists, anns = s.range_search(None, q, 1, ld[:, 9], classes=cls)
    pos = _pos_of(s, anns)
    n = np.diff(lims)
    assert (n >= 10).all()
    head = lims[:-1, None] + np.arange(10)[None, :]
    assert np.array_equal(_f32_bits(dists[head]), ld.view(np.uint32)), "not the lists' float32 bits"
    assert np.array_equal(pos[head], lpos)
    # everything after the list is tied with its 10th distance (the comparison is inclusive)
    tail = np.ones(dists.size, bool)
    tail[head.ravel()] = False
    qi = np.repeat(np.arange(NQ), n)
    assert np.array_equal(_f32_bits(dists[tail]), ld[qi[tail], 9].view(np.uint32))
    # (the duplicate rows of bucket 0 make such ties: some query has one)
    _check_order(lims, dists, pos)


def test_round_trip_tagged_at_768_with_the_general_kernels_lists():
    """A tagged call at d = 768 runs the general kernel's collect form, so its
    distances are those of the general kernel's lists: k_list = 16 with a want
    word (scan_kernel TAG; the 10-entry tagged lists run the 8-wave ring)."""
    f, s = _fixture(768), _tagged(768)
    q, cls = _T(f["q"][:270]), _T(f["classes"][:270, :1])        # (bucket 0: enough eligible rows)
    _, ld, lpos, st = s.lists(None, q, 1, 16, classes=cls, want=1)
    torch.cuda.synchronize()
    ld, lpos = ld.cpu().numpy()[:, 0], lpos.cpu().numpy()[:, 0]
    assert int(st.item()) == 0 and np.isfinite(ld).all()
    lims, dists, anns = s.range_search(None, q, 1, ld[:, 15], classes=cls, want=1)
    head = lims[:-1, None] + np.arange(16)[None, :]
    assert (np.diff(lims) >= 16).all()
    assert np.array_equal(_f32_bits(dists[head]), ld.view(np.uint32))
    assert np.array_equal(_pos_of(s, anns)[head], lpos)


# ---- 4. capacity ------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dist", [(768, "f32"), (96, "f32"), (96, "f64")])
def test_result_does_not_depend_on_pair_cap(d, dist):
    f, s = _fixture(d), _tagged(d)
    t_small, t_large = {}, {}
    small = _range(s, f, 2.0, dist=dist, pair_cap=32, timings=t_small)
    large = _range(s, f, 2.0, dist=dist, pair_cap=4096, timings=t_large)
    assert t_small["scans"] == 2 and t_large["scans"] == 1
    assert t_small["results"] == t_large["results"] == small[0][-1]
    for a, b in zip(small, large):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # the counts are exact whatever the cap, and only pairs of bucket 1 (37 rows) fit 32... none do
    count, cand, st = bucket_range(s.index, _T(f["q"]), _T(f["classes"]), 2.0, pair_cap=32)
    assert np.array_equal(count.cpu().numpy(), s.index.bucket_size[f["classes"]])
    assert tuple(cand.shape) == (NQ, R, 32) and int(st.item()) == 0
    # mixed radii: some pairs overflow 32 slots, most do not
    radius = _numpy64(d)[2]
    t_mixed = {}
    a = _range(s, f, radius, dist=dist, pair_cap=32, timings=t_mixed)
    b = _range(s, f, radius, dist=dist, pair_cap=4096)
    assert t_mixed["scans"] == 2
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ---- 5. tags ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d,exact,dist", [(96, True, "f32"), (200, True, "f32"), (96, False, "f32"),
                                          (96, True, "f64"), (768, True, "f64")])
def test_per_query_want_equals_the_eligible_rows_index(d, exact, dist):
    """(float32 at 96 / 200: the general kernel on both sides, so bitwise.  At
    768 the tagged call runs the general kernel and the untagged index the
    8-wave ring, two kernel families whose float32 distances differ in the last
    bits: there the float64 results are compared, which no family enters.)"""
    f, s = _fixture(d, exact), _tagged(d, exact)
    radius = _numpy64(d, exact)[2].astype(np.float64)
    lims, dists, anns = _range(s, f, radius, want=f["want"], dist=dist)
    for w in WANTS:
        rows = np.flatnonzero(f["want"] == w)
        assert rows.size
        rl, rd, ra = _range(_eligible(d, w, exact), f, radius[rows], rows=rows, dist=dist)
        assert np.array_equal(np.diff(lims)[rows], np.diff(rl)), (d, w)
        sel = np.concatenate([np.arange(lims[i], lims[i + 1]) for i in rows]).astype(np.int64)
        assert np.array_equal(anns[sel], ra), (d, w)
        assert np.array_equal(dists[sel].view(np.uint64), rd.view(np.uint64)), (d, w)
    n = np.diff(lims)
    assert n[f["want"] == 1 << 31].max() <= 4 and n[f["want"] == 1].max() > 100


def test_tagged_at_768_against_numpy_float64():
    f, s = _fixture(768), _tagged(768)
    D, probed, radius = _numpy64(768)
    eps = refine_eps(768, True)
    ok = (s.index.tags_by_pos[None, :] & f["want"][:, None]) == f["want"][:, None]
    must = probed & ok & (D < radius[:, None].astype(np.float64) - eps)
    never = ~(probed & ok) | (D > radius[:, None].astype(np.float64) + eps)
    lims, dists, anns = _range(s, f, radius, want=f["want"])
    pos = _pos_of(s, anns)
    _check_order(lims, dists, pos)
    qi = np.repeat(np.arange(NQ), np.diff(lims))
    got = np.zeros((NQ, N), bool)
    got[qi, pos] = True
    assert not (must & ~got).any() and not (never & got).any()
    assert np.abs(dists - D[qi, pos]).max() <= eps


# ---- 6. float64 against the project's own float64 lists ------------------------------------------
SMALL = (200, 37, 150)


@functools.lru_cache(maxsize=None)
def _small(d):
    rng = np.random.default_rng(77 + d)
    n, nq = sum(SMALL), 60
    x = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((nq, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(3), SMALL)).astype(np.int64)
    # a stored row whose norm lies between the float64 and the float32 zero rules:
    # one element of 2^-24 (the smallest fp16 value), norm 6e-8, in bucket 0
    low = int(np.flatnonzero(labels == 0)[5])
    x[low] = 0
    x[low, 3] = np.float16(2.0 ** -24)
    classes = np.stack([np.arange(nq) % 3, (np.arange(nq) + 1) % 3], axis=1).astype(np.int32)
    ix = DeviceIndex(x, labels, 3, ids=np.arange(n) + 1, chunk_rows=64, device=DEV)
    assert ix.storage == "f16" and ix.inv_norm64 is not None
    return dict(x=x, q=q, classes=classes, low=low), Searcher(ix, None)


@pytest.mark.parametrize("d", [768, 96])
def test_f64_equals_the_filter_of_the_float64_lists(d):
    f, s = _small(d)
    nq = f["q"].shape[0]
    q, cls = _T(f["q"]), _T(f["classes"])
    _, ld, lpos, st = s.lists(None, q, 2, 200, classes=cls, dist="f64")
    torch.cuda.synchronize()
    ld, lpos = ld.cpu().numpy(), lpos.cpu().numpy()
    assert not int(st.item()) & _lib.LMI_STATUS_INTERNAL
    assert np.array_equal((lpos >= 0).sum(axis=2), s.index.bucket_size[f["classes"]])   # every row is listed
    radius = np.empty(nq, np.float64)
    for i in range(nq):
        v = np.sort(ld[i][lpos[i] >= 0])
        # -1, 2, a listed distance exactly (the 1st, the 20th), a midpoint
        radius[i] = (-1.0, 2.0, v[0], v[19], 0.5 * (v[60] + v[61]))[i % 5]
    lims, dists, anns = s.range_search(None, q, 2, radius, classes=cls, dist="f64")
    low_pos = int(np.flatnonzero(s.index.pos_to_id == f["low"] + 1)[0])
    seen_low = 0
    for i in range(nq):
        keep = (lpos[i] >= 0) & (ld[i] <= radius[i])
        dd, pp = ld[i][keep], lpos[i][keep]
        o = np.lexsort((pp, dd))
        a, b = lims[i], lims[i + 1]
        assert b - a == o.size, i
        assert np.array_equal(dists[a:b].view(np.uint64), dd[o].view(np.uint64)), i
        assert np.array_equal(anns[a:b].astype(np.int64), s.index.pos_to_id[pp[o]]), i
        seen_low += int(low_pos in pp)
    assert (np.diff(lims)[2::5] >= 1).all() and (np.diff(lims)[3::5] >= 20).all()   # inclusive at a listed value
    assert seen_low >= 4                        # the low-norm row answers (with its true norm)
    # its distance is that of its direction, not the ~1 a norm of 1 would give
    i = next(i for i in range(1, nq, 5) if 0 in f["classes"][i])
    seg = slice(lims[i], lims[i + 1])
    d_low = dists[seg][anns[seg] == f["low"] + 1]
    qv = f["q"][i].astype(np.float64)
    assert d_low.size == 1 and abs(d_low[0] - (1.0 - qv[3] / np.linalg.norm(qv))) < 1e-12


# ---- 7. probes and empty buckets --------------------------------------------------------------
def test_unprobed_entries_an_empty_bucket_and_an_empty_batch():
    f = _fixture(96)
    # the same rows in an index of 5 buckets: 3 and 4 are empty
    s = Searcher(DeviceIndex(f["x"], f["labels"], 5, ids=f["ids"], chunk_rows=CHUNK, device=DEV), None)
    cls = f["classes"].copy()
    cls[0::4, 0] = -1
    cls[1::4, 1] = 3
    cls[2::8] = -1
    radius = _numpy64(96)[2]
    for dist in ("f32", "f64"):
        lims, dists, anns = _range(s, f, radius, classes=_T(cls), dist=dist)
        # each probe alone, through the other column unprobed
        parts = []
        for r in range(R):
            one = np.full_like(cls, -1)
            one[:, r] = np.where(cls[:, r] == 3, -1, cls[:, r])
            parts.append(_range(s, f, radius, classes=_T(one), dist=dist))
        n = np.diff(lims)
        assert np.array_equal(n, np.diff(parts[0][0]) + np.diff(parts[1][0]))
        assert (n[2::8] == 0).all() and n.sum() > 0
        for i in range(NQ):
            dd = np.concatenate([p[1][p[0][i]:p[0][i + 1]] for p in parts])
            aa = np.concatenate([p[2][p[0][i]:p[0][i + 1]] for p in parts])
            assert np.array_equal(np.sort(aa), np.sort(anns[lims[i]:lims[i + 1]])), i
            assert np.array_equal(np.sort(dd), np.sort(dists[lims[i]:lims[i + 1]])), i
        lims0, d0, a0 = s.range_search(None, _T(f["q"][:0]), R, 0.5, classes=_T(cls[:0]), dist=dist)
        assert lims0.tolist() == [0] and d0.size == 0 and a0.size == 0
    # a bucket named twice answers twice
    twice = np.tile(np.array([[1, 1]], np.int32), (8, 1))
    lims, dists, anns = s.range_search(None, _T(f["q"][:8]), R, 2.0, classes=_T(twice))
    assert (np.diff(lims) == 2 * SIZES[1]).all()
    assert np.array_equal(anns[0:2 * SIZES[1]:2], anns[1:2 * SIZES[1]:2])


def test_stop_mass_through_the_router():
    w = workloads.clustered(n=3000, d=96, nq=64, C=8, arch="MLP", label_mode="skewed")
    layers = [(a.copy(), b.copy()) for a, b in w["layers"]]
    layers[-1] = (layers[-1][0] * np.float32(100), layers[-1][1] * np.float32(100))
    s = Searcher(DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=512, device=DEV),
                 DeviceRouter(layers, device=DEV))
    qn, q = _T(w["qn"]), _T(w["q"])
    cls = s.route(qn, 4, stop_mass=0.8)
    assert bool((cls < 0).any()) and bool((cls[:, 0] >= 0).all())
    tm = {}
    got = s.range_search(qn, q, 4, 0.9, stop_mass=0.8, timings=tm)
    ref = s.range_search(None, q, 4, 0.9, classes=cls)
    full = s.range_search(qn, q, 4, 0.9)
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert 0 < got[0][-1] <= full[0][-1]
    assert 1.0 <= tm["mean_probes"] < 4.0


# ---- 8. the drop-in class ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_learned_index_range_search(dtype):
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    Cw = 8
    w = workloads.clustered(n=2000, d=96, nq=64, C=Cw, seed=11, label_mode="router")
    nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=Cw, lr=0.009, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    x, q = w["x"].astype(dtype), w["q"].astype(dtype)
    nav, ds = pd.DataFrame(w["xn"][:1900]), pd.DataFrame(x[:1900])
    nav.index += 1
    ds.index += 1
    li_ = LearnedIndex()
    li_.model = nn
    li_.attach(nav, ds, w["labels"][:1900])
    dist = "f64" if dtype == np.float16 else "f32"
    radius = np.linspace(0.5, 1.0, 64)

    def both(nav, ds, labels):
        got = li_.range_search(nav, w["qn"], ds, q, labels, radius, n_buckets=3)
        s = li_._get_searcher(li_._index)
        ref = s.range_search(_T(w["qn"]), _T(q.astype(np.float32)), 3, radius, dist=dist)
        assert got[0][-1] > 0
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        return got

    first = both(nav, ds, w["labels"][:1900])
    nav_new, ds_new = pd.DataFrame(w["xn"][1900:]), pd.DataFrame(x[1900:])
    nav_new.index += 1901
    ds_new.index += 1901
    nav2, ds2, lab2 = li_.insert(nav, ds, w["labels"][:1900], nav_new, ds_new, inplace=False)
    second = both(nav2, ds2, lab2)
    assert second[0][-1] > first[0][-1] and np.isin(second[2], np.arange(1901, 2001)).any()


# ---- a stale fp16 check: the scan reports it and the call is redone in fp32 math -------------------
@pytest.mark.parametrize("d", [768, 96])
@pytest.mark.parametrize("dist", ["f32", "f64"])
def test_a_stale_fp16_check_is_redone_in_fp32_math(d, dist):
    """Queries that fp16 does not hold, scanned as LMI_Q_F16 because the cached check said so: the
    scan raises LMI_STATUS_QUERY_NOT_F16 and range_search runs again with exact fp32 MFMA, in
    float64 under the bound of that arithmetic's eps.  The answer is the one of a Searcher that
    decided fp32 math at once, bit for bit."""
    f = _fixture(d)
    ix = _tagged(d).index
    q = _T(f["q"] * np.float32(1.0 + 2.0 ** -13))
    assert not torch.equal(q.half().float(), q)
    radius = _numpy64(d)[2]
    t0, t1 = {}, {}
    right = _range(Searcher(ix, None), dict(f, q=q.cpu().numpy()), radius, dist=dist, timings=t0)
    stale = Searcher(ix, None)
    stale.qmode = lambda _q: _lib.LMI_Q_F16
    got = _range(stale, dict(f, q=q.cpu().numpy()), radius, dist=dist, timings=t1)
    assert "fp32_redo" not in t0 and t1["fp32_redo"] == 1
    assert right[0][-1] > 0 and t0["results"] == t1["results"]
    for u, v in zip(right, got):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ---- the widths at the collect scan's limits -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide(d, storage):
    """Two buckets of 100 / 37 rows (chunk_rows = 64: bucket 0 is a full chunk and one of 36 rows =
    a 32-row block + a 4-row tail), 9 queries x 1 probe."""
    rng = np.random.default_rng(7700 + d + (0 if storage == "f16" else 1))
    x = rng.standard_normal((137, d)).astype(np.float32)
    q = rng.standard_normal((9, d)).astype(np.float32)
    if storage == "f16":
        x, q = x.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    labels = np.repeat(np.arange(2), (100, 37)).astype(np.int64)
    classes = (np.arange(9, dtype=np.int32) % 2)[:, None]
    return dict(x=x, q=q, labels=labels, classes=classes)


@pytest.mark.parametrize("d,storage", [(1248, "f16"), (1248, "f32"), (1056, "f16")])
def test_the_widest_query_tiles_answer(d, storage):
    """d_pad = 1248 is the widest query tile that fits a workgroup's LDS in either arithmetic (1280
    is refused, below), and 1056 is past the float64 search's limit but not float32's.  Radii: 2.0
    (the whole bucket) for odd queries, the float32 midpoint between the 5th and 6th smallest
    float64 distance for even ones, under test 1's bounds."""
    w = _wide(d, storage)
    s = Searcher(DeviceIndex(w["x"], w["labels"], 2, chunk_rows=64, device=DEV, storage=storage), None)
    order, off = s.index.layout.order, s.index.layout.bucket_off
    xn = w["x"][order].astype(np.float64)
    xn /= np.linalg.norm(xn, axis=1, keepdims=True)
    qn = w["q"].astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    D = 1.0 - qn @ xn.T
    eps = refine_eps(d, storage == "f16")
    radius = np.full(9, 2.0, np.float32)
    for i in range(0, 9, 2):
        v = np.sort(D[i, off[0]:off[1]])
        radius[i] = np.float32(0.5 * (v[4] + v[5]))
    lims, dists, anns = s.range_search(None, _T(w["q"]), 1, radius, classes=_T(w["classes"]))
    pos = _pos_of(s, anns)
    _check_order(lims, dists, pos)
    for i in range(9):
        c = int(w["classes"][i, 0])
        got, dd = pos[lims[i]:lims[i + 1]], dists[lims[i]:lims[i + 1]]
        assert np.all((got >= off[c]) & (got < off[c + 1])), i
        assert np.all(np.abs(dd - D[i, got]) <= eps), i
        row = D[i, off[c]:off[c + 1]]
        r = float(radius[i])
        must = off[c] + np.flatnonzero(row < r - eps)
        assert np.isin(must, got).all(), i
        assert not np.any(D[i, got] > r + eps), i
        if i % 2:
            assert got.size == off[c + 1] - off[c], i


# ---- 9. refusals, each before a workspace exists ---------------------------------------------------
def test_refusals_come_before_any_workspace():
    f = _fixture(96)
    q, cls = _T(f["q"]), _T(f["classes"])

    def fresh(**kw):
        kw.setdefault("tags", f["tags"])
        return Searcher(DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV, **kw),
                        None)

    def refused(s, radius=0.5, q=q, **kw):
        with pytest.raises(ValueError):
            s.range_search(None, q, R, radius, classes=cls, **kw)
        assert not s.index._ws, "a workspace was allocated before the refusal"

    s = fresh()
    refused(s, float("nan"))
    refused(s, np.full(NQ, np.nan))
    refused(s, np.where(np.arange(NQ) == 7, np.nan, 0.5))
    refused(s, np.full(NQ - 1, 0.5))                               # shape
    refused(s, np.full((NQ, 1), 0.5))
    refused(s, dist="f16")
    refused(s, pair_cap=0)
    refused(s, stop_mass=1.5)
    refused(s, want=-1)
    refused(s, want=np.ones(NQ - 1, np.int64))
    refused(fresh(tags=None), want=1)                               # an untagged index
    # float64 queries that float32 rounding changes (those it does not change are taken)
    q64 = f["q"].astype(np.float64)
    refused(s, q=_T(q64 * (1.0 + 2.0 ** -40)))
    refused(s, q=_T(q64 * (1.0 + 2.0 ** -40)), dist="f64")
    # a sub-cluster layout, a stripe, an exchange group
    g = _fixture(768)
    sub = Searcher(DeviceIndex(g["x"], g["labels"], C, ids=g["ids"], chunk_rows=CHUNK, device=DEV,
                               subcluster=True), None)
    assert sub.index.chunk_centroid is not None
    with pytest.raises(ValueError):
        sub.range_search(None, _T(g["q"]), R, 0.5, classes=cls)
    assert not sub.index._ws
    refused(Searcher(DeviceIndex(f["x"], f["labels"], C, ids=f["ids"], chunk_rows=CHUNK, device=DEV,
                                 rank=0, world=2), None))
    ex = fresh()
    ex.exchange = True
    refused(ex)
    # storage "f32x" (the split mode): float32 values that are not fp16-exact at d_pad 768
    g = _fixture(768, False)
    sx = Searcher(DeviceIndex(g["x"][:300], g["labels"][:300], C, chunk_rows=CHUNK, device=DEV), None)
    assert sx.index.storage == "f32x"
    with pytest.raises(ValueError):
        sx.range_search(None, _T(g["q"]), R, 0.5, classes=_T(g["classes"]))
    # float64 rows (corpus64)
    s64 = Searcher(DeviceIndex(f["x"].astype(np.float64) * (1.0 + 2.0 ** -40), f["labels"], C, chunk_rows=CHUNK,
                               device=DEV), None)
    assert s64.index.corpus64 is not None
    with pytest.raises(ValueError):
        s64.range_search(None, q, R, 0.5, classes=cls, dist="f64")
    # a width the search refuses: in float64 d > 1024 (the float64 search's own limit; float32 takes
    # it), and in either arithmetic a d_pad whose query tile passes a workgroup's LDS (d_pad > 1248)
    for d, storage, dists in ((1056, "f16", ("f64",)), (1280, "f32", ("f32", "f64")), (1280, "f16", ("f32",))):
        w = _wide(d, storage)
        sw = Searcher(DeviceIndex(w["x"], w["labels"], 2, chunk_rows=64, device=DEV, storage=storage), None)
        assert sw.index.d_pad == d and not sw.index._ws
        for dist in dists:
            with pytest.raises(ValueError):
                sw.range_search(None, _T(w["q"]), 1, 0.5, classes=_T(w["classes"]), dist=dist)
            assert not sw.index._ws, (d, storage, dist)
        if d > 1248:
            with pytest.raises(ValueError):
                bucket_range(sw.index, _T(w["q"]), _T(w["classes"]), 0.5)
            assert not sw.index._ws, (d, storage)
    # a consumed index raises as everywhere else
    gone = fresh(capacity=N + 8)
    gone.index.add(f["x"][:2], f["labels"][:2], ids=[1, 2], inplace=True)
    with pytest.raises(RuntimeError):
        gone.range_search(None, q, R, 0.5, classes=cls)
    # the index still answers, and float64 queries that float32 holds are taken
    a = s.range_search(None, q, R, 0.9, classes=cls)
    b = s.range_search(None, _T(q64), R, 0.9, classes=cls)
    assert a[0][-1] > 0
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
