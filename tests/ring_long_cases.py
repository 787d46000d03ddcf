"""The 8-wave rings' shared fixture at real tile lengths, in plain numpy: the rows,
queries, tags and probed classes that tests/test_gpu_ring_long.py scans on storage
"i8", "mx4", "mx6" and on the metric ring (l2 / ip), and the conditions planted in
them, each asserted here from a restatement's distances alone
(tests/test_ring_long_cases_host.py runs these asserts without a GPU).

chunk_rows = 2112 (66 blocks of 32 rows), d = 768, R = 2, eight buckets with
unpermuted labels (position == row).  A tile is one chunk of one bucket:

  bucket  rows  blocks of its tiles     the smallest case of
  0         65  3 (one-row tail)        the steady-state wait (two blocks ahead), no in-loop DMA
  1         97  4                       the first in-loop DMA, into slot 3
  2        129  5                       the slot wrap back to slot 0
  3        257  9                       the norm-area wrap (mx rings: eight areas)
  4       1024  32                      the bound exchange on the tile's last block
  5       1025  33 (one-row tail)       an exchanged bound consumed by a later block
  6       5264  66, 66, 33 (16 rows)    two exchanges a tile (blocks 31, 63); three concurrent
                                        tiles of one pair
  7          0  none                    an empty bucket

Probing, written out: 257 queries.  Column 0 of `classes` is bucket 6 for every
query (257 pairs: a full 256-pair tile plus a one-pair tile, on each of the three
chunks); column 1 gives buckets 0..3 five pairs each, bucket 4 32, bucket 5 33,
bucket 7 four, names one class >= C, and is -1 (a probe a stop rule dropped) for
the 167 queries left.  (No query probes one bucket twice, so the 257 pairs of
bucket 6 need 257 queries: the second column cannot be filled with live probes
without changing the pair counts.)  Pairs of a bucket are scanned in ascending
pair id, so pair number j of bucket 6 is query j.

Planted on top of standard_normal rows and queries rounded to fp16:

  P1  heterogeneous bounds in one tile.  Four directions g_0..g_3; 16 rows
      g_i + 0.05 noise each at in-chunk rows below 992 of bucket 6's chunk 0, and
      every even query but QTIE is g_(j/2 % 4) + 0.05 noise.  Those pairs own a
      tight bound before block 31 publishes it, the odd pairs nothing near it: an
      exchanged bound read back for the wrong pair empties the odd lists from
      block 32 on.  Asserted: each even pair's 16 best are its direction's rows,
      and each odd pair's 10th- / 16th-best distance exceeds every even pair's
      by more than `margin` (100 TOL for the cosine storages).
  P2  ties at an exchanged bound.  20 exact copies of one row of bucket 6 over
      its three chunks (TIE_AT), 15 of them at in-chunk offsets of 1024 or more;
      query QTIE is twice that row.  Asserted: the copies' distances are bitwise
      equal and strictly below every other row's of the bucket.  Expected of a
      scan: the k lowest positions, one distance bit pattern.

Tags (storage "i8"): random bits 0..2, and bit 31 on six rows of bucket 6, all
at in-chunk offsets of 1024 or more (three of them copies of P2's row): a query
wanting bit 31 meets its first eligible row after the first exchange.

The metric workload scales every row by a seeded factor in [0.5, 4] and every
query by one in [0.5, 2] (without the norm spread l2 and ip rank like cosine).
The factors are not uniform: twelve rows of every bucket (bucket 6: past row 1024
of a chunk, so a list's best rows arrive after the first exchange) take the spaced
factors 0.5, 0.56 .. 1.16 and every other row one in [1.5, 4] -- under uniform
factors the l2 top-10 of a 5264-row bucket has a gap inside test_gpu_metric's
bound in 56 % of the lists, and its strict-id rule would exempt them.  A
direction's queries share one factor s in [1.5, 2] and its rows take s + 0.03 j,
j = 1..16; P2's row has factor 2 and its query (twice the scaled row) too: P1 and
P2 hold under l2 and under ip, asserted likewise on float64 distances by the
definition.  SEED: picked on the CPU so that the float64 references alone keep
_check's strict-id exemption under its cap of 10 % of the lists; METRIC_SHARES
records the measured shares (the host test measures them again).
"""
import functools

import numpy as np

CHUNK, D, R = 2112, 768, 2
SIZES = (65, 97, 129, 257, 1024, 1025, 5264, 0)
PROBES = (5, 5, 5, 5, 32, 33, 257, 4)
BLOCKS = {3, 4, 5, 9, 32, 33, 66}
N, C, NQ = sum(SIZES), len(SIZES), 257
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
B6 = int(OFF[6])
TOL = 768 * 2.0 ** -23            # tests/test_gpu_mx4.py's derived bound
SEED = 7690
METRIC_SHARES = {("l2", 1): 0.008, ("l2", 10): 0.019, ("ip", 1): 0.004, ("ip", 10): 0.058}    # of 514 lists, SEED 7690
GROUPS = 4
QTIE = 100
# (chunk of bucket 6, in-chunk row) of P2's copies
TIE_AT = ((0, 5), (0, 1030), (0, 1500), (0, 2100),
          (1, 40), (1, 1024), (1, 1055), (1, 1056), (1, 1600), (1, 2047), (1, 2048), (1, 2111),
          (2, 0), (2, 31), (2, 1023), (2, 1024), (2, 1025), (2, 1030), (2, 1038), (2, 1039))
TIE_POS = np.array([B6 + c * CHUNK + r for c, r in TIE_AT], np.int64)
# bit 31: six rows of bucket 6 past the first exchange, three of them P2's copies
WANT31_AT = ((0, 1024), (0, 1500), (0, 2111), (1, 1057), (1, 2048), (2, 1030))
WANT31_POS = np.array([B6 + c * CHUNK + r for c, r in WANT31_AT], np.int64)
# the i8 ring tests' predicates (want, avoid); (1 << 28, 0) wants a bit no row carries
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 2), (0, 7), (1 << 31, 1), (4, 3), (1 << 28, 0))

assert len(TIE_AT) == 20 and sum(r >= 1024 for _, r in TIE_AT) == 15 and np.all(np.diff(TIE_POS) > 0)
assert all(r >= 1024 for _, r in WANT31_AT) and np.isin(WANT31_POS, TIE_POS).sum() == 3


def classes():
    """int32 [NQ, 2], written out (see the module docstring)."""
    col1 = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(PROBES) if c != 6] +
                          [np.array([C + 3], np.int32)])
    cls = np.full((NQ, R), -1, np.int32)
    cls[:, 0] = 6
    cls[:col1.size, 1] = col1
    return cls


def tile_blocks():
    """The 32-row block count of every tile (chunk of a bucket), from OFF and CHUNK."""
    out = []
    for c in range(C):
        rows = int(OFF[c + 1] - OFF[c])
        out += [(min(CHUNK, rows - a) + 31) // 32 for a in range(0, rows, CHUNK)]
    return out


def check_shape(cls):
    """The pair counts and the tiles' block counts."""
    live = (cls >= 0) & (cls < C)
    assert tuple(np.bincount(cls[live], minlength=C)) == PROBES
    assert (cls >= C).sum() == 1 and (cls[~live & (cls < C)] == -1).all()
    assert all(np.unique(row[(row >= 0) & (row < C)]).size == ((row >= 0) & (row < C)).sum() for row in cls)
    assert (cls[:, 0] == 6).all()                       # pair j of bucket 6 is query j
    assert set(tile_blocks()) == BLOCKS and len(tile_blocks()) == 9
    assert sorted(tile_blocks())[-3:] == [33, 66, 66]


@functools.lru_cache(maxsize=None)
def fixture():
    rng = np.random.default_rng(SEED)
    x = rng.standard_normal((N, D)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((NQ, D)).astype(np.float16).astype(np.float32)
    g = rng.standard_normal((GROUPS, D))
    free = np.setdiff1d(np.arange(992), [r for c, r in TIE_AT if c == 0])
    plant = np.sort(rng.choice(free, (GROUPS, 16), replace=False), axis=1)       # in-chunk rows of chunk 0
    for i in range(GROUPS):
        x[B6 + plant[i]] = (g[i] + 0.05 * rng.standard_normal((16, D))).astype(np.float16)
    even = np.array([j for j in range(0, NQ, 2) if j != QTIE])
    odd = np.arange(1, NQ, 2)
    group = (even // 2) % GROUPS
    q[even] = (g[group] + 0.05 * rng.standard_normal((even.size, D))).astype(np.float16)
    x[TIE_POS] = x[TIE_POS[0]]
    q[QTIE] = 2.0 * x[TIE_POS[0]]
    labels = np.repeat(np.arange(C), SIZES).astype(np.int64)
    tags = rng.integers(0, 8, N).astype(np.uint32)
    tags[WANT31_POS] = np.uint32(1 << 31) | np.uint32(2)
    pair = rng.integers(0, len(PAIRS), NQ)
    pair[:len(PAIRS)] = np.arange(len(PAIRS))
    pair[[QTIE, 31, 32, 254, 255, 256]] = PAIRS.index((1 << 31, 1))             # both pair tiles, even and odd pairs
    pw = np.array(PAIRS, np.int64)[pair]
    # the metric workload's factors
    sx, sq = rng.uniform(1.5, 4.0, N), rng.uniform(0.5, 2.0, NQ)
    for c in range(C - 1):                              # a bucket's twelve short rows (bucket 6: past row 1024 of a chunk)
        at = np.arange(OFF[c], OFF[c + 1])
        if c == 6:
            at = np.setdiff1d(at[(at - B6) % CHUNK >= 1024], TIE_POS)
        sx[rng.choice(at, 12, replace=False)] = 0.5 + 0.06 * rng.permutation(12)
    sg = rng.uniform(1.5, 2.0, GROUPS)
    for i in range(GROUPS):
        sx[B6 + plant[i]] = sg[i] + 0.03 * (1 + rng.permutation(16))
    sq[even] = sg[group]
    sx[TIE_POS], sq[QTIE] = 2.0, 2.0
    xm = (x * sx[:, None]).astype(np.float16).astype(np.float32)
    qm = (q * sq[:, None]).astype(np.float16).astype(np.float32)
    assert np.isfinite(xm).all() and np.isfinite(qm).all()
    assert np.array_equal(xm[TIE_POS], np.tile(xm[TIE_POS[0]], (20, 1))) and np.array_equal(qm[QTIE], 2 * xm[TIE_POS[0]])
    f = dict(x=x, q=q, labels=labels, classes=classes(), tags=tags, want=pw[:, 0].copy(), avoid=pw[:, 1].copy(),
             plant=B6 + plant, even=even, odd=odd, group=group, xm=xm, qm=qm)
    for v in f.values():
        v.setflags(write=False)
    check_shape(f["classes"])
    assert np.array_equal(np.bincount(labels, minlength=C), SIZES)
    return f


def eligible(tags, want, avoid):
    """bool [nq, n]: (tag & want) == want and (tag & avoid) == 0."""
    t = np.asarray(tags, np.uint32)[None, :]
    w, a = np.asarray(want).astype(np.uint32)[:, None], np.asarray(avoid).astype(np.uint32)[:, None]
    return ((t & w) == w) & ((t & a) == 0)


@functools.lru_cache(maxsize=None)
def restated(storage):
    """[NQ, N] distances of the fixture by the storage's numpy restatement (i8:
    float32, exact; mx4 / mx6: float64), computed once and left unchanged."""
    f = fixture()
    if storage == "i8":
        import i8_cases as I8
        cx, ix = I8.quantize(f["x"])
        cq, iq = I8.quantize(f["q"])
        dist = I8.distances(cq, iq, cx, ix)
    else:
        M = __import__({"mx4": "mx4_cases", "mx6": "mx6_cases"}[storage])
        vy, vq = M.quantize(f["x"]), M.quantize(f["q"])
        dist = M.distances64(vq[3], vq[2], vy[3], vy[2])
    dist.setflags(write=False)
    return dist


def metric_dist64(metric):
    """float64 [NQ, N] of the metric workload by the definition."""
    f = fixture()
    q, x = f["qm"].astype(np.float64), f["xm"].astype(np.float64)
    acc = q @ x.T
    if metric == "ip":
        return -acc
    if metric == "l2":
        return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * acc
    return 1.0 - acc / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :])


@functools.lru_cache(maxsize=None)
def metric_reference(metric, depth=11):
    """(D [NQ, N]; ref_d, ref_p [NQ, R, depth], (inf, -1) padded): every probed
    bucket's rows by (float64 distance, position)."""
    D, cls = metric_dist64(metric), fixture()["classes"]
    rd = np.full((NQ, R, depth), np.inf)
    rp = np.full((NQ, R, depth), -1, np.int64)
    for i in range(NQ):
        for r in range(R):
            c = int(cls[i, r])
            if 0 <= c < C:
                a, b = OFF[c], OFF[c + 1]
                o = np.argsort(D[i, a:b], kind="stable")[:depth]
                rd[i, r, :o.size], rp[i, r, :o.size] = D[i, a:b][o], a + o
    for v in (D, rd, rp):
        v.setflags(write=False)
    return D, rd, rp


def bucket_mask(cls):
    """bool [NQ, R, N]: position p lies in the bucket cls[i, r] names."""
    live = (cls >= 0) & (cls < C)
    c = np.where(live, cls, 0)
    pos = np.arange(N)[None, None, :]
    return live[..., None] & (pos >= OFF[c][..., None]) & (pos < OFF[c + 1][..., None])


def check_planted(dist, margin, ks=(10, 16)):
    """P1 and P2 on dist [NQ, N] (any restatement's, or a metric's float64)."""
    f = fixture()
    d6 = dist[:, B6:B6 + SIZES[6]]
    order = np.argsort(d6, axis=1, kind="stable")
    kth = np.take_along_axis(d6, order, 1)
    # P1: an even pair's 16 best are its direction's 16 rows, all below in-chunk row 992 of chunk 0 ...
    best16 = np.sort(order[f["even"], :16], axis=1) + B6
    assert np.array_equal(best16, f["plant"][f["group"]]) and (best16 < B6 + 992).all()
    # ... and every odd pair's k-th best lies more than `margin` above every even pair's
    for k in ks:
        gap = kth[f["odd"], k - 1].min() - kth[f["even"], k - 1].max()
        assert gap > margin, (k, gap, margin)
    # P2: the copies' distances are one bit pattern, strictly below every other row of the bucket
    tie = dist[QTIE, TIE_POS]
    assert np.unique(np.ascontiguousarray(tie).view(np.uint32 if tie.dtype == np.float32 else np.uint64)).size == 1
    rest = np.setdiff1d(np.arange(B6, B6 + SIZES[6]), TIE_POS)
    assert tie[0] < dist[QTIE, rest].min()
    assert np.array_equal(order[QTIE, :20] + B6, TIE_POS)
    return {k: float(kth[f["odd"], k - 1].min() - kth[f["even"], k - 1].max()) for k in ks}


def check_tags():
    """Bit 31 is carried by WANT31_POS alone, each eligible under (1 << 31, 1); bit
    28 by no row; every predicate of PAIRS is used, (1 << 31, 1) on both pair
    tiles of bucket 6 and on QTIE."""
    f = fixture()
    t = f["tags"]
    assert np.array_equal(np.flatnonzero(t & np.uint32(1 << 31)), np.sort(WANT31_POS))
    assert eligible(t, [1 << 31], [1])[0].sum() == len(WANT31_AT) and not (t & np.uint32(1 << 28)).any()
    used = set(zip(f["want"].tolist(), f["avoid"].tolist()))
    assert used == set(PAIRS)
    on31 = np.flatnonzero(f["want"] == 1 << 31)
    assert {QTIE, 255, 256} <= set(on31.tolist())
    assert ((WANT31_POS - B6) % CHUNK >= 1024).all()


def strict_id_share(metric, k, bound):
    """The share of the metric reference's lists with a gap of at most bound[i]
    among their first k + 1 distances: what _check's strict-id rule exempts."""
    _, rd, _ = metric_reference(metric)
    with np.errstate(invalid="ignore"):
        gaps = np.diff(rd[..., :k + 1], axis=-1)
    gaps[np.isnan(gaps)] = np.inf
    return 1.0 - np.all(gaps > bound[:, None, None], axis=-1).mean()
