"""Inputs of the replay's parameter checks (tests/test_replay_params_host.py on
the CPU, tests/test_gpu_replay_params.py on the device): seeded
per-(query, probe) lists of any width and dtype, and the branch of
replay_group_body (csrc/lmi_replay_gpu.hip) a group takes, derived from the
inputs alone so a test can assert it before it reads a device result.

The lists are synthetic (no corpus): a replay reads only the lists, the
bucket sizes and the position -> id table."""
import collections

import numpy as np

# replay_group_body's dispatch constants (csrc/lmi_replay_gpu.hip)
TG = 1024          # kTG: threads of the group kernel's workgroup
UCAP = 8192        # kUCap: a group's entries staged in LDS, global scratch beyond
BM_BITS = 196608   # kBmBits: positions the selection bitmap spans
MAX_KR = 32        # kMaxKr
MAX_K = 64         # kMaxW

KR_CLASSES = {"<=10": (1, 10), "11-16": (11, 16), "17-32": (17, 32)}  # fill<10 | 16 | 32>


def kr_class(kr):
    return next(name for name, (a, b) in KR_CLASSES.items() if a <= kr <= b)


def _pool(rng, n, dtype):
    """n distances: float32 from a pool rounded to 3 decimals (exact ties
    likely); float64 = that pool plus 0..3 times 1e-12, which ties in float32
    but not in float64, with exact float64 ties where both terms repeat."""
    base = np.round(rng.random(n) * 0.6 + 0.2, 3)
    if np.dtype(dtype) == np.float32:
        return base.astype(np.float32)
    return base + rng.integers(0, 4, n) * 1e-12


def make_lists(seed, nq, R, C, k_list, dtype=np.float32, sized=None, empty=(), probe_empty=False):
    """(classes [nq, R] int32, d [nq, R, k_list] dtype, pos int32, bucket sizes
    int64 [C], ids int64): every list sorted by (distance, position), its
    empty entries last as (+inf, -1).  `sized`: {category: forced size};
    `empty`: categories of size 0; `probe_empty`: queries may probe an empty
    category (a group the reference's groupby never visits)."""
    rng = np.random.default_rng(seed)
    size = rng.integers(40, 400, C).astype(np.int64)
    for c, n in (sized or {}).items():
        size[c] = n
    for c in empty:
        size[c] = 0
    off = np.concatenate([[0], np.cumsum(size)])
    live = np.arange(C) if probe_empty else np.nonzero(size > 0)[0]
    p = rng.dirichlet(np.full(live.size, 0.5))
    classes = np.stack([rng.choice(live, R, replace=False, p=p) for _ in range(nq)]).astype(np.int32)
    d = np.full((nq, R, k_list), np.inf, dtype)
    pos = np.full((nq, R, k_list), -1, np.int32)
    for q in range(nq):
        for r in range(R):
            c = classes[q, r]
            n = int(min(k_list, size[c]))
            if n == 0:
                continue
            pp = rng.choice(size[c], n, replace=False) + off[c]
            dd = _pool(rng, n, dtype)
            o = np.lexsort((pp, dd))
            d[q, r, :n], pos[q, r, :n] = dd[o], pp[o]
    ids = rng.permutation(int(off[-1])).astype(np.int64) + 1
    return classes, d, pos, size, ids


def wide_lists(seed, n_group, R, k_list, dtype=np.float32, big=300_000, small=5000):
    """Lists over three buckets of `big`, `small` and `small` rows, 3 * n_group
    queries, query q probing bucket (q + r) % 3 in round r: every round has one
    group of n_group queries per bucket.  A list in the big bucket holds
    positions below 1000 and above 250 000 in random distance order, so the
    relevant positions of its group span more than the selection bitmap
    whatever the thresholds keep; the small buckets are its twins inside the
    bitmap's span.  (Vectorised: no corpus, no per-query loop.)"""
    rng = np.random.default_rng(seed)
    nq = 3 * n_group
    size = np.array([big, small, small], np.int64)
    off = np.concatenate([[0], np.cumsum(size)])
    classes = ((np.arange(nq)[:, None] + np.arange(R)[None, :]) % 3).astype(np.int32)
    n_lo = (k_list + 1) // 2
    d = np.empty((nq, R, k_list), dtype)
    pos = np.empty((nq, R, k_list), np.int32)
    for r in range(R):
        lo = np.argsort(rng.random((nq, 1000)), axis=1)[:, :n_lo]
        hi = 250_001 + 24 * np.argsort(rng.random((nq, 2000)), axis=1)[:, :k_list - n_lo]
        p_big = np.concatenate([lo, hi], axis=1)
        p_small = (small // 1000) * np.argsort(rng.random((nq, 1000)), axis=1)[:, :k_list]
        pp = np.where((classes[:, r] == 0)[:, None], p_big, p_small) + off[classes[:, r]][:, None]
        dd = _pool(rng, nq * k_list, dtype).reshape(nq, k_list)
        # random distance order over the positions, then sorted by (distance, position)
        pp = np.take_along_axis(pp, np.argsort(rng.random((nq, k_list)), axis=1), axis=1)
        o = np.stack([np.lexsort((pp[q], dd[q])) for q in range(nq)])
        d[:, r], pos[:, r] = np.take_along_axis(dd, o, axis=1), np.take_along_axis(pp, o, axis=1)
    ids = rng.permutation(int(off[-1])).astype(np.int64) + 1
    return classes, d, pos, size, ids


def check_sorted(d, pos):
    """The lists' contract: ascending (distance, position), empties last."""
    e = pos < 0
    assert np.all(np.isinf(d[e])) and np.all(np.isfinite(d[~e]))
    assert np.all(e[..., 1:] | ~e[..., :-1]), "an entry after an empty one"
    a, b = d[..., :-1], d[..., 1:]
    both = ~e[..., 1:]
    assert np.all((a < b) | ((a == b) & (pos[..., :-1] < pos[..., 1:])) | ~both)


Branch = collections.namedtuple(
    "Branch", "n_group nU n_rel n_unique span staging select rows fill merge")


def group_branches(classes_r, d_r, pos_r, size, k_round, thr=None):
    """{category: Branch} of one round, for every category replay_group_body
    works on (a non-empty bucket with a non-empty group), from the inputs:
    classes_r [nq], this round's lists d_r / pos_r [nq, k_list], the bucket
    sizes, and `thr` [nq] (None: an unthresholded round).

      n_group, nU = n_group * k_round      the group and its entries
      n_rel, n_unique, span                relevant entries (pos >= 0 and
                                           d < thr), their distinct positions,
                                           max - min position
      staging   'lds' | 'global'           U in LDS (nU <= 8192) or scratch
      select    'bitmap' | 'sel2' | 'sel4' | 'sel8' | 'sel16' | 'loop'
                                           (span < 196608, else by nU)
      rows      'copy' | 'quirk0' | 'skipped' | 'fill' | 'quirk_thr'
      fill      10 | 16 | 32               membership width (by k_round)
      merge     4 | 8 | 16                 wave-list merge registers
    select, fill and merge are None where the kernel does not get there."""
    kr = int(k_round)
    out = {}
    for c in range(len(size)):
        G = np.nonzero(classes_r == c)[0]
        if G.size == 0 or size[c] <= 0:
            continue
        nU = int(G.size) * kr
        if thr is None:
            out[c] = Branch(G.size, nU, None, None, None, None, None,
                            "copy" if size[c] >= kr else "quirk0", None, None)
            continue
        dd, pp = d_r[G, :kr].astype(np.float64), pos_r[G, :kr]
        rel = (pp >= 0) & (dd < np.asarray(thr, np.float64)[G, None])
        # (a per-entry test is the reference's "leading entries" on sorted lists)
        assert np.all(rel[:, :-1] | ~rel[:, 1:])
        staging = "lds" if nU <= UCAP else "global"
        if not rel.any():
            out[c] = Branch(G.size, nU, 0, 0, None, staging, None, "skipped", None, None)
            continue
        u = np.unique(pp[rel])
        span = int(u[-1] - u[0])
        if span < BM_BITS:
            select, merge = "bitmap", None
        else:
            select = next((f"sel{m}" for m in (2, 4, 8, 16) if nU <= m * TG), "loop")
            merge = next(m for m in (4, 8, 16) if (TG // 64) * 2 * kr <= m * 64)
        rows = "fill" if u.size >= kr else "quirk_thr"
        fill = (10 if kr <= 10 else 16 if kr <= 16 else 32) if rows == "fill" else None
        out[c] = Branch(G.size, nU, int(rel.sum()), int(u.size), span, staging, select, rows, fill,
                        merge)
    return out


def running_thresholds(replay_fn, r, classes, d, pos, **kw):
    """Round r's thresholds (r >= 1, use_threshold on): the row maxima of the
    merged result of rounds 0 .. r-1, from `replay_fn` (the host twin or the
    oracle) run on those rounds alone."""
    assert r >= 1
    fd, _ = replay_fn(np.ascontiguousarray(classes[:, :r]), np.ascontiguousarray(d[:, :r]),
                      np.ascontiguousarray(pos[:, :r]), **kw)
    return np.asarray(fd, np.float64).max(axis=1)


def k_finals(k_round, R):
    """The grid's k_final values that are legal: {1, kr - 1, kr, kr + 1,
    min(64, 2 kr)} within [1, 2 kr] (the reference's assert at every merge);
    R = 1 ignores k_final (the row is k_round wide), so one value."""
    if R == 1:
        return [k_round]
    ks = {1, k_round - 1, k_round, k_round + 1, min(MAX_K, 2 * k_round)}
    return sorted(k for k in ks if 1 <= k <= min(MAX_K, 2 * k_round))
