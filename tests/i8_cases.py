"""The 8-bit storage restated in numpy (include/lmi_hip.h, LMI_I8 and
lmi_quantize_rows_i8): quantise, distances, lists by (distance, position).
Independent of li/: every bit an i8 index produces is pinned against these few
lines, with no tolerance anywhere.

  quantise   m = max |v_j| in float32; !(m >= 2^-100): all codes 0; else
             s = m / 127 and c_j = clip(rint(v_j / s), -127, 127), both
             divisions IEEE float32, rint half-to-even; columns d..d_pad 0;
             inv = 1 if sum c^2 == 0 else float32(1 / sqrt(float64(sum c^2)))
  distance   acc = sum cq_j cy_j (an exact integer, |acc| < 2^24);
             d = fmaf(-float(acc), invq * invy, 1) with invq * invy one
             float32 product p.  acc * p has at most 48 significant bits and
             p >= 2^-29, so 1 - acc * p is exact in float64: one rounding to
             float32 gives the fma's bits
  lists      per (query, probe): the bucket's rows by (d, global position),
             the first k, padded (+inf, -1)
"""
import numpy as np


def d_pad_of(d: int) -> int:
    return (int(d) + 31) // 32 * 32


def quantize(v):
    """(codes int8 [n, d_pad], inv float32 [n]) of the rows v [n, d] (fp16
    and float32 as they are, float64 rounded to float32 first)."""
    v = np.asarray(v)
    assert v.ndim == 2 and v.dtype in (np.float16, np.float32, np.float64)
    v = v.astype(np.float32)
    n, d = v.shape
    codes = np.zeros((n, d_pad_of(d)), np.int8)
    with np.errstate(invalid="ignore"):
        m = np.max(np.abs(v), axis=1) if d else np.zeros(n, np.float32)   # (a NaN makes the maximum NaN)
        live = m >= np.float32(2.0 ** -100)
    s = (m[live] / np.float32(127.0)).astype(np.float32)
    r = np.rint(v[live] / s[:, None])
    assert r.dtype == np.float32
    codes[live, :d] = np.clip(r, -127.0, 127.0).astype(np.int8)
    ss = (codes.astype(np.int64) ** 2).sum(axis=1)
    inv = np.ones(n, np.float32)
    inv[ss > 0] = (1.0 / np.sqrt(ss[ss > 0].astype(np.float64))).astype(np.float32)
    return codes, inv


def distances(cq, invq, cy, invy):
    """float32 [nq, n]: the distance of every query to every row."""
    acc = cq.astype(np.float64) @ cy.astype(np.float64).T       # exact: integers below 2^53
    assert np.array_equal(acc, np.rint(acc)) and (np.abs(acc) < 2.0 ** 24).all()
    p = invq.astype(np.float32)[:, None] * invy.astype(np.float32)[None, :]
    assert p.dtype == np.float32 and (p >= np.float32(2.0 ** -29)).all()
    return (1.0 - acc * p.astype(np.float64)).astype(np.float32)


def bucket_lists(dist, bucket_off, classes, k, eligible=None):
    """(d float32 [nq, R, k], pos int32 [nq, R, k]) from dist [nq, n] over the
    rows in bucket-sorted position order: per (query, probe) the rows of the
    probed bucket (with `eligible` [nq, n] bool: the eligible ones) by
    (distance, position), the first k, padded (+inf, -1).  A class outside
    [0, C) is a probe with no bucket."""
    classes = np.asarray(classes)
    nq, R = classes.shape
    out_d = np.full((nq, R, k), np.inf, np.float32)
    out_p = np.full((nq, R, k), -1, np.int32)
    C = len(bucket_off) - 1
    for i in range(nq):
        for r in range(R):
            c = int(classes[i, r])
            if not 0 <= c < C:
                continue
            p = np.arange(bucket_off[c], bucket_off[c + 1])
            if eligible is not None:
                p = p[eligible[i, p]]
            best = p[np.lexsort((p, dist[i, p]))][:k]
            out_d[i, r, :best.size], out_p[i, r, :best.size] = dist[i, best], best
    return out_d, out_p


def merged_topk(lists_d, lists_pos, k, pos_to_id):
    """The exact semantics' answer from per-probe lists: each query's k best
    by (distance, position) over its R lists, ids for positions, (10000, 0)
    past the end -> (float64 [nq, k], uint32 [nq, k])."""
    nq = lists_d.shape[0]
    d, p = lists_d.reshape(nq, -1), lists_pos.reshape(nq, -1)
    out_d = np.full((nq, k), 10000.0, np.float64)
    out_a = np.zeros((nq, k), np.uint32)
    for i in range(nq):
        keep = np.flatnonzero(p[i] >= 0)
        best = keep[np.lexsort((p[i, keep], d[i, keep]))][:k]
        out_d[i, :best.size] = d[i, best].astype(np.float64)
        out_a[i, :best.size] = pos_to_id[p[i, best]].astype(np.uint32)
    return out_d, out_a
