"""Search inside an id allow-list (bucket_topk(subset=), scan_subset_kernel) against
plain float64 numpy: for each (query, probe) pair the subset's rows of the probed
bucket, 1 - <q, y> / (|q| |y|), sorted by (distance, position).  Distances within
d_pad * 2^-23 (fp32 accumulation of d_pad fp16 products); positions equal wherever
the reference's gap to every other entry of its k + 1 deep list is above that
tolerance or exactly 0 (equal rows: ties go by position).

One index of 3 uneven buckets (608, 150, 70 rows, fp16-exact; rows 100..119 of
bucket 0 are one vector) and 40 queries: round 0 puts all 40 on bucket 0 (two
groups of a bucket), round 1 cycles buckets 1, 2 and no probe.  Queries 0..3 are
the repeated vector.  The subsets, by rows taken of each bucket:
  0-1-32   no row, one row, exactly one block
  33       a block and one row in one slice (sub_rows 64); 1; 0
  slices   148 of bucket 0 at sub_rows 64: three slices, the last short
  whole    every row, sub_rows the call's own
  deep     every row at sub_rows 640: bucket 0 is one slice of 19 blocks, five a
           wave -- the position queue's third entry (d 96: a block a stage) and
           its rotation hold real blocks
  ties     54 rows, the 20 equal ones, 31 more of bucket 0 at sub_rows 64: the equal
           rows are entries 54..73, across the slice boundary at 64
Every subset's ids are given shuffled."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_topk

pytestmark = pytest.mark.gpu

SIZES, NQ, R = (608, 150, 70), 40, 2
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
_r = lambda n, m, seed: np.sort(np.random.default_rng(seed).choice(n, m, replace=False))  # noqa: E731
SUBSETS = {  # name -> (bucket-local rows of each bucket, sub_rows)
    "0-1-32": (([], [7], _r(70, 32, 1)), None),
    "33": ((_r(300, 33, 2), [149], []), 64),
    "slices": ((_r(300, 148, 3), _r(150, 40, 4), _r(70, 5, 5)), 64),
    "whole": ((np.arange(608), np.arange(150), np.arange(70)), None),
    "deep": ((np.arange(608), np.arange(150), np.arange(70)), 640),
    "ties": ((np.r_[0:54, 100:120, 150:181], _r(150, 9, 6), []), 64),
}


@functools.lru_cache(maxsize=None)
def _fixture(d):
    rng = np.random.default_rng(d)
    n = sum(SIZES)
    x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    x[100:120] = x[100]
    q = rng.standard_normal((NQ, d)).astype(np.float16).astype(np.float32)
    q[:4] = x[100]
    labels = np.repeat(np.arange(3), SIZES)  # (bucket-sorted already: position == input row, id == row + 1)
    classes = np.stack([np.zeros(NQ, np.int32), np.array([1, 2, -1], np.int32)[np.arange(NQ) % 3]], axis=1)
    ix = DeviceIndex(x, labels, 3, storage="f16", chunk_rows=64, device="cuda")
    return x, q, labels, classes, ix


def _positions(name):
    rows, sub_rows = SUBSETS[name]
    off = np.r_[0, np.cumsum(SIZES)]
    return np.concatenate([off[c] + np.asarray(r, np.int64) for c, r in enumerate(rows)]), sub_rows


@functools.lru_cache(maxsize=None)
def _reference(d, name):
    """(dist float64 [NQ, R, 17], pos [NQ, R, 17]) padded (inf, -1)."""
    x, q, labels, classes, _ = _fixture(d)
    pos, _ = _positions(name)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    out_d, out_p = np.full((NQ, R, 17), np.inf), np.full((NQ, R, 17), -1, np.int64)
    for i in range(NQ):
        for r in range(R):
            rows = pos[labels[pos] == classes[i, r]]
            # (row by row, not a gemv: equal rows get bit-equal distances, whatever the BLAS blocks)
            y = x64[rows]
            dist = 1.0 - (y * q64[i]).sum(axis=1) / (np.sqrt((y * y).sum(axis=1)) * np.sqrt((q64[i] * q64[i]).sum()))
            order = np.lexsort((rows, dist))[:17]
            out_d[i, r, :order.size], out_p[i, r, :order.size] = dist[order], rows[order]
    if name == "ties":  # (the 20 equal rows head the lists of queries 0..3, at one distance)
        assert np.all(out_d[:4, 0, :17] == out_d[:4, 0, :1]) and np.all(out_p[:4, 0, :17] == 100 + np.arange(17))
    return out_d, out_p


@pytest.mark.parametrize("name", sorted(SUBSETS))
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("d", [96, 768, 992])
def test_subset_lists_match_float64(d, k, name):
    x, q, labels, classes, ix = _fixture(d)
    pos, sub_rows = _positions(name)
    ref_d, ref_p = _reference(d, name)
    tol = (d + 31) // 32 * 32 * 2.0 ** -23
    with np.errstate(invalid="ignore"):
        gap = np.abs(ref_d[..., :k, None] - ref_d[..., None, :k + 1])
    gap[np.isnan(gap)] = np.inf  # (inf - inf: padding against padding)
    clear = np.all((gap > tol) | (gap == 0), axis=-1)
    assert clear.mean() >= 0.9, f"the gap rule exempts {1 - clear.mean():.1%} of the entries"
    ids = np.random.default_rng(k).permutation(pos + 1)
    got_d, got_p, st = bucket_topk(ix, T(q), T(classes), k, subset=ids, sub_rows=sub_rows)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    got_d, got_p = got_d.cpu().numpy(), got_p.cpu().numpy()
    assert got_d.dtype == np.float32 and got_d.shape == (NQ, R, k)
    full = np.isfinite(ref_d[..., :k])
    assert np.array_equal(np.isfinite(got_d), full) and np.all(got_p[~full] == -1)
    err = np.abs(got_d[full] - ref_d[..., :k][full]).max(initial=0.0)
    print(f"[subset] d{d} k{k} {name}: max |d - ref| {err:.3g} (tol {tol:.3g}), clear {clear.mean():.1%}")
    assert err <= tol
    assert np.array_equal(got_p[clear], ref_p[..., :k][clear])


def test_subset_lists_are_the_few_scan_of_the_subset_index_bit_for_bit():
    """768 x k = 10: both kernels add the same fp32 products in the same order
    (segments of 128 k, eight MFMAs each), so the lists of the index built from
    the subset's rows alone are these lists, positions mapped back."""
    x, q, labels, classes, ix = _fixture(768)
    pos, sub_rows = _positions("slices")
    got_d, got_p, _ = bucket_topk(ix, T(q), T(classes), 10, subset=pos[::-1] + 1, sub_rows=sub_rows)
    small = DeviceIndex(x[pos], labels[pos], 3, storage="f16", chunk_rows=64, device="cuda")
    few_d, few_p, _ = bucket_topk(small, T(q), T(classes), 10, few=True, few_rows=32)
    torch.cuda.synchronize()
    few_p = few_p.cpu().numpy()
    back = np.where(few_p >= 0, pos[np.maximum(few_p, 0)], -1)
    assert np.array_equal(got_d.cpu().numpy().view(np.int32), few_d.cpu().numpy().view(np.int32))
    assert np.array_equal(got_p.cpu().numpy(), back)


def test_an_empty_subset_is_all_padding():
    x, q, labels, classes, ix = _fixture(96)
    got_d, got_p, st = bucket_topk(ix, T(q), T(classes), 10, subset=np.zeros(0, np.int64))
    assert bool(torch.isinf(got_d).all()) and bool((got_p == -1).all()) and int(st.item()) == 0


@pytest.mark.parametrize("semantics", ["reference", "exact"])
def test_search_in_a_subset_is_the_search_of_the_subset_index(semantics):
    w = workloads.clustered(n=1500, d=96, nq=5, C=8, seed=1996, label_mode="skewed")
    n, C = 1500, 8
    s = Searcher(DeviceIndex(w["x"], w["labels"], C, chunk_rows=256, device="cuda"),
                 DeviceRouter(w["layers"], device="cuda"))
    keep = np.sort(np.random.default_rng(3).choice(n, n // 3, replace=False))
    dists, anns = s.search(T(w["qn"]), T(w["q"]), 3, k=10, semantics=semantics, subset=keep[::-1] + 1)
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    if semantics == "exact":
        ref_d, ref_a = O.search_exact(w["labels"][keep], keep + 1, w["x"][keep], w["q"], classes, C, 3, k=10)
    else:  # (Searcher.search's default: the thresholded round merge)
        ref_d, ref_a = O.search_via_lists(w["labels"][keep], keep + 1, w["x"][keep], w["q"], classes, C, 3, k=10,
                                          use_threshold=True)
    assert O.compare_lists(ref_d, ref_a, dists, anns) == 0
