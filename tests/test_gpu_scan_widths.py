"""The scan (K2), its float64 refinement, Searcher.search, the batch stream and
the graphed step at row widths other than 768, against the oracle on float64
copies of the inputs.  Every width is there for a branch of the code:

    d     d_pad  what it exercises
    8     32     the general kernel's trailing 32-wide half block alone (the
                 fp16-math prologue must not load: it would read past the row)
    30    32     d % 4 != 0: scalar prep loads, the scalar row_dist64
    96    96     one full 64-wide block + the trailing block (pca96)
    100   128    padding inside the last block
    192   192    no trailing block, one piece per lane in the refinement
    740   768    the rings over zero-padded rows and queries, d % 4 == 0
    750   768    the same with d % 4 != 0
    800   800    trailing block; four pieces per lane (refine_kernel<.., 4>)
    832   832    d_pad % 64 == 0 above 768
    992   992    the largest d_pad the general kernel launches
    1024  1024   refused: the general kernel's LDS budget (below)

One seeded workload per (width, label mode), seed SEEDS[d] (900 + d unless
that workload broke a cap of the strict-id rule, below); the oracle's lists
are taken k + 1 deep (one O.bucket_lists call per workload at the deepest
k + 1 any case needs -- a list ordered by (distance, position) is a prefix of
every deeper one -- sliced per k and shared by every case)."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li import _lib
from li.index import (DeviceIndex, DeviceRouter, Searcher, bucket_topk, bucket_topk_f64,
                      refine_eps)

pytestmark = pytest.mark.gpu

N, NQ, C, R, CHUNK = 3000, 96, 8, 3, 256
WIDTHS = (8, 30, 96, 100, 192, 740, 750, 800, 832, 992)
TIE_WIDTHS = (30, 96, 800)      # "near" and "dup" beside "skewed": ties, duplicates
LO_WIDTHS = (96, 800)           # k = 40: the lower-bound passes on the general kernel
RING_WIDTHS = (740, 750)        # d_pad 768: fp16 math runs on the rings
# 900 + d, except where that workload's "skewed" lists put more rows inside the
# strict-id rule's bound than its caps allow (96: 12.9 % at k = 40; 800: 22.2 %
# at k = 40; 992: 13.2 % at k = 16, fp16 math): those widths take another seed
SEEDS = {d: 900 + d for d in WIDTHS}
SEEDS.update({96: 1996, 800: 7700, 992: 3892})
F16, F32 = _lib.LMI_Q_F16, _lib.LMI_Q_F32
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def _pad(d):
    return (d + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _workload(d, mode):
    w = workloads.clustered(n=N, d=d, nq=NQ, C=C, seed=SEEDS[d], label_mode=mode)
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    return w, np.ascontiguousarray(classes[:, :R])


@functools.lru_cache(maxsize=None)
def _inputs64(d, mode, f64in):
    """The oracle's operands: float64 copies of the float32 values, or
    workloads.float64_inputs (values that float32 rounding changes)."""
    w, _ = _workload(d, mode)
    if f64in:
        return workloads.float64_inputs(w, SEEDS[d])
    return w["x"].astype(np.float64), w["q"].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference_deep(d, mode, f64in):
    w, classes = _workload(d, mode)
    x64, q64 = _inputs64(d, mode, f64in)
    depth = (40 if d in LO_WIDTHS and not f64in else 16) + 1
    return O.bucket_lists(w["labels"], x64, q64, classes, R, depth, C)


def _reference(d, mode, k, f64in=False):
    """(distances, positions) [NQ, R, k + 1], float64."""
    rd, rp = _reference_deep(d, mode, f64in)
    return rd[..., :k + 1], rp[..., :k + 1]


@functools.lru_cache(maxsize=None)
def _index(d, mode, storage, f64in=False):
    w, _ = _workload(d, mode)
    data = _inputs64(d, mode, True)[0] if f64in else w["x"]
    ix = DeviceIndex(data, w["labels"], C, storage=storage, chunk_rows=CHUNK, device="cuda")
    assert ix.d_pad == _pad(d) and (ix.corpus64 is not None) == f64in
    return ix


def _clear_rows(ref_d, bound):
    """Rows (query, probe) whose consecutive oracle distances over the first
    k + 1 entries all differ by more than `bound`: two objects can change
    places only when the scan's distances, each within bound / 2 of the
    oracle's, cross.  (A gap to or between empty slots is infinite.)"""
    with np.errstate(invalid="ignore"):
        gaps = np.diff(ref_d.reshape(-1, ref_d.shape[-1]), axis=-1)
    gaps[np.isnan(gaps)] = np.inf
    return np.all(gaps > bound, axis=-1)


def _check(name, ref, got, k, *, f64, bound, cap=None):
    """`cap` (a share of the rows): also the strict-id rule -- every row whose
    oracle gaps all exceed `bound` has the oracle's ids -- after the cap on the
    rows that rule exempts, asserted from the oracle alone, before the GPU
    lists are looked at (it keeps the rule from emptying itself)."""
    ref_d, ref_p = ref
    got_d, got_p, st = got
    clear = _clear_rows(ref_d, bound)
    exempt = 1.0 - clear.mean()
    if cap is not None:
        assert exempt <= cap, f"{name}: the strict-id rule exempts {exempt:.1%} of the rows (cap {cap:.0%})"
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    got_d, got_p = got_d.cpu().numpy(), got_p.cpu().numpy()
    assert got_d.dtype == (np.float64 if f64 else np.float32) and got_d.shape == (NQ, R, k)
    tol = dict(atol=1e-12, tie=1e-12) if f64 else {}
    stats = {}
    bad = O.compare_lists(ref_d[..., :k], ref_p[..., :k], got_d, got_p, stats=stats, **tol)
    print(f"[widths] {name}: exempt {exempt:.2%} of {clear.size} rows (gap <= {bound:.3g}), "
          f"tie rows {stats['tie_rows']} ({stats['exact_tie_rows']} exact), mismatched {bad}")
    assert bad == 0
    if cap is not None:
        same = np.all(got_p.reshape(-1, k) == ref_p.reshape(-1, k + 1)[:, :k], axis=-1)
        assert np.all(same[clear]), f"{name}: ids differ in {int((~same & clear).sum())} clear rows"


def _f32_cases():
    """(d, mode, storage, qmode, k).  What cannot exist is not listed: at
    d_pad 768 (740, 750) fp16 storage with fp16-exact queries runs on the
    rings (k <= 15 the 8-wave ring, 16 the 4-wave one), never on the general
    kernel's fp16-math variant -- those rows are the rings over padding, with
    k = 12 for the 8-wave ring's 15-entry lists; k = 40 is asked only where
    the general LO kernel runs with and without a trailing block."""
    out = []
    for d in WIDTHS:
        for mode in ("skewed",) + (("near", "dup") if d in TIE_WIDTHS else ()):
            for k in (1, 10, 16) + ((12,) if d in RING_WIDTHS else ()):
                out.append((d, mode, "f16", F16, k))
            out.append((d, mode, "f16", F32, 10))      # fp32 math on fp16 rows
            out.append((d, mode, "f32", F32, 10))      # fp32 rows
            if d in LO_WIDTHS:
                out.append((d, mode, "f16", F16, 40))
                out.append((d, mode, "f32", F32, 40))
    return out


def _id32(c):
    d, mode, storage, qmode, k = c
    return f"d{d}-{mode}-{storage}-{'qf16' if qmode == F16 else 'qf32'}-k{k}"


@pytest.mark.parametrize("case", _f32_cases(), ids=_id32)
def test_float32_lists_match_oracle(case):
    """lmi_bucket_topk: compare_lists with the float32 defaults, and on
    "skewed" identical ids in every row whose oracle gaps exceed
    2 * refine_eps(d_pad, f16math), the proven bound on |d32 - d64|."""
    d, mode, storage, qmode, k = case
    w, classes = _workload(d, mode)
    f16math = storage == "f16" and qmode == F16
    got = bucket_topk(_index(d, mode, storage), T(w["q"]), T(classes.astype(np.int32)), k, qmode=qmode)
    _check(_id32(case), _reference(d, mode, k), got, k, f64=False,
           bound=2 * refine_eps(_pad(d), f16math),
           cap=(0.10 if f16math else 0.50) if mode == "skewed" else None)


def _f64_cases():
    return [(d, mode, f64in) for d in WIDTHS
            for mode in ("skewed",) + (("near", "dup") if d in TIE_WIDTHS else ())
            for f64in in (False, True)]


def _id64(c):
    d, mode, f64in = c
    return f"d{d}-{mode}-{'x64q64' if f64in else 'x16q32'}"


@pytest.mark.parametrize("case", _f64_cases(), ids=_id64)
def test_float64_lists_match_oracle(case):
    """lmi_bucket_topk_f64, k = 10, fp16 storage: float32 queries (TC = fp16
    rows; d % 4 picks the vector or the scalar row distance, ceil(d / 256) the
    pieces per lane), and float64 rows and queries (TC = double).  Lists
    within 1e-12; on "skewed" identical ids where the gaps exceed 2e-12."""
    d, mode, f64in = case
    w, classes = _workload(d, mode)
    q = _inputs64(d, mode, True)[1] if f64in else w["q"]
    got = bucket_topk_f64(_index(d, mode, "f16", f64in), T(q), T(classes.astype(np.int32)), 10)
    _check(_id64(case), _reference(d, mode, 10, f64in), got, 10, f64=True, bound=2e-12,
           cap=0.10 if mode == "skewed" else None)


@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_phases_compose_off_768(storage, dist):
    """The PLAN / SCAN / MERGE phase calls on the general kernel (d = 96) give
    the one-call lists bit for bit: what the batch stream runs at this width."""
    w, classes = _workload(96, "skewed")
    ix, q, cls = _index(96, "skewed", storage), T(w["q"]), T(classes.astype(np.int32))
    fn = bucket_topk_f64 if dist == "f64" else bucket_topk
    qmode = F16 if storage == "f16" else F32
    d0, p0, st0 = fn(ix, q, cls, 10, qmode=qmode)
    ws = torch.empty_like(ix._ws["f64"] if dist == "f64" else ix._ws["buf"])
    out = (torch.empty_like(d0), torch.empty_like(p0), torch.zeros_like(st0))
    for ph in (_lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_MERGE):
        fn(ix, q, cls, 10, qmode=qmode, out=out, ws=ws, phases=ph)
    assert torch.equal(out[0], d0) and torch.equal(out[1], p0) and int(out[2].item()) == 0 == int(st0.item())


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_width_1024_is_refused_before_the_launch(storage, f64):
    """The general kernel keeps a tile's queries in LDS: QB * (d_pad + QPAD)
    elements (fp16 math: 64 * (d_pad + 8) * 2 B; fp32 math: 32 * (d_pad + 4)
    * 4 B = 128 B per column either way; the merge buffer that aliases them is
    smaller), + the candidate queues 4 waves * 16 * 64 * 8 B = 32 KiB, + QB *
    12 B of bounds and norms + 16 B.  Under the 160 KiB cap: fp16 math
    128 (d_pad + 8) <= 163840 - 32768 - 784 -> d_pad <= 1009; fp32 math
    128 (d_pad + 4) <= 163840 - 32768 - 400 -> d_pad <= 1016; d_pad is a
    multiple of 32, so 992 launches (in the matrix above) and 1024 is refused
    by launch_scan's host-side check, for both variants and both list
    lengths.  Nothing is launched, nothing faults, and the process goes on
    answering: a d = 96 search afterwards equals the oracle."""
    w = workloads.clustered(n=N, d=1024, nq=NQ, C=C, seed=900 + 1024, label_mode="skewed")
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))[:, :R]
    ix = DeviceIndex(w["x"], w["labels"], C, storage=storage, chunk_rows=CHUNK, device="cuda")
    assert ix.d_pad == 1024
    fn = bucket_topk_f64 if f64 else bucket_topk
    with pytest.raises(_lib.LmiError, match=r"d_pad=1024 needs \d+ B of LDS"):
        fn(ix, T(w["q"]), T(classes.astype(np.int32)), 10)
    torch.cuda.synchronize()
    w, classes = _workload(96, "skewed")
    got = fn(_index(96, "skewed", storage), T(w["q"]), T(classes.astype(np.int32)), 10)
    _check(f"after-1024-{storage}-{'f64' if f64 else 'f32'}", _reference(96, "skewed", 10), got, 10,
           f64=f64, bound=0.0)


# ---------------------------------------------------------------------------
# end to end: Searcher.search against the oracle; the batch stream and the
# graphed step against Searcher.search on the same Searcher
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _searcher(d):
    w, _ = _workload(d, "skewed")
    return Searcher(_index(d, "skewed", "f16"), DeviceRouter(w["layers"], device="cuda"))


@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("d", [96, 100, 750])
def test_search_matches_oracle(d, dist):
    w, _ = _workload(d, "skewed")
    s = _searcher(d)
    dists, anns = s.search(T(w["qn"]), T(w["q"]), R, k=10, use_threshold=True, dist=dist)
    x, q = _inputs64(d, "skewed", False) if dist == "f64" else (w["x"], w["q"])
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    ids = np.arange(1, N + 1)
    ref_d, ref_a = O.search_via_lists(w["labels"], ids, x, q, classes, C, R, k=10, use_threshold=True)
    tol = dict(atol=1e-12, tie=1e-12) if dist == "f64" else {}
    stats = {}
    bad = O.compare_lists(ref_d, ref_a, dists, anns, stats=stats, **tol)
    print(f"[widths] search d{d}-{dist}: tie rows {stats['tie_rows']} of {stats['rows']}, mismatched {bad}")
    assert bad == 0


@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("d", [96, 100])
def test_stream_and_graph_equal_search(d, dist):
    w, _ = _workload(d, "skewed")
    s = _searcher(d)
    d0, a0 = s.search(T(w["qn"]), T(w["q"]), R, k=10, use_threshold=True, dist=dist)
    with s.streamed(w["qn"], w["q"], R, k=10, dist=dist) as st:
        for _ in range(2):
            d1, a1 = st.step()
            np.testing.assert_array_equal(d1, d0)
            np.testing.assert_array_equal(a1, a0)
    g = s.graph(w["qn"], w["q"], R, k=10, dist=dist)
    try:
        d2, a2 = g.run()
        np.testing.assert_array_equal(d2, d0)
        np.testing.assert_array_equal(a2, a0)
    finally:
        g.close()


def test_stream_refuses_an_odd_width():
    """The stream stages fp16 rows as int32 words (d / 2 per row)."""
    w = workloads.clustered(n=N, d=99, nq=NQ, C=C, seed=900 + 99, label_mode="skewed")
    s = Searcher(DeviceIndex(w["x"], w["labels"], C, chunk_rows=CHUNK, device="cuda"),
                 DeviceRouter(w["layers"], device="cuda"))
    with pytest.raises(ValueError, match="even d"):
        s.streamed(w["qn"], w["q"], R, k=10)


# ---------------------------------------------------------------------------
# the split mode (storage "f32x": float32 rows that are not fp16-exact, d_pad
# 768) with d < 768; test_gpu_split_mode.py's check and tolerance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [752, 750])
@pytest.mark.parametrize("k", [10, 16])
def test_split_lists_match_oracle_under_768(d, k):
    """d = 752 (a multiple of 16: the rows normalised in float32 beside the
    index, corpus32n) and d = 750 (no such copy; every candidate normalised
    when it is scored): both answer, float32 and float64 arithmetic, within
    the split mode's tolerances of the oracle's lists."""
    w = workloads.clustered(n=N, d=d, nq=NQ, C=C, seed=900 + d, label_mode="near")
    x, q = workloads.float32_inputs(w, 900 + d)
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))[:, :R]
    ix = DeviceIndex(x, w["labels"], C, chunk_rows=CHUNK, device="cuda")
    assert ix.storage == "f32x" and ix.d_pad == 768 and (ix.corpus32n is not None) == (d % 16 == 0)
    cls = T(classes.astype(np.int32))
    got_d, got_p, st = bucket_topk(ix, T(q), cls, k)
    assert int(st.item()) == 0
    ref_d, ref_p = O.bucket_lists(w["labels"], x, q, classes, R, k, C)
    assert O.compare_lists(ref_d, ref_p, got_d.cpu().numpy(), got_p.cpu().numpy(), atol=1e-5, tie=1e-6) == 0
    q64 = q.astype(np.float64)
    d64, p64, st64 = bucket_topk_f64(ix, T(q64), cls, k)
    assert int(st64.item()) == 0
    ref_d64, ref_p64 = O.bucket_lists(w["labels"], x, q64, classes, R, k, C)
    assert O.compare_lists(ref_d64, ref_p64, d64.cpu().numpy(), p64.cpu().numpy(), atol=1e-12,
                           tie=1e-12) == 0
