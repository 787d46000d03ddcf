"""The scan (K2), its float64 refinement and Searcher.search on rows and
queries that are not unit length.  The search's contract is the reference's:
1 - cosine of whatever it is given, with sklearn's rule that a norm below
10 eps(dtype) counts as 1 -- eps of float32 in the float32 mode, of float64
in the float64 mode.  Every other GPU test scans L2-normalised vectors.

  A  rows and queries times a power of two drawn per row: the oracle's lists,
     and bit for bit the lists of the unit workload in the same call
     (d = fma(-dot, invq * inv_y, 1) is built from operations that commute
     with such a scale while nothing leaves the normal range);
  B  rows scaled down until most (2^-10) or all (2^-17) components are fp16
     subnormals: the MFMAs must keep them;
  C  rows and queries between the two zero-norm rules (norm in [10 eps64,
     10 eps32)): each mode follows its own rule;
  D  DeviceIndex.inv_norm64, which C's float64 cases need, through everything
     that permutes or extends inv_norm.

Shapes, comparator, tolerances and the strict-id rule are
test_gpu_scan_widths.py's (_check); the oracle is O.bucket_lists on float64
copies of the stored values (float32 arrays where the float32 rule is the
subject).  Strict-id caps, from the oracle on the CPU (share of exempt rows,
"skewed"): d 768 seed 1668 unscaled 2.4 / 4.2 / 9.0 % at k = 10 / 12 / 16
(bound 2^-15) and 28.5 % at k = 40, which is over the cap of 10 %: that case
has no strict-id rule; 2^-10: 3.1 / 8.0 % at k = 10 / 16; 2^-17: 2.4 / 5.2 %;
d 96 and 800, fp32 math: 6.6 % and 24.0 % at k = 40 against 50 %."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li import _lib
from li.index import (DeviceIndex, DeviceRouter, Searcher, bucket_topk, bucket_topk_f64,
                      refine_eps)
from test_gpu_scan_widths import C, CHUNK, F16, F32, N, NQ, R, SEEDS as WIDTH_SEEDS, T, _check, _pad

pytestmark = pytest.mark.gpu

SEED = {768: 1668, 96: WIDTH_SEEDS[96], 800: WIDTH_SEEDS[800]}
EPS32, EPS64 = 10 * float(np.finfo(np.float32).eps), 10 * float(np.finfo(np.float64).eps)
F64 = lambda a: np.asarray(a).astype(np.float64)  # noqa: E731
TOL64 = dict(atol=1e-12, tie=1e-12)


@contextlib.contextmanager
def _env(name):
    """The launch choice's switch `name` for the calls inside."""
    if name:
        os.environ[name] = "1"
    _lib.load().lmi_config_reload()
    try:
        yield
    finally:
        if name:
            os.environ.pop(name, None)
        _lib.load().lmi_config_reload()


@functools.lru_cache(maxsize=None)
def _unit(d, mode="skewed"):
    w = workloads.clustered(n=N, d=d, nq=NQ, C=C, seed=SEED[d], label_mode=mode)
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    return w, np.ascontiguousarray(classes[:, :R])


def _cls(classes):
    return T(classes.astype(np.int32))


def _index(x, labels, storage="f16", **kw):
    return DeviceIndex(x, labels, C, storage=storage, chunk_rows=CHUNK, device="cuda", **kw)


def _lists(x, q, d, mode, depth):
    w, classes = _unit(d, mode)
    return O.bucket_lists(w["labels"], x, q, classes, R, depth, C)


# ---------------------------------------------------------------------------
# A. power-of-two scales
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scaled(d, storage):
    """Rows and queries times 2^e, one exponent per row: fp16 storage [0, 14]
    (max |x| 2816 at d 768); storage "f32" rows [-16, 40], queries [-16, 20]
    (the smallest row norm 1.5e-5 stays above the float32 rule)."""
    w, _ = _unit(d)
    rng = np.random.default_rng(SEED[d] + 7)
    lo, hi, qhi = (0, 14, 14) if storage == "f16" else (-16, 40, 20)
    xs, _ = workloads.pow2_scaled(w["x"], rng, lo, hi)
    qs, eq = workloads.pow2_scaled(w["q"], rng, lo, qhi)
    if storage == "f16":
        assert np.array_equal(xs.astype(np.float16).astype(np.float32), xs)
        assert np.array_equal(qs.astype(np.float16).astype(np.float32), qs)
    assert np.linalg.norm(F64(xs), axis=1).min() > 10 * EPS32
    return xs, qs, eq


@functools.lru_cache(maxsize=None)
def _ref_a(d, storage, scaled):
    w, _ = _unit(d)
    x, q = _scaled(d, storage)[:2] if scaled else (w["x"], w["q"])
    return _lists(F64(x), F64(q), d, "skewed", 41)


@functools.lru_cache(maxsize=None)
def _index_a(d, storage, scaled):
    w, _ = _unit(d)
    ix = _index(_scaled(d, storage)[0] if scaled else w["x"], w["labels"], storage)
    assert ix.storage == storage and ix.inv_norm64 is None
    return ix


A_CASES = [
    (768, "f16", F16, 10, None), (768, "f16", F16, 12, None),    # 8-wave ring, 10- and 15-entry lists
    (768, "f16", F16, 16, None),                                 # 4-wave ring
    (768, "f16", F16, 40, None),                                 # bound + collect
    (768, "f16", F16, 40, "LMI_WIDE_PASSES"),                    # the lower-bound passes
    (768, "f16", F16, 10, "LMI_SCAN_V1"), (768, "f16", F16, 16, "LMI_SCAN_V1"),  # general, fp16 math
    (768, "f16", F32, 16, None),                                 # general, fp16 rows x fp32 queries
    (96, "f32", F32, 10, None), (96, "f32", F32, 40, None),      # general fp32, trailing block
    (800, "f32", F32, 10, None), (800, "f32", F32, 40, None),
]


def _id_a(c):
    d, storage, qmode, k, env = c
    return f"d{d}-{storage}-{'qf16' if qmode == F16 else 'qf32'}-k{k}" + (f"-{env}" if env else "")


def _same_bits(a, b):
    return torch.equal(a[0].view(torch.int64 if a[0].dtype == torch.float64 else torch.int32),
                       b[0].view(torch.int64 if b[0].dtype == torch.float64 else torch.int32)) and \
        torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", A_CASES, ids=_id_a)
def test_pow2_scale_float32(case):
    """(1) the scaled run matches the oracle; (2) its distances (bit
    patterns) and positions are the unit run's of the same call."""
    d, storage, qmode, k, env = case
    w, classes = _unit(d)
    qs = _scaled(d, storage)[1]
    ref_u, ref_s = _ref_a(d, storage, False), _ref_a(d, storage, True)
    assert np.array_equal(ref_s[1], ref_u[1])        # the oracle does not see the scale
    f16math = storage == "f16" and qmode == F16
    cap = None if (d, k) == (768, 40) else (0.10 if f16math else 0.50)
    with _env(env):
        got_u = bucket_topk(_index_a(d, storage, False), T(w["q"]), _cls(classes), k, qmode=qmode)
        got_s = bucket_topk(_index_a(d, storage, True), T(qs), _cls(classes), k, qmode=qmode)
        torch.cuda.synchronize()
    _check("scale " + _id_a(case), (ref_s[0][..., :k + 1], ref_s[1][..., :k + 1]), got_s, k, f64=False,
           bound=2 * refine_eps(_pad(d), f16math), cap=cap)
    assert int(got_u[2].item()) == 0
    assert _same_bits(got_s, got_u), "the scaled lists differ from the unit run's"


@pytest.mark.parametrize("q64", [False, True], ids=["q32", "q64"])
def test_pow2_scale_float64(q64):
    """bucket_topk_f64 at k = 10 on the fp16 case, float32 queries and float64
    queries times 2^e: the oracle within 1e-12, the unit run's bits, and the
    unit run's fallback count (identical d32 give identical bands)."""
    w, classes = _unit(768)
    xs, qs, eq = _scaled(768, "f16")
    qu = w["q"]
    if q64:
        qu = workloads.float64_inputs(w, SEED[768])[1]
        qs = np.ldexp(qu, eq[:, None])
    ref_u = _lists(F64(w["x"]), F64(qu), 768, "skewed", 11)
    ref_s = _lists(F64(xs), F64(qs), 768, "skewed", 11)
    assert np.array_equal(ref_s[1], ref_u[1])
    got_u = bucket_topk_f64(_index_a(768, "f16", False), T(qu), _cls(classes), 10, fallback_count=True)
    got_s = bucket_topk_f64(_index_a(768, "f16", True), T(qs), _cls(classes), 10, fallback_count=True)
    _check(f"scale f64 {'q64' if q64 else 'q32'}", ref_s, got_s[:3], 10, f64=True, bound=2e-12, cap=0.10)
    assert int(got_u[2].item()) == 0
    print(f"[scale] fallback pairs: unit {got_u[3]}, scaled {got_s[3]}")
    assert _same_bits(got_s, got_u) and got_s[3] == got_u[3]


@pytest.mark.parametrize("dist", ["f32", "f64"])
def test_search_and_stream_on_scaled_inputs(dist):
    w, classes = _unit(768)
    xs, qs, _ = _scaled(768, "f16")
    s = Searcher(_index_a(768, "f16", True), DeviceRouter(w["layers"], device="cuda"))
    x, q = (F64(xs), F64(qs)) if dist == "f64" else (xs, qs)
    full = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    ref_d, ref_a = O.search_direct(w["labels"], np.arange(1, N + 1), x, q, full, n_buckets=R, k=10,
                                   use_threshold=True)
    d0, a0 = s.search(T(w["qn"]), T(qs), R, k=10, use_threshold=True, dist=dist)
    assert O.compare_lists(ref_d, ref_a, d0, a0, **(TOL64 if dist == "f64" else {})) == 0
    with s.streamed(w["qn"], qs, R, k=10, dist=dist) as st:
        d1, a1 = st.step()
    np.testing.assert_array_equal(d1, d0)
    np.testing.assert_array_equal(a1, a0)


# ---------------------------------------------------------------------------
# B. subnormal components
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sub(d, mode, s):
    w, _ = _unit(d, mode)
    x, q = workloads.subnormal_scaled(w, s)
    ix = _index(x, w["labels"])
    assert ix.inv_norm64 is None
    return x, q, ix, _lists(F64(x), F64(q), d, mode, 17)


def _b_cases():
    out = [(768, mode, s, k, f64, None) for s in (10, 17) for mode in ("skewed", "near")
           for k, f64 in ((10, False), (16, False), (10, True))]
    return out + [(96, mode, 10, k, f64, "LMI_SCAN_V1") for mode in ("skewed", "near")
                  for k, f64 in ((10, False), (16, False), (10, True))]


def _id_b(c):
    d, mode, s, k, f64, env = c
    return f"d{d}-{mode}-s{s}-k{k}-{'f64' if f64 else 'f32'}" + (f"-{env}" if env else "")


@pytest.mark.parametrize("case", _b_cases(), ids=_id_b)
def test_subnormal_components_are_kept(case):
    """x16 = (x * 2^-s).astype(float16), every other query the same: at d 768
    at least 90 % (s = 10) and all (s = 17) of the components are fp16
    subnormals; at d 96 (unit components of ~0.1, s = 10: 1e-4 against the
    smallest normal 6.1e-5) at least 40 %.  A flush of such operands moves
    the distances by far more than the tolerances."""
    d, mode, s, k, f64, env = case
    w, classes = _unit(d, mode)
    x, q, ix, ref = _sub(d, mode, s)
    share = min(workloads.subnormal_share(x), workloads.subnormal_share(q[::2]))
    assert share == 1.0 if s == 17 else share >= (0.9 if d == 768 else 0.4), share
    assert min(np.linalg.norm(F64(x), axis=1).min(), np.linalg.norm(F64(q), axis=1).min()) > EPS32
    ref = (ref[0][..., :k + 1], ref[1][..., :k + 1])
    cap = 0.10 if mode == "skewed" else None
    with _env(env):
        if f64:
            got = bucket_topk_f64(ix, T(q), _cls(classes), k)
        else:
            got = bucket_topk(ix, T(q), _cls(classes), k, qmode=F16)
        torch.cuda.synchronize()
    _check("sub " + _id_b(case), ref, got, k, f64=f64,
           bound=2e-12 if f64 else 2 * refine_eps(_pad(d), True), cap=cap)


# ---------------------------------------------------------------------------
# C. between the two zero-norm rules
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted():
    """The planted-row workload and what the oracles alone say about it."""
    w = workloads.clustered(n=N, d=768, nq=NQ, C=C, seed=1668, label_mode="router")
    full = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    classes = np.ascontiguousarray(full[:, :R])
    x, planted = workloads.planted_low_norm(w, classes, R, C)
    order, _ = O.layout(w["labels"], C)
    inv = np.empty(N, np.int64)
    inv[order] = np.arange(N)
    m = planted >= 0
    pos = np.where(m, inv[np.maximum(planted, 0)], -1)
    nrm = np.linalg.norm(F64(x[planted[m]]), axis=1)
    assert m.sum() >= 100 and nrm.min() >= EPS64 and nrm.max() < EPS32
    return dict(w=w, full=full, classes=classes, x=x, rows=planted, m=m, pos=pos)


def _planted_ref64(x64, q64):
    """The float64 oracle's lists, k + 1 = 11 deep, after asserting that every
    planted row is entry 0 of its pair."""
    p = _planted()
    rd, rp = O.bucket_lists(p["w"]["labels"], x64, q64, p["classes"], R, 11, C)
    assert np.array_equal(rp[..., 0][p["m"]], p["pos"][p["m"]])
    return rd, rp


@functools.lru_cache(maxsize=None)
def _planted_index(storage="f16"):
    p = _planted()
    ix = _index(p["x"], p["w"]["labels"], storage)
    assert ix.inv_norm64 is not None
    return ix


def _planted_first(got_p):
    p = _planted()
    return np.array_equal(got_p[..., 0][p["m"]], p["pos"][p["m"]])


def test_planted_rows_float32_rule():
    """bucket_topk and Searcher.search(dist='f32') score the planted rows with
    norm 1, as the reference's float32 branch does: none is in a top-10."""
    p = _planted()
    w, x = p["w"], p["x"]
    rd, rp = O.bucket_lists(w["labels"], x, w["q"], p["classes"], R, 10, C)
    assert rd.dtype == np.float32 and not np.isin(rp, p["pos"][p["m"]]).any()
    ix = _planted_index()
    d, pos, st = bucket_topk(ix, T(w["q"]), _cls(p["classes"]), 10)
    assert int(st.item()) == 0
    assert O.compare_lists(rd, rp, d.cpu().numpy(), pos.cpu().numpy()) == 0
    s = Searcher(ix, DeviceRouter(w["layers"], device="cuda"))
    ref_d, ref_a = O.search_direct(w["labels"], np.arange(1, N + 1), x, w["q"], p["full"], n_buckets=R,
                                   k=10, use_threshold=True)
    got_d, got_a = s.search(T(w["qn"]), T(w["q"]), R, k=10, use_threshold=True, dist="f32")
    assert O.compare_lists(ref_d, ref_a, got_d, got_a) == 0


@pytest.mark.parametrize("q64", [False, True], ids=["q32", "q64"])
def test_planted_rows_float64_lists(q64):
    p = _planted()
    w = p["w"]
    q = workloads.float64_inputs(w, 1668)[1] if q64 else w["q"]
    ref = _planted_ref64(F64(p["x"]), F64(q))
    got = bucket_topk_f64(_planted_index(), T(q), _cls(p["classes"]), 10)
    _check(f"planted f64 {'q64' if q64 else 'q32'}", ref, got, 10, f64=True, bound=2e-12, cap=0.10)
    assert _planted_first(got[1].cpu().numpy())


def test_planted_rows_float64_search_and_stream():
    p = _planted()
    w, x = p["w"], p["x"]
    _planted_ref64(F64(x), F64(w["q"]))
    ref_d, ref_a = O.search_direct(w["labels"], np.arange(1, N + 1), F64(x), F64(w["q"]), p["full"],
                                   n_buckets=R, k=10, use_threshold=True)
    s = Searcher(_planted_index(), DeviceRouter(w["layers"], device="cuda"))
    cls, _, pos, st = s.lists(T(w["qn"]), T(w["q"]), R, 10, dist="f64")
    assert int(st.item()) == 0 and np.array_equal(cls.cpu().numpy(), p["classes"])
    assert _planted_first(pos.cpu().numpy())
    got = {}
    for on in ("device", "host"):
        got[on] = s.search(T(w["qn"]), T(w["q"]), R, k=10, use_threshold=True, dist="f64", replay_on=on)
        assert O.compare_lists(ref_d, ref_a, *got[on], **TOL64) == 0, on
    with s.streamed(w["qn"], w["q"], R, k=10, dist="f64") as stream:
        d1, a1 = stream.step()
    np.testing.assert_array_equal(d1, got["device"][0])
    np.testing.assert_array_equal(a1, got["device"][1])


def test_planted_rows_float64_corpus():
    """The same through corpus64: float64_inputs of the workload with the
    planted rows at norm 1e-9, still above the float64 rule.  Their float32
    rounding is not fp16-exact, so the rows are stored as float32 (storage
    'f32' asked for: 'auto' would pick the split mode, which is not the
    subject here)."""
    p = _planted()
    w = p["w"]
    x64 = workloads.float64_inputs(dict(x=p["x"], q=w["q"]), 1668)[0]
    x64[p["rows"][p["m"]]] *= 1e-3
    nrm = np.linalg.norm(x64[p["rows"][p["m"]]], axis=1)
    assert nrm.min() >= EPS64 and nrm.max() < 2e-9
    ref = _planted_ref64(x64, F64(w["q"]))
    ix = _index(x64, w["labels"], "f32")
    assert ix.corpus64 is not None and ix.inv_norm64 is not None
    got = bucket_topk_f64(ix, T(w["q"]), _cls(p["classes"]), 10)
    _check("planted corpus64", ref, got, 10, f64=True, bound=2e-12, cap=0.10)
    assert _planted_first(got[1].cpu().numpy())


def _small_queries(kind):
    """Every third query under the float32 rule: fp16 values at norm 1e-6,
    float64 values at norm 1e-9, float32 values at norm 1e-6."""
    p = _planted()
    q = F64(p["w"]["q"])
    t = 1e-9 if kind == "q64" else 1e-6
    q[::3] *= t / np.linalg.norm(q[::3], axis=1)[:, None]
    if kind == "q16":
        q = q.astype(np.float16).astype(np.float32)
    elif kind == "q32":
        q = q.astype(np.float32)
    else:
        q[1::3] *= 1.0 + 2e-10        # (no longer float32-exact: kept as float64 queries)
    nrm = np.linalg.norm(F64(q[::3]), axis=1)
    assert nrm.min() >= EPS64 and nrm.max() < EPS32
    return q


@pytest.mark.parametrize("kind", ["q16", "q64", "q32"])
def test_queries_under_the_float32_rule(kind):
    """Float64 mode: the float64 oracle's lists (the query normalised), status
    0; such a query's d32 are all ~1, so its pairs may take the fallback.
    Float32 mode: the float32 oracle, i.e. the query unnormalised."""
    p = _planted()
    w = p["w"]
    q = _small_queries(kind)
    ix = _planted_index("f32" if kind == "q32" else "f16")
    ref = O.bucket_lists(w["labels"], F64(p["x"]), F64(q), p["classes"], R, 11, C)
    q_f32 = q.astype(np.float32)
    r32 = O.bucket_lists(w["labels"], p["x"], q_f32, p["classes"], R, 10, C)
    assert r32[0].dtype == np.float32
    # (float64 queries at norm 1e-9 are not fp16 values: fp32 arithmetic, as Searcher.qmode picks)
    qmode = F32 if kind == "q64" else None
    got = bucket_topk_f64(ix, T(q), _cls(p["classes"]), 10, qmode=qmode, fallback_count=True)
    _check(f"small queries {kind} f64", ref, got[:3], 10, f64=True, bound=2e-12)
    print(f"[scale] small queries {kind}: {got[3]} of {NQ * R} pairs took the fallback")
    d, pos, st = bucket_topk(ix, T(q_f32), _cls(p["classes"]), 10, qmode=qmode)
    assert int(st.item()) == 0
    assert O.compare_lists(r32[0], r32[1], d.cpu().numpy(), pos.cpu().numpy()) == 0


def test_zero_vectors_in_float64_mode():
    """test_gpu_edges.py's zero rows and zero query with dist='f64': under
    either rule a zero norm counts as 1 and every such distance is exactly 1."""
    w = workloads.clustered(n=2000, nq=64, C=8, seed=31, label_mode="router")
    w["x"][::97] = 0.0
    w["q"][5] = 0.0
    ix = DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=CHUNK, device="cuda")
    assert ix.inv_norm64 is None
    s = Searcher(ix, DeviceRouter(w["layers"], device="cuda"))
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    rd, ra = O.search_direct(w["labels"], np.arange(1, 2001), F64(w["x"]), F64(w["q"]), classes,
                             n_buckets=3, k=10, use_threshold=True)
    d, a = s.search(T(w["qn"]), T(w["q"]), 3, k=10, use_threshold=True, dist="f64")
    assert O.compare_lists(rd, ra, d, a, **TOL64) == 0
    assert np.all(d[5] == 1.0)


# ---------------------------------------------------------------------------
# D. inv_norm64 through everything that permutes or extends inv_norm: carried,
# so that the table is the one of the index built from scratch
# ---------------------------------------------------------------------------
def _expected64(ix):
    """inv_norm64 recomputed on the host from the index's own stored rows."""
    x = ix.corpus.double().cpu().numpy()
    nrm = np.sqrt(np.einsum("ij,ij->i", x, x))
    low = (nrm >= EPS64) & (nrm < EPS32)
    inv = ix.inv_norm.cpu().numpy().copy()
    inv[low] = (1.0 / nrm[low]).astype(np.float32)
    return inv, int(low.sum())


def _same_tables(got, want):
    assert torch.equal(got.corpus, want.corpus) and torch.equal(got.inv_norm, want.inv_norm)
    assert (got.inv_norm64 is None) == (want.inv_norm64 is None)
    exp, n_low = _expected64(got)
    if got.inv_norm64 is None:
        assert n_low == 0
    else:
        assert n_low > 0 and torch.equal(got.inv_norm64, want.inv_norm64)
        assert np.array_equal(got.inv_norm64.cpu().numpy(), exp)
    return n_low


def _mixed():
    """Rows [0, 2000) of the unit workload and rows [2000, N) of the planted one."""
    p = _planted()
    cut = 2000
    assert (p["rows"][p["m"]] >= cut).any() and (p["rows"][p["m"]] < cut).any()
    return p, cut, np.arange(1, N + 1, dtype=np.int64)


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
@pytest.mark.parametrize("holder", ["batch", "index"])
def test_add_carries_inv_norm64(holder, inplace):
    """The batch brings the low-norm rows to an index without any (the
    ingest's LMI_STATUS_ROWS_LOW_NORM), or the index holds them and the batch
    brings none."""
    p, cut, ids = _mixed()
    lab = p["w"]["labels"]
    a, b = (p["w"]["x"], p["x"]) if holder == "batch" else (p["x"], p["w"]["x"])
    base = _index(a[:cut], lab[:cut], ids=ids[:cut], capacity=N if inplace else None)
    assert (base.inv_norm64 is None) == (holder == "batch")
    got = base.add(b[cut:], lab[cut:], ids[cut:], inplace=inplace)
    want = _index(np.concatenate([a[:cut], b[cut:]]), lab, ids=ids)
    assert _same_tables(got, want) > 0


@pytest.mark.parametrize("inplace", [False, True], ids=["copy", "inplace"])
def test_remove_carries_inv_norm64(inplace):
    p, _, ids = _mixed()
    lab, low = p["w"]["labels"], np.unique(p["rows"][p["m"]])
    gone = np.concatenate([low[::2], np.setdiff1d(np.arange(0, N, 11), low)])
    keep = np.setdiff1d(np.arange(N), gone)
    got = _index(p["x"], lab, ids=ids, capacity=N if inplace else None).remove(ids[gone], inplace=inplace)
    assert _same_tables(got, _index(p["x"][keep], lab[keep], ids=ids[keep])) == low.size - low[::2].size
    keep = np.setdiff1d(np.arange(N), low)
    got = _index(p["x"], lab, ids=ids).remove(ids[low])
    assert _same_tables(got, _index(p["x"][keep], lab[keep], ids=ids[keep])) == 0


def test_relabel_and_reserve_carry_inv_norm64():
    p, _, ids = _mixed()
    lab = p["w"]["labels"]
    base = _index(p["x"], lab, ids=ids)
    new_lab = (lab * 5 + np.arange(N)) % (C + 3)
    got = base.relabel(new_lab, C + 3)
    want = DeviceIndex(p["x"], new_lab, C + 3, ids=ids, storage="f16", chunk_rows=CHUNK, device="cuda")
    assert _same_tables(got, want) > 0
    res = base.reserve(N + 100)
    assert _same_tables(res, base) > 0 and res.inv_norm64.data_ptr() != base.inv_norm64.data_ptr()


def test_subcluster_and_stripes_carry_inv_norm64():
    """The sub-cluster reorder permutes the table with the rows, and a stripe
    holds the entries of its own rows: each equals the table recomputed from
    the rows where they now are, and the float64 lists are the oracle's."""
    p = _planted()
    w = p["w"]
    ref = _planted_ref64(F64(p["x"]), F64(w["q"]))
    sub = DeviceIndex(p["x"], w["labels"], C, chunk_rows=64, device="cuda", subcluster=True)
    assert sub.chunk_centroid is not None and not torch.equal(sub.gpos, _planted_index().gpos)
    exp, n_low = _expected64(sub)
    assert n_low == np.unique(p["rows"][p["m"]]).size
    assert np.array_equal(sub.inv_norm64.cpu().numpy(), exp)
    got = bucket_topk_f64(sub, T(w["q"]), _cls(p["classes"]), 10)
    _check("planted subcluster", ref, got, 10, f64=True, bound=2e-12, cap=0.10)
    total = 0
    for rank in range(2):
        ix = DeviceIndex(p["x"], w["labels"], C, chunk_rows=CHUNK, device="cuda", rank=rank, world=2)
        exp, k_low = _expected64(ix)
        assert k_low > 0 and np.array_equal(ix.inv_norm64.cpu().numpy(), exp)
        total += k_low
    assert total == n_low
