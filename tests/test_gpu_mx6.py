"""The 6-bit storage (storage "mx6": lmi_quantize_rows_mx6, prep_mx6_kernel,
scan3_mx6_kernel) against the numpy restatement of tests/mx6_cases.py, on the i8
ring's fixture shape: chunk_rows = 64, R = 2, buckets of (1, 31, 32, 33, 64, 65,
97, 0, 300) rows probed by (1, 31, 32, 33, 255, 256, 257, 4, 258) pairs, one
class outside [0, C).  TOL = d_pad * 2^-23 as derived in test_gpu_mx4.py.
These fixtures stop at 2 blocks a tile; the ring's steady state (in-loop DMA, slot
and norm-area wraps, the bound exchange) is in test_gpu_ring_long.py."""
import functools

import numpy as np
import pytest
import torch

import mx6_cases as M6
from li.index import DeviceIndex, Searcher, bucket_topk, quantize_rows_mx6, scan_family
from test_gpu_mx4 import C, CHUNK, DEV, N, NQ, R, SAME, SIZES, TOL, _T, _check_lists, _classes, _lists

pytestmark = pytest.mark.gpu


def _restate(x, q, ix):
    vy, vq = M6.quantize(x[ix.layout.order]), M6.quantize(q)
    return vq[3], vq[2], vy[3], vy[2]


# ---- 1. the quantiser, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("d", [768, 740])
def test_quantiser_bits(d, dtype):
    rng = np.random.default_rng(61 + d)
    x = rng.standard_normal((70, d)).astype(np.float16).astype(np.float32)
    x[1] = 0.0                                                    # a zero row
    x[2, 64:96] = 0.0                                             # a zero block
    ties = ((M6.E2M3[:-1] + M6.E2M3[1:]) / 2).astype(np.float32)  # all 31 of the grid, 0.0625 .. 7.25
    x[3, 0], x[3, 32] = 4.0, -4.0                                 # e_b = 0: t = v
    x[3, 1:32], x[3, 33:64] = ties, -ties
    x[4, 32:64] = 0.0
    x[4, 32], x[4, 33], x[4, 34] = 7.75, -7.625, 7.9              # |t| in (7.5, 8): saturates
    x[5, 96:128] = 2.0 ** -24                                     # fp16 subnormals
    x[6, 128:160] = 65504.0
    x[7, 160:192] = rng.choice([-65504.0, 2.0 ** -24, 0.0], 32)
    codes, scales, inv, _ = M6.quantize(x.astype(dtype))
    assert scales[3, 0] == 127 and scales[3, 12] == 127 and scales[4, 12] == 127 and scales[2, 1] == 127
    assert scales[6, 2] == 140
    assert (codes[3, :3] == [0x18, 0x20, 0x08]).all()             # 4 | .0625 -> 0 | .1875 -> .25 | .3125 -> .25
    assert (codes[3, 24:27] == [0x38, 0x20, 0x8A]).all()          # the same negated: no sign on the zero
    assert (codes[4, 24:27] == [0xDF, 0xFF, 0x01]).all()          # 7.5, -7.5, 7.5, 0
    got_c = torch.full((72, 576), 0xEE, dtype=torch.uint8, device=DEV)
    got_s = torch.full((72, 24), 0xEE, dtype=torch.uint8, device=DEV)
    got_i = torch.full((72,), -1.0, dtype=torch.float32, device=DEV)
    dst = torch.from_numpy(rng.permutation(72)[:70].astype(np.int64)).to(DEV)
    quantize_rows_mx6(_T(x.astype(dtype)), 768, got_c, got_s, got_i, dst_rows=dst)
    torch.cuda.synchronize()
    at = dst.cpu().numpy()
    assert np.array_equal(got_c.cpu().numpy()[at], codes)
    assert np.array_equal(got_s.cpu().numpy()[at], scales)
    assert np.array_equal(got_i.cpu().numpy()[at].view(np.uint32), inv.view(np.uint32))
    rest = np.setdiff1d(np.arange(72), at)
    assert (got_c.cpu().numpy()[rest] == 0xEE).all() and (got_s.cpu().numpy()[rest] == 0xEE).all()
    assert (got_i.cpu().numpy()[rest] == -1.0).all()


# ---- 2. lists against float64 ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(d):
    rng = np.random.default_rng(7686 + d)
    x = rng.standard_normal((N, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    s = Searcher(DeviceIndex(x, labels, C, ids=ids, chunk_rows=CHUNK, device=DEV, storage="mx6"), None)
    dist = M6.distances64(*_restate(x, q, s.index))
    dist.setflags(write=False)
    return dict(x=x, q=q, classes=_classes(), s=s, dist=dist)


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("d", [768, 740])
def test_lists_against_float64(d, k):
    f = _fixture(d)
    ix = f["s"].index
    assert ix.storage == "mx6" and ix.d_pad == 768 and scan_family(ix, k, lists16=k > 10) == "ring8-mx6"
    got_d, got_p = _lists(f["s"], f["q"], f["classes"], k)
    _check_lists(got_d, got_p, f["dist"], ix.layout.bucket_off, f["classes"], k)
    assert np.isfinite(got_d[f["classes"] == 8]).all() and np.isinf(got_d[f["classes"] == 7]).all()


def test_search_and_phases_run_on_the_lists():
    """search (exact semantics, a stop rule's dropped probes) and the PLAN / SCAN /
    MERGE phases give the lists of the one call."""
    from li import _lib
    f = _fixture(768)
    s, q, cls = f["s"], _T(f["q"]), f["classes"].copy()
    whole = bucket_topk(s.index, q, _T(cls), 10)
    out = (torch.empty_like(whole[0]), torch.empty_like(whole[1]), torch.zeros_like(whole[2]))
    for ph in (_lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_MERGE):
        bucket_topk(s.index, q, _T(cls), 10, out=out, phases=ph)
    torch.cuda.synchronize()
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])
    cls[::3, 1] = -1                                              # probes a stop rule dropped
    d, a = s.search(None, q, R, k=10, classes=_T(cls), semantics="exact")
    ld, lp = _lists(s, f["q"], cls, 10)
    best = np.sort(np.where(lp.reshape(NQ, -1) >= 0, ld.reshape(NQ, -1), np.inf), axis=1)[:, :10]
    assert np.array_equal(np.where(np.isinf(best), 10000.0, best.astype(np.float64)), d)
    d2, a2 = s.search(None, q, R, k=10, classes=_T(cls), semantics="reference")
    assert d2.shape == d.shape and (a2[cls[:, 0] == 8] > 0).all()


# ---- 3. exact inputs, bit for bit -----------------------------------------------------------------
def _exact_inputs(k, sizes, same, chunk):
    """Grid-valued rows and queries (the codes hold them exactly, the sums are exact
    in float32) in two buckets of `sizes` rows; the 20 rows `same` of bucket 0 are
    equal and query 0 is twice them.  Every list bit for bit against distances32."""
    rng = np.random.default_rng(6610)
    d, nq = 768, 40
    same = np.asarray(same)
    n = sum(sizes)

    def grid(m):
        v = rng.choice(M6.E2M3, (m, d)) * rng.choice([-1.0, 1.0], (m, d))
        v.reshape(m, 24, 32)[:, :, 0] = rng.choice(M6.E2M3[24:], (m, 24)) * rng.choice([-1.0, 1.0], (m, 24))
        return (v * 2.0 ** rng.integers(-3, 4, (m, 1))).astype(np.float32)    # one exponent a vector
    x, q = grid(n), grid(nq)
    labels = np.repeat(np.arange(2), sizes).astype(np.int64)
    assert same.size == 20
    x[same] = x[same[0]]
    q[0] = x[same[0]] * 2.0
    classes = np.tile(np.array([[0, 1]], np.int32), (nq, 1))
    s = Searcher(DeviceIndex(x, labels, 2, chunk_rows=chunk, device=DEV, storage="mx6"), None)
    assert np.array_equal(s.index.layout.order, np.arange(n))
    vq, iq, vy, iy = _restate(x, q, s.index)
    assert np.array_equal(vy, x) and np.array_equal(vq, q)        # the codes hold the inputs exactly
    dist = M6.distances32(vq, iq, vy, iy)                         # (asserts the sums exact in float32)
    order = np.lexsort((np.arange(sizes[0]), dist[0, :sizes[0]]))[:k]
    assert np.array_equal(order, same[:k])                        # the tie straddles the list's bound
    got_d, got_p = _lists(s, q, classes, k)
    off = s.index.layout.bucket_off
    for i in range(nq):
        for r in range(R):
            rows = np.arange(off[r], off[r + 1])
            best = rows[np.lexsort((rows, dist[i, rows]))][:k]
            assert np.array_equal(got_p[i, r, :best.size], best), (i, r)
            assert np.array_equal(got_d[i, r, :best.size].view(np.uint32), dist[i, best].view(np.uint32)), (i, r)


@pytest.mark.parametrize("k", [10, 16])
def test_exact_inputs_bit_for_bit(k):
    """Pins the fragment's bit order, the scale order and op_sel: any other reading
    of the stored bytes gives other sums."""
    assert np.unique(np.array(SAME) // CHUNK).size == 6
    _exact_inputs(k, (384, 33), SAME, CHUNK)


# ---- 4. re-rank -----------------------------------------------------------------------------------
def test_rerank_equals_the_fp16_float64_lists():
    d = 768
    rng = np.random.default_rng(4420)                             # mx4's clustered fixture
    g = rng.standard_normal(d)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    x = rng.standard_normal((N, d))
    for c in range(C):
        rows = np.flatnonzero(labels == c)
        if rows.size >= 16:
            x[rows[:12]] = g + 0.1 * rng.standard_normal((12, d))
    x = x.astype(np.float16)
    q = (g + 0.1 * rng.standard_normal((NQ, d))).astype(np.float16)
    classes = _classes()
    ix16 = DeviceIndex(x, labels, C, chunk_rows=CHUNK, device=DEV, storage="f16")
    ix6 = ix16.quantized(storage="mx6", keep_rows=True)
    assert ix6.storage == "mx6" and ix6.rows16 is ix16.corpus
    xs, qs = x[ix16.layout.order].astype(np.float64), q.astype(np.float64)
    d64 = 1.0 - (qs @ xs.T) / np.linalg.norm(qs, axis=1)[:, None] / np.linalg.norm(xs, axis=1)[None, :]
    d6 = M6.distances64(*_restate(x.astype(np.float32), q.astype(np.float32), ix6))
    off = ix16.layout.bucket_off
    for i in range(NQ):                                           # every pair: float64 top 10 inside mx6 top 16
        for c in classes[i]:
            if 0 <= c < C:
                rows = np.arange(off[c], off[c + 1])
                top10 = rows[np.lexsort((rows, d64[i, rows]))][:10]
                top16 = rows[np.lexsort((rows, d6[i, rows]))][:16]
                assert np.isin(top10, top16).all(), (i, c)
    _, rd, rp, st = Searcher(ix6, None).lists(None, _T(q), R, 10, classes=_T(classes), dist="f64", rerank=16)
    _, fd, fp, st2 = Searcher(ix16, None).lists(None, _T(q), R, 10, classes=_T(classes), dist="f64")
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(st2.item()) == 0
    assert torch.equal(rp, fp) and torch.equal(rd.view(torch.int64), fd.view(torch.int64))
