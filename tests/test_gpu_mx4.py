"""The 4-bit storage (storage "mx4": lmi_quantize_rows_mx4, prep_mx4_kernel,
scan3_mx4_kernel) against the numpy restatement of tests/mx4_cases.py, on the i8
ring's fixture shape: chunk_rows = 64, R = 2, buckets of (1, 31, 32, 33, 64, 65,
97, 0, 300) rows probed by (1, 31, 32, 33, 255, 256, 257, 4, 258) pairs, one
class outside [0, C).  These fixtures stop at 2 blocks a tile; the ring's steady state
(in-loop DMA, slot and norm-area wraps, the bound exchange) is in test_gpu_ring_long.py.

tol = d_pad * 2^-23: any fp32 summation order of n terms errs by at most
(n - 1) 2^-24 sum |terms|, sum |q^ y^| invq invy <= 1, and tol is twice that."""
import functools

import numpy as np
import pytest
import torch

import mx4_cases as M4
from li.index import DeviceIndex, Searcher, quantize_rows_mx4, scan_family

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 64, 65, 97, 0, 300)
PROBES = (1, 31, 32, 33, 255, 256, 257, 4, 258)
N, C, CHUNK, R = sum(SIZES), len(SIZES), 64, 2
NQ = (sum(PROBES) + 1) // R
TOL = 768 * 2.0 ** -23
DEV = "cuda"


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _classes():
    flat = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(PROBES)] + [np.array([C + 3], np.int32)])
    cls = np.ascontiguousarray(np.stack([flat[:NQ], flat[NQ:]], axis=1))
    assert flat.size == NQ * R and (cls[:, 0] != cls[:, 1]).all()
    return cls


def _lists(s, q, classes, k, **kw):
    _, d, pos, st = s.lists(None, _T(q), R, k, classes=_T(classes), lists16=k > 10, **kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    return d.cpu().numpy(), pos.cpu().numpy()


def _restate(x, q, ix):
    vy, vq = M4.quantize(x[ix.layout.order]), M4.quantize(q)
    return vq[3], vq[2], vy[3], vy[2]


# ---- 1. the quantiser, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("d", [768, 740])
def test_quantiser_bits(d, dtype):
    rng = np.random.default_rng(41 + d)
    x = rng.standard_normal((70, d)).astype(np.float16).astype(np.float32)
    x[1] = 0.0                                                    # a zero row
    x[2, 64:96] = 0.0                                             # a zero block
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
    x[3, :32] = 0.0
    x[3, 0] = 4.0                                                 # e_b = 0: t = v
    x[3, 1:8], x[3, 8:15] = ties, -ties
    x[4, 32:64] = 0.0
    x[4, 32], x[4, 33], x[4, 34] = 7.5, -6.5, 7.0                 # |t| in (6, 8): saturates
    x[5, 96:128] = 2.0 ** -24                                     # fp16 subnormals
    x[6, 128:160] = 65504.0
    x[7, 160:192] = rng.choice([-65504.0, 2.0 ** -24, 0.0], 32)
    codes, scales, inv, _ = M4.quantize(x.astype(dtype))
    assert scales[3, 0] == 127 and scales[4, 12] == 127 and scales[2, 1] == 127 and scales[6, 2] == 140
    assert (codes[3, :4] == [0x06, 0x22, 0x44, 0x66]).all()       # 4, .25->0 | .75->1, 1.25->1 | 1.75->2, 2.5->2 | 3.5->4, 5->4
    assert (codes[4, 16:18] == [0xF7, 0x07]).all()
    got_c = torch.full((72, 384), 0xEE, dtype=torch.uint8, device=DEV)
    got_s = torch.full((72, 24), 0xEE, dtype=torch.uint8, device=DEV)
    got_i = torch.full((72,), -1.0, dtype=torch.float32, device=DEV)
    dst = torch.from_numpy(rng.permutation(72)[:70].astype(np.int64)).to(DEV)
    quantize_rows_mx4(_T(x.astype(dtype)), 768, got_c, got_s, got_i, dst_rows=dst)
    torch.cuda.synchronize()
    at = dst.cpu().numpy()
    assert np.array_equal(got_c.cpu().numpy()[at], codes)
    assert np.array_equal(got_s.cpu().numpy()[at], scales)
    assert np.array_equal(got_i.cpu().numpy()[at].view(np.uint32), inv.view(np.uint32))
    rest = np.setdiff1d(np.arange(72), at)
    assert (got_c.cpu().numpy()[rest] == 0xEE).all() and (got_i.cpu().numpy()[rest] == -1.0).all()


# ---- 2. lists against float64 ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(d):
    rng = np.random.default_rng(7684 + d)
    x = rng.standard_normal((N, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    classes = _classes()
    got = np.bincount(classes[(classes >= 0) & (classes < C)], minlength=C)
    assert tuple(got) == PROBES and ((classes < 0) | (classes >= C)).sum() == 1
    s = Searcher(DeviceIndex(x, labels, C, ids=ids, chunk_rows=CHUNK, device=DEV, storage="mx4"), None)
    dist = M4.distances64(*_restate(x, q, s.index))
    dist.setflags(write=False)
    return dict(x=x, q=q, classes=classes, s=s, dist=dist)


def _check_lists(got_d, got_p, dist, off, classes, k):
    """Every pair: ascending by (distance, position); every distance within TOL of
    its position's float64 one; no row left out more than 2 TOL below the last entry."""
    for i in range(classes.shape[0]):
        for r in range(classes.shape[1]):
            c, dl, pl = int(classes[i, r]), got_d[i, r], got_p[i, r]
            rows = np.arange(off[c], off[c + 1]) if 0 <= c < len(off) - 1 else np.arange(0)
            n = min(k, rows.size)
            assert (pl[n:] == -1).all() and np.isinf(dl[n:]).all() and (pl[:n] >= 0).all(), (i, r)
            assert np.isin(pl[:n], rows).all() and np.unique(pl[:n]).size == n, (i, r)
            key = list(zip(dl[:n].tolist(), pl[:n].tolist()))
            assert key == sorted(key), (i, r)
            assert (np.abs(dl[:n].astype(np.float64) - dist[i, pl[:n]]) <= TOL).all(), (i, r)
            out = np.setdiff1d(rows, pl[:n])
            if out.size:
                assert dist[i, out].min() >= float(dl[n - 1]) - 2 * TOL, (i, r)


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("d", [768, 740])
def test_lists_against_float64(d, k):
    f = _fixture(d)
    ix = f["s"].index
    assert ix.storage == "mx4" and ix.d_pad == 768 and scan_family(ix, k, lists16=k > 10) == "ring8-mx4"
    got_d, got_p = _lists(f["s"], f["q"], f["classes"], k)
    _check_lists(got_d, got_p, f["dist"], ix.layout.bucket_off, f["classes"], k)
    assert np.isfinite(got_d[f["classes"] == 8]).all() and np.isinf(got_d[f["classes"] == 7]).all()


def test_search_and_phases_run_on_the_lists():
    """search (exact semantics, a stop rule's dropped probes) and the PLAN / SCAN /
    MERGE phases give the lists of the one call."""
    from li import _lib
    from li.index import bucket_topk
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
SAME = (3, 9, 60, 64, 70, 127, 128, 130, 190, 200, 255, 256, 257, 300, 319, 320, 321, 350, 382, 383)


def _exact_inputs(k, sizes, same, chunk):
    """Grid-valued rows and queries (the codes hold them exactly, the sums are exact
    in float32) in two buckets of `sizes` rows; the 20 rows `same` of bucket 0 are
    equal and query 0 is twice them.  Every list bit for bit against distances32."""
    rng = np.random.default_rng(4410)
    d, nq = 768, 40
    same = np.asarray(same)
    n = sum(sizes)

    def grid(m):
        v = rng.choice(M4.E2M1, (m, d)) * rng.choice([-1.0, 1.0], (m, d))
        v.reshape(m, 24, 32)[:, :, 0] = rng.choice([4.0, -4.0, 6.0, -6.0], (m, 24))   # one exponent a vector
        return (v * 2.0 ** rng.integers(-3, 4, (m, 1))).astype(np.float32)
    x, q = grid(n), grid(nq)
    labels = np.repeat(np.arange(2), sizes).astype(np.int64)
    assert same.size == 20
    x[same] = x[same[0]]
    q[0] = x[same[0]] * 2.0
    classes = np.tile(np.array([[0, 1]], np.int32), (nq, 1))
    s = Searcher(DeviceIndex(x, labels, 2, chunk_rows=chunk, device=DEV, storage="mx4"), None)
    assert np.array_equal(s.index.layout.order, np.arange(n))
    vq, iq, vy, iy = _restate(x, q, s.index)
    assert np.array_equal(vy, x) and np.array_equal(vq, q)        # the codes hold the inputs exactly
    dist = M4.distances32(vq, iq, vy, iy)
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
    assert np.unique(np.array(SAME) // CHUNK).size == 6
    _exact_inputs(k, (384, 33), SAME, CHUNK)


# ---- 4. re-rank -----------------------------------------------------------------------------------
def test_rerank_equals_the_fp16_float64_lists():
    d = 768
    rng = np.random.default_rng(4420)
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
    ix4 = ix16.quantized(storage="mx4", keep_rows=True)
    assert ix4.storage == "mx4" and ix4.rows16 is ix16.corpus
    xs, qs = x[ix16.layout.order].astype(np.float64), q.astype(np.float64)
    d64 = 1.0 - (qs @ xs.T) / np.linalg.norm(qs, axis=1)[:, None] / np.linalg.norm(xs, axis=1)[None, :]
    d4 = M4.distances64(*_restate(x.astype(np.float32), q.astype(np.float32), ix4))
    off = ix16.layout.bucket_off
    for i in range(NQ):                                           # every pair: float64 top 10 inside mx4 top 16
        for c in classes[i]:
            if 0 <= c < C:
                rows = np.arange(off[c], off[c + 1])
                top10 = rows[np.lexsort((rows, d64[i, rows]))][:10]
                top16 = rows[np.lexsort((rows, d4[i, rows]))][:16]
                assert np.isin(top10, top16).all(), (i, c)
    _, rd, rp, st = Searcher(ix4, None).lists(None, _T(q), R, 10, classes=_T(classes), dist="f64", rerank=16)
    _, fd, fp, st2 = Searcher(ix16, None).lists(None, _T(q), R, 10, classes=_T(classes), dist="f64")
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(st2.item()) == 0
    assert torch.equal(rp, fp) and torch.equal(rd.view(torch.int64), fd.view(torch.int64))
