"""K3 (csrc/lmi_merge.hip) on synthetic lists against a numpy oracle, bit for
bit.  The lists real stripes produce are full, with distinct keys and disjoint
positions; these are not: short lists, all-empty rows, exact distance ties
across ranks (the distances come from a pool of a dozen values), positions up
to 2^31 - 1, one row, rows around the 256-thread block edge, k below and at the
register lists' lengths (10, 16), the first wide k (17) and the cap, and packed
buffers wider than the minimum with garbage in the pad words.

Oracle: per row, the G * k input entries ordered by (distance, position as
uint32, so -1 sorts last) with np.lexsort, the first k; empty slots are
(+inf, -1).

-0.0 and NaN are kept out of the pool on purpose: the narrow float32 kernel
orders distances by their f2ord bit pattern (-0.0 before +0.0, NaN by its
bits) while the float64 and the wide kernels compare with `<` (-0.0 == +0.0),
so the kernels would disagree among themselves on such inputs -- and the scan
writes neither value (its distances are 1 - cos rounded once, and rows past a
chunk's end never reach a list)."""
import numpy as np
import pytest
import torch

from li import _lib
from li.dist import packed_lists
from li.index import merge_topk

pytestmark = pytest.mark.gpu

KMAX = _lib.LMI_MAX_K_PASSES
GARBAGE = 0x5A5A5A5A
POOL32 = np.array([0.0, -1e-8, -3e-8, 1e-8, 0.25, 0.5, 0.5 + 2.0 ** -24, 1.0, 2.0 - 2.0 ** -22,
                   2.0 - 2.0 ** -23, 2.0], np.float32)
# (float64 also: values that differ only past float32's 24 bits)
POOL64 = np.concatenate([POOL32.astype(np.float64),
                         [0.5 + 1e-12, 0.5 - 1e-13, 2.0 - 1e-15, -1e-8 - 1e-20, 1.0 + 2.0 ** -40]])


def _lists(G, rows, k, f64, seed):
    """[G, rows, k] distances and int32 positions: per (rank, row) an
    ascending list of n_valid in [0, k] entries, then (+inf, -1).  Positions
    are unique within a row across the ranks, drawn from three bands: from 0,
    from 2^30, and up to 2^31 - 1.  Row 0 is full on every rank, row rows // 2
    (rows >= 3) empty on every rank."""
    rng = np.random.default_rng(seed)
    pool = POOL64 if f64 else POOL32
    n = G * k
    band = np.concatenate([np.arange(n), 2 ** 30 + np.arange(n), 2 ** 31 - n + np.arange(n)])
    pos = rng.permuted(np.tile(band, (rows, 1)), axis=1)[:, :n]
    pos = pos.reshape(rows, G, k).transpose(1, 0, 2).astype(np.int64)
    if rows and not (pos[:, 0] == 2 ** 31 - 1).any():
        pos[0, 0, 0] = 2 ** 31 - 1                    # (row 0 is full: the largest position is merged)
    d = pool[rng.integers(0, pool.size, (G, rows, k))]
    n_valid = rng.integers(0, k + 1, (G, rows))
    n_valid[:, 0] = k
    if rows >= 3:
        n_valid[:, rows // 2] = 0
    empty = np.arange(k)[None, None, :] >= n_valid[:, :, None]
    d = np.where(empty, np.inf, d).astype(pool.dtype)
    pos_u = np.where(empty, 0xFFFFFFFF, pos)
    o = np.lexsort((pos_u, d), axis=-1)
    d, pos_u = np.take_along_axis(d, o, -1), np.take_along_axis(pos_u, o, -1)
    return np.ascontiguousarray(d), np.where(pos_u == 0xFFFFFFFF, -1, pos_u).astype(np.int32)


def _oracle(d, pos, k):
    G, rows, _ = d.shape
    dd = d.transpose(1, 0, 2).reshape(rows, G * k)
    pp = pos.transpose(1, 0, 2).reshape(rows, G * k)
    pu = np.where(pp < 0, 0xFFFFFFFF, pp.astype(np.int64))
    o = np.lexsort((pu, dd), axis=-1)[:, :k]
    return np.take_along_axis(dd, o, -1), np.take_along_axis(pp, o, -1)


def _assert_bitwise(got_d, got_p, ref_d, ref_p):
    got_d, got_p = got_d.cpu().numpy(), got_p.cpu().numpy()
    assert got_d.dtype == ref_d.dtype and got_d.shape == ref_d.shape
    itype = np.uint64 if ref_d.dtype == np.float64 else np.uint32
    assert np.array_equal(got_d.view(itype), ref_d.view(itype))
    assert np.array_equal(got_p, ref_p)


def _merge_packed(d, pos, k, extra, bits):
    """lmi_merge_topk_packed over the buffer an all-gather of G packed_lists
    buffers gives, each rank's slice `extra` words longer than the minimum and
    the words K3 has no business reading filled with garbage."""
    G, rows, _ = d.shape
    f64 = d.dtype == np.float64
    lib = _lib.load()
    W0 = int(lib.lmi_packed_rank_words(rows, k, int(f64)))
    W = W0 + extra
    gathered = torch.full((G, W), GARBAGE, dtype=torch.int32, device="cuda")
    for g in range(G):
        buf, dv, pv, sv = packed_lists(rows, k, f64, "cuda")
        assert buf.numel() == W0
        buf.fill_(GARBAGE)
        dv.copy_(torch.from_numpy(d[g]).view(-1))
        pv.copy_(torch.from_numpy(pos[g]).view(-1))
        sv.fill_(bits[g])
        gathered[g, :W0] = buf
    md = torch.full((max(rows, 1), k), -7.0, dtype=torch.float64 if f64 else torch.float32, device="cuda")
    mp = torch.full((max(rows, 1), k), -7, dtype=torch.int32, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check("lmi_merge_topk_packed", lib.lmi_merge_topk_packed(
        _lib.ptr(gathered), G, W, rows, k, int(f64), _lib.ptr(md), _lib.ptr(mp), _lib.ptr(st),
        _lib.stream_handle(torch.device("cuda"))))
    torch.cuda.synchronize()
    return md, mp, int(st.item())


def _shapes():
    out = []
    for k in (1, 10, 11, 16, 17, 40, KMAX):
        for G in (1, 2, 8):
            for rows in ((1, 3) if k == KMAX else (1, 255, 257, 600)):
                out.append((k, G, rows))
    return out


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("k,G,rows", _shapes())
def test_merge_matches_numpy(k, G, rows, f64):
    d, pos = _lists(G, rows, k, f64, seed=1000 * k + 10 * G + rows)
    assert pos.max() == 2 ** 31 - 1
    ref_d, ref_p = _oracle(d, pos, k)
    got_d, got_p = merge_topk(torch.from_numpy(d).cuda(), torch.from_numpy(pos).cuda(), k)
    _assert_bitwise(got_d, got_p, ref_d, ref_p)
    bits = [1 << (3 * g + 1) for g in range(G)]
    for extra in (0, 2):
        md, mp, st = _merge_packed(d, pos, k, extra, bits)
        _assert_bitwise(md, mp, ref_d, ref_p)
        assert st == sum(bits)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [10, 16, 40])
@pytest.mark.parametrize("G", [2, 8])
def test_replicated_lists_are_not_deduplicated(G, k, f64):
    """G identical lists give every entry G times over, in list order: K3
    merges, it does not deduplicate -- why a whole index must not exchange
    its lists over a group of several ranks (Searcher.exchange)."""
    d1, p1 = _lists(1, 257, k, f64, seed=77 + k)
    d, pos = np.repeat(d1, G, axis=0), np.repeat(p1, G, axis=0)
    ref_d, ref_p = np.repeat(d1[0], G, axis=-1)[:, :k], np.repeat(p1[0], G, axis=-1)[:, :k]
    od, op = _oracle(d, pos, k)
    assert np.array_equal(od, ref_d) and np.array_equal(op, ref_p)
    got_d, got_p = merge_topk(torch.from_numpy(d).cuda(), torch.from_numpy(pos).cuda(), k)
    _assert_bitwise(got_d, got_p, ref_d, ref_p)
    md, mp, st = _merge_packed(d, pos, k, 0, [0] * G)
    _assert_bitwise(md, mp, ref_d, ref_p)
    assert st == 0


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [10, 40])
def test_no_rows(k, f64):
    """rows = 0: OK, and nothing is written but the packed form's status."""
    lib = _lib.load()
    G = 2
    dt = np.float64 if f64 else np.float32
    d, pos = np.zeros((G, 0, k), dt), np.zeros((G, 0, k), np.int32)
    md, mp, st = _merge_packed(d, pos, k, 0, [4, 1])
    assert st == 5 and bool((md == -7.0).all()) and bool((mp == -7).all())
    fn = lib.lmi_merge_topk_f64 if f64 else lib.lmi_merge_topk
    _lib.check("lmi_merge_topk", fn(None, None, G, 0, k, _lib.ptr(md), _lib.ptr(mp),
                                    _lib.stream_handle(torch.device("cuda"))))
    torch.cuda.synchronize()
    assert bool((md == -7.0).all()) and bool((mp == -7).all())
