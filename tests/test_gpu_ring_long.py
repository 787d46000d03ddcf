"""The i8, mx4, mx6 and metric rings (scan3_i8_kernel, scan3_mx4_kernel,
scan3_mx6_kernel, scan3_kernel MODE 5 / 6) on tiles of 3 to 66 blocks: the
fixture of tests/ring_long_cases.py (chunk_rows = 2112; tiles of 3, 4, 5, 9, 32,
33 and 66 blocks; P1, heterogeneous bounds in one pair tile; P2, ties at an
exchanged bound), whose conditions tests/test_ring_long_cases_host.py proves
from the references alone.  The other test files of these rings stop at 2 (i8:
16, metric: 8) blocks a tile, where the in-loop DMA, the steady-state wait, the
slot and norm-area wraps and the bound exchange every 32 blocks never run.

Every list is compared with an independent restatement -- mx4 / mx6: float64 of
mx4_cases / mx6_cases within TOL = 768 * 2^-23 (test_gpu_mx4.py's derivation)
and bit for bit on exact inputs; i8: bit for bit against i8_cases and the
general i8 kernel; l2 / ip: float64 by the definition under test_gpu_metric's
bound -- and bit for bit with the same call on one workgroup, where the tiles
run one after another and every later tile starts from the bound the earlier
ones published: the sums do not depend on pruning, so any difference is a
pruning bug."""
import functools

import numpy as np
import pytest

import i8_cases as I8
import ring_long_cases as L
import test_gpu_i8_ring as RING
import test_gpu_metric as MET
import test_gpu_mx4 as MX4
import test_gpu_mx6 as MX6
from li import _lib
from li.index import DeviceIndex, Searcher, bucket_topk, i8_lists16, scan_family

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the exact-input tests' 20 equal rows of a 1056-row (33-block) bucket, 16 of them past block 31
SAME_LONG = (3, 500, 1000, 1023, 1024, 1025, 1026, 1030, 1031, 1032, 1033, 1040, 1041, 1042, 1043, 1050, 1052, 1053,
             1054, 1055)


class _one_workgroup:
    """The scans of this thread on a grid of one workgroup."""

    def __enter__(self):
        self.prev = _lib.load().lmi_scan_set_workgroups(1)

    def __exit__(self, *exc):
        assert _lib.load().lmi_scan_set_workgroups(self.prev) == 1


def _assert_ties(got_d, got_p, k):
    """P2: the k lowest positions of the 20 equal rows, one distance bit pattern."""
    assert np.array_equal(got_p[L.QTIE, 0, :k], L.TIE_POS[:k]), got_p[L.QTIE, 0]
    assert np.unique(RING._bits(got_d[L.QTIE, 0, :k])).size == 1


# ---- 1. mx4 and mx6 ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mx(storage):
    f = L.fixture()
    s = Searcher(DeviceIndex(f["x"], f["labels"], L.C, chunk_rows=L.CHUNK, device=DEV, storage=storage), None)
    assert np.array_equal(s.index.layout.order, np.arange(L.N))
    assert np.array_equal(s.index.layout.bucket_off, L.OFF) and s.index.max_chunks == 3
    return s


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("storage", ["mx4", "mx6"])
def test_mx_lists_against_float64_and_one_workgroup(storage, k):
    assert MX4.TOL == L.TOL == 768 * 2.0 ** -23
    f, s, dist = L.fixture(), _mx(storage), L.restated(storage)
    L.check_planted(dist, 100 * L.TOL)
    assert s.index.storage == storage and scan_family(s.index, k, lists16=k > 10) == "ring8-" + storage
    got_d, got_p = MX4._lists(s, f["q"], f["classes"], k)
    MX4._check_lists(got_d, got_p, dist, L.OFF, f["classes"], k)
    _assert_ties(got_d, got_p, k)
    with _one_workgroup():
        one_d, one_p = MX4._lists(s, f["q"], f["classes"], k)
    assert np.array_equal(one_p, got_p) and np.array_equal(RING._bits(one_d), RING._bits(got_d))


@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("mod", [MX4, MX6], ids=["mx4", "mx6"])
def test_mx_exact_inputs_bit_for_bit_on_a_33_block_tile(mod, k):
    assert sum(p >= 1024 for p in SAME_LONG) == 16 and len(SAME_LONG) == 20
    mod._exact_inputs(k, (1056, 33), SAME_LONG, L.CHUNK)


# ---- 2. i8 ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _i8():
    f = L.fixture()
    s = Searcher(DeviceIndex(f["x"], f["labels"], L.C, chunk_rows=L.CHUNK, device=DEV, storage="i8",
                             tags=f["tags"]), None)
    assert np.array_equal(s.index.layout.order, np.arange(L.N)) and s.index.max_chunks == 3
    return s


def _i8_case(k, tagged):
    """RING._both (restatement and general kernel, bit for bit) and P2; tagged: a
    query wanting bit 31 lists exactly that bit's rows, all past the first exchange."""
    f, s, dist = L.fixture(), _i8(), L.restated("i8")
    if not tagged:
        got_d, got_p = RING._both(s, f["q"], f["classes"], k, dist)
        _assert_ties(got_d, got_p, k)
        return
    L.check_tags()
    got_d, got_p = RING._both(s, f["q"], f["classes"], k, dist, want=f["want"], avoid=f["avoid"])
    elig = L.eligible(f["tags"], f["want"], f["avoid"])
    for i in np.flatnonzero(f["want"] == 1 << 31):
        rows = np.sort(L.WANT31_POS)
        best = rows[np.lexsort((rows, dist[i, rows]))][:k]
        assert elig[i].sum() == rows.size and np.array_equal(got_p[i, 0, :best.size], best), i
        assert (got_p[i, 0, best.size:] == -1).all()
    if k > 1:                                                  # QTIE: the bit's three copies first, by position
        assert np.array_equal(got_p[L.QTIE, 0, :3], np.sort(L.WANT31_POS[np.isin(L.WANT31_POS, L.TIE_POS)]))
        assert np.unique(RING._bits(got_d[L.QTIE, 0, :3])).size == 1


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [1, 10, 11, 16])
def test_i8_ring_plain_and_tagged(k, tagged):
    L.check_planted(L.restated("i8"), 100 * L.TOL)
    if k <= 10:
        return _i8_case(k, tagged)
    assert scan_family(_i8().index, k, tagged=tagged) == "general"
    with i8_lists16():
        _i8_case(k, tagged)


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [10, 16])
def test_i8_ring_one_workgroup(k, tagged):
    f, s, dist = L.fixture(), _i8(), L.restated("i8")
    kw = dict(want=f["want"], avoid=f["avoid"]) if tagged else {}
    elig = L.eligible(f["tags"], f["want"], f["avoid"]) if tagged else None
    ref = I8.bucket_lists(dist, L.OFF, f["classes"], k, eligible=elig)
    with i8_lists16():
        assert scan_family(s.index, k, tagged=tagged) == "ring8-i8"
        with _one_workgroup():
            got = RING._lists(s, f["q"], f["classes"], k, **kw)
        RING._same(got, ref, "one workgroup vs restatement")
        RING._same(got, RING._lists(s, f["q"], f["classes"], k, **kw), "one workgroup vs the whole grid")


# ---- 3. the metric ring -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _metric_index(metric):
    f = L.fixture()
    ix = DeviceIndex(f["xm"], f["labels"], L.C, storage="f16", chunk_rows=L.CHUNK, device=DEV, metric=metric)
    assert ix.metric == metric and np.array_equal(ix.layout.order, np.arange(L.N))
    return ix


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_metric_ring_against_float64_and_one_workgroup(metric, k):
    f, ix = L.fixture(), _metric_index(metric)
    D, rd, rp = L.metric_reference(metric)
    w = dict(q=f["qm"], xs=f["xm"].astype(np.float64))
    err = MET._errfn(768, metric, True, w)
    qn, yn = err.norms
    L.check_planted(D, 100 * (2.0 * err(qn, yn.max())).max(), ks=(1, 10))
    if metric == "ip":
        assert (rd[:, 0, 0] < 0).all()                         # negative bounds cross the exchange
    # from the reference alone: the metric's lists are not the cosine's
    _, _, cp = L.metric_reference("cosine")
    full = rp[..., 9] >= 0
    differ = np.any(np.sort(rp[..., :10], -1) != np.sort(cp[..., :10], -1), axis=-1)
    assert differ[full].mean() >= 0.90, f"only {differ[full].mean():.1%} of the top-10 lists differ from cosine"
    # the 8-wave ring (scan3_kernel MODE 5 / 6), not scan_kernel_metric: the plan's family at this k
    assert ix.d_pad == 768 and scan_family(ix, k, qmode=MET.F16) == "ring8"
    q, cls = MET.T(f["qm"]), MET.T(f["classes"])
    got_d, got_p = MET._lists(bucket_topk(ix, q, cls, k, qmode=MET.F16))
    MET._check(D, rd, rp, got_d, got_p, k, err, L.bucket_mask(f["classes"]), cap=0.10)
    _assert_ties(got_d, got_p, k)
    with _one_workgroup():
        one_d, one_p = MET._lists(bucket_topk(ix, q, cls, k, qmode=MET.F16))
    assert np.array_equal(one_p, got_p) and np.array_equal(RING._bits(one_d), RING._bits(got_d))
