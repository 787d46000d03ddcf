"""The device replay (lmi_replay_device, csrc/lmi_replay_gpu.hip) off the one
point test_gpu_replay.py holds it at (k_round = k_list = 10, float32 lists):
k_round 1 .. 32 on both sides of every dispatch edge of replay_group_body
(fill<10|16|32>, mrg<4|8|16>, sel<2|4|8|16> and the global loop), lists wider
than k_round, float64 lists, k_final 1 .. 2 k_round -- bit for bit against the
host twin (pinned to the oracle by test_replay_params_host.py) and, where it
is cheap, against the oracle itself.  The branch a case is there for is
asserted from its inputs (replay_cases.group_branches) or from the oracle's
counters before the device result is read."""
import numpy as np
import pandas as pd
import pytest
import torch

import lmi_oracle as O
import replay_cases as RC
import workloads
from li import _lib
from li.index import DeviceIndex, DeviceRouter, Searcher, replay, replay_device

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}


def _T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _upload(classes, d, pos, size, ids):
    return dict(classes=_T(classes), lists_d=_T(d), lists_pos=_T(pos), bucket_size=_T(size),
                pos_to_id=_T(ids))


def _device(up, thr_round0=None, **kw):
    dd, aa, st = replay_device(up["classes"], up["lists_d"], up["lists_pos"],
                               bucket_size=up["bucket_size"], pos_to_id=up["pos_to_id"],
                               thr_round0=_T(thr_round0), **kw)
    assert int(st.item()) == 0
    return dd.cpu().numpy(), aa.cpu().numpy().view(np.uint32)


def _equal(got, ref, what):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"distances, {what}")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"ids, {what}")


# --------------------------------------------------------------------------
# the grid: both sides of every k_round edge (fill: 10|11, 16|17; mrg: 8|9,
# 16|17; the ends 1, 2, 31, 32)
# --------------------------------------------------------------------------
GRID_KR = (1, 2, 8, 9, 10, 11, 16, 17, 31, 32)
GRID_NQ, GRID_C = 500, 24


def grid_lists(kr, R, thr, k_list, dtype):
    # buckets of 1 and k_round - 1 rows, an empty one, and probes of it
    lists = RC.make_lists(100 * kr + 10 * R + thr, GRID_NQ, R, GRID_C, k_list, dtype,
                          sized={3: 1, 7: kr - 1}, empty=(5,), probe_empty=True)
    RC.check_sorted(lists[1], lists[2])
    return lists


def grid_expected(kr, R, stats):
    """The oracle counters one (k_round, R) cell of the grid must have hit
    over its thresholds, widths and k_final values.  A bucket below k_round
    needs k_round >= 2; |U| < k_round of a non-empty U likewise.  A skipped
    group (no entry of the whole group beats its queries' thresholds) is
    asked for at R = 4 only: with one thresholded round it is rare."""
    want = []
    if kr >= 2:
        want.append("quirk0")
    if R > 1:
        want += ["fillers"] + (["quirk_thr"] if kr >= 2 else []) + (["skipped"] if R == 4 else [])
    missing = [key for key in want if not stats.get(key)]
    assert not missing, (kr, R, missing, stats)


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kr", GRID_KR)
def test_grid_device_replay_equals_host_and_oracle(kr, dt, R):
    stats = {}
    for thr in (True, False):
        for k_list in (kr, kr + 5):
            classes, d, pos, size, ids = grid_lists(kr, R, thr, k_list, DTYPES[dt])
            up = _upload(classes, d, pos, size, ids)
            for k_final in RC.k_finals(kr, R):
                kw = dict(k_round=kr, k_final=k_final, use_threshold=thr)
                ref = O.replay(classes, d, pos, bucket_size=size, pos_to_id=ids, stats=stats, **kw)
                host = replay(classes, d, pos, bucket_size=size, pos_to_id=ids, **kw)
                _equal(host, ref, f"host twin vs oracle {kw} k_list={k_list}")
                _equal(_device(up, **kw), ref, f"device vs oracle {kw} k_list={k_list}")
    grid_expected(kr, R, stats)


# --------------------------------------------------------------------------
# R = 1 with threshold_dist
# --------------------------------------------------------------------------
def round0_thresholds(classes, d, seed):
    """Per category c: c % 3 == 0 nothing relevant (the group is skipped),
    1: only the first two queries of the group keep their nearest entry and
    its ties (a few relevant positions: |U| < k_round from k_round = 8 on),
    2: everything or about half of every list."""
    rng = np.random.default_rng(seed)
    nq = classes.shape[0]
    thr = np.zeros(nq)
    c = classes[:, 0]
    most = c % 3 == 2
    thr[most] = rng.choice([0.45, 1.0], int(most.sum()))
    for cat in np.unique(c[c % 3 == 1]):
        for q in np.nonzero(c == cat)[0][:2]:
            if np.isfinite(d[q, 0, 0]):
                thr[q] = float(d[q, 0, 0]) + 5e-4  # (the pool's step is 1e-3)
    return thr


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kr", [1, 8, 16, 17, 32])
def test_single_round_with_threshold_dist(kr, dt):
    for k_list in (kr, kr + 5):
        classes, d, pos, size, ids = RC.make_lists(900 + kr, 500, 1, 16, k_list, DTYPES[dt],
                                                   sized={2: 1, 4: max(kr - 1, 1)})
        thr0 = round0_thresholds(classes, d, kr)
        rows = {b.rows for b in RC.group_branches(classes[:, 0], d[:, 0], pos[:, 0], size, kr,
                                                  thr0).values()}
        # (a non-empty U has at least one member: no |U| < k_round at k_round = 1)
        assert rows >= ({"skipped", "fill", "quirk_thr"} if kr > 1 else {"skipped", "fill"}), rows
        kw = dict(k_round=kr, k_final=kr, use_threshold=False, thr_round0=thr0)
        st = {}
        ref = O.replay(classes, d, pos, bucket_size=size, pos_to_id=ids, stats=st, **kw)
        assert st["skipped"] > 0 and st["fillers"] > 0 and (kr == 1 or st["quirk_thr"] > 0), st
        host = replay(classes, d, pos, bucket_size=size, pos_to_id=ids, **kw)
        _equal(host, ref, f"host twin vs oracle k_list={k_list}")
        _equal(_device(_upload(classes, d, pos, size, ids), **kw), ref, f"device k_list={k_list}")


# --------------------------------------------------------------------------
# selection tiers: groups whose relevant positions span more than the bitmap
# --------------------------------------------------------------------------
# group sizes by k_round so that nU = size * k_round lands in each tier
TIER_GROUP = {8: {"sel4": 400, "sel8": 800, "sel16": 1500, "loop": 2200},
              10: {"sel4": 300, "sel8": 600, "sel16": 1200, "loop": 1700},
              32: {"sel4": 100, "sel8": 200, "sel16": 400, "loop": 600}}
TIER_NU = {"sel4": (2048, 4096), "sel8": (4096, 8192), "sel16": (8192, 16384), "loop": (16384, 1 << 30)}
TIER_STAGING = {"sel4": "lds", "sel8": "lds", "sel16": "global", "loop": "global"}
TIER_CASES = [(kr, tier, 1, "f32") for kr in TIER_GROUP for tier in TIER_GROUP[kr]] + [
    (10, "loop", 3, "f32"), (32, "sel8", 3, "f32"),     # running thresholds decide relevance
    (32, "sel16", 1, "f64"), (10, "loop", 1, "f64"),    # float64 lists
    (32, "loop", 3, "f64")]


@pytest.mark.parametrize("kr,tier,R,dt", TIER_CASES)
def test_selection_tiers_beyond_the_bitmap(kr, tier, R, dt):
    """A bucket of 300 000 rows (tables only) whose group's relevant positions
    lie below 1000 and above 250 000: selection by wave minima from 4, 8 or 16
    registers per lane or by the loop over U, U in LDS or in global scratch,
    and the wave-list merge (mrg<4> at k_round = 8, <8> at 10, <16> at 32);
    two small buckets with groups of the same size take the bitmap in the
    same launch."""
    n_group = TIER_GROUP[kr][tier]
    k_list = kr if (R == 1 and dt == "f32") else kr + 5
    classes, d, pos, size, ids = RC.wide_lists(7 * kr + n_group, n_group, R, k_list, DTYPES[dt])
    RC.check_sorted(d, pos)
    kw = dict(k_round=kr, k_final=kr, bucket_size=size, pos_to_id=ids, use_threshold=R > 1)
    thr0 = np.full(classes.shape[0], 2.0) if R == 1 else None  # above every distance: U = the lists
    for r in range(R):
        if R == 1:
            thr = thr0
        elif r == 0:
            continue  # an unthresholded round copies its rows
        else:
            thr = RC.running_thresholds(replay, r, classes, d, pos, **kw)
        br = RC.group_branches(classes[:, r], d[:, r], pos[:, r], size, kr, thr)
        big = br[0]
        assert big.n_group == n_group and TIER_NU[tier][0] < big.nU <= TIER_NU[tier][1], big
        assert big.span >= RC.BM_BITS and big.select == tier and big.staging == TIER_STAGING[tier], big
        assert big.rows == "fill" and big.fill == {8: 10, 10: 10, 32: 32}[kr], big
        assert big.merge == {8: 4, 10: 8, 32: 16}[kr], big
        if R > 1:  # the thresholds cut: relevance is decided per entry
            assert 0 < big.n_rel < big.nU, big
        for c in (1, 2):
            assert br[c].select == "bitmap" and br[c].nU == big.nU and br[c].rows == "fill", br[c]
    host = replay(classes, d, pos, thr_round0=thr0, **kw)
    if tier in ("sel4", "sel8") and R == 1:  # (the oracle's union scan is quadratic)
        okw = dict(kw, thr_round0=thr0)
        _equal(host, O.replay(classes, d, pos, **okw), "host twin vs oracle")
    del kw["bucket_size"], kw["pos_to_id"]
    _equal(_device(_upload(classes, d, pos, size, ids), thr_round0=thr0, **kw), host, "device vs host twin")


# --------------------------------------------------------------------------
# the phased call at the far corner
# --------------------------------------------------------------------------
def test_phased_replay_at_k_round_32_float64():
    """GROUPS then ROUNDS on one workspace at k_round = 32, k_list = 37,
    float64 lists, R = 3, k_final = 40 = the one-call replay = the host
    twin."""
    kr, k_list, R, k_final, nq = 32, 37, 3, 40, 500
    classes, d, pos, size, ids = RC.make_lists(3237, nq, R, 24, k_list, np.float64,
                                               sized={3: 1, 7: kr - 1}, empty=(5,), probe_empty=True)
    kw = dict(k_round=kr, k_final=k_final, use_threshold=True)
    st = {}
    ref = O.replay(classes, d, pos, bucket_size=size, pos_to_id=ids, stats=st, **kw)
    assert st["quirk0"] > 0 and st["quirk_thr"] > 0 and st["fillers"] > 0, st
    host = replay(classes, d, pos, bucket_size=size, pos_to_id=ids, **kw)
    _equal(host, ref, "host twin vs oracle")
    up = _upload(classes, d, pos, size, ids)
    one = _device(up, **kw)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    out = (torch.empty((nq, k_final), dtype=torch.float64, device="cuda"),
           torch.empty((nq, k_final), dtype=torch.int32, device="cuda"),
           torch.full((1,), 0x70, dtype=torch.int32, device="cuda"))
    tab = dict(bucket_size=up["bucket_size"], pos_to_id=up["pos_to_id"])
    replay_device(up["classes"], None, None, out=out, phases=_lib.LMI_REPLAY_PHASE_GROUPS, ws=ws,
                  k_list=k_list, **tab, **kw)
    torch.cuda.synchronize()
    assert int(out[2].item()) == 0
    replay_device(up["classes"], up["lists_d"], up["lists_pos"], out=out,
                  phases=_lib.LMI_REPLAY_PHASE_ROUNDS, ws=ws, **tab, **kw)
    assert int(out[2].item()) == 0
    phased = (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32))
    _equal(phased, one, "phased vs one call")
    _equal(phased, host, "phased vs host twin")


# --------------------------------------------------------------------------
# refusals: before any launch
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kr,R,k_list,k_final", [(5, 2, 5, 11), (32, 2, 32, 65), (1, 4, 1, 3),  # k_final
                                                 (33, 2, 33, 33),                               # k_round
                                                 (16, 2, 15, 16)])                              # k_list
def test_device_replay_refuses_what_it_does_not_hold(kr, R, k_list, k_final):
    classes, d, pos, size, ids = RC.make_lists(5, 64, R, 8, k_list)
    with pytest.raises(_lib.LmiError) as e:
        replay_device(_T(classes), _T(d), _T(pos), k_round=kr, k_final=k_final, bucket_size=_T(size),
                      pos_to_id=_T(ids), use_threshold=True)
    assert e.value.rc == _lib.LMI_E_INVALID


# --------------------------------------------------------------------------
# through the callers
# --------------------------------------------------------------------------
def _nn(layers, arch, C):
    from li.model import NeuralNetwork
    nn = NeuralNetwork(input_dim=96, output_dim=C, lr=0.009, model_type=arch)
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (w, b) in zip(lin, layers):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    return nn


def _spread_classes(seed, nq, R, C):
    """R distinct buckets per query, uniform over all C: the skewed workload's
    big, tiny (fewer rows than k) and empty buckets all get a group in every
    round, which its untrained router's own top R would not give."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(C, R, replace=False) for _ in range(nq)]).astype(np.int64)


def single_thresholds(w, cls, k, seed):
    """threshold_dist for search_single: per query the j-th smallest distance
    to its bucket (j in 0 .. 2k + 1, so none, a few, or more than k objects
    beat it), moved at least 2e-5 away from every distance of the bucket so
    that float32 rounding cannot flip an object across it."""
    rng = np.random.default_rng(seed)
    D = O.pairwise_cosine(w["q"], w["x"])
    thr = np.zeros(cls.size)
    for q, c in enumerate(cls):
        row = np.sort(D[q, w["labels"] == c].astype(np.float64))
        if row.size == 0:
            continue
        t = row[min(int(rng.integers(0, 2 * k + 2)), row.size - 1)]
        while np.abs(row - t).min() < 2e-5:
            t += 5e-5
        thr[q] = t
    return thr


@pytest.mark.parametrize("with_thr", [False, True])
@pytest.mark.parametrize("k", [1, 17, 32])
def test_search_single_off_k10(k, with_thr):
    """LearnedIndex.search_single passes k as k_round = k_list to the device
    replay: against the reference's search_single restated (tie-aware, the
    scan's float32 arithmetic is not numpy's), and bit for bit against the
    host twin run on the scan's own lists."""
    from li.LearnedIndex import LearnedIndex
    n, nq, C = 3000, 200, 16
    w = workloads.clustered(n=n, nq=nq, C=C, seed=61, label_mode="skewed")
    cls = _spread_classes(61 + k, nq, 1, C)[:, 0]
    thr = single_thresholds(w, cls, k, k) if with_thr else None
    ref_d, ref_a = O.search_single_direct(w["labels"], np.arange(1, n + 1), w["x"], w["q"], cls, k=k,
                                          threshold_dist=thr)
    li = LearnedIndex()
    li.model = _nn(w["layers"], "MLP", C)
    data = pd.DataFrame(w["xn"])
    data.index += 1
    data["category"] = w["labels"]
    data_search = pd.DataFrame(w["x"])
    data_search.index += 1
    dists, anns = li.search_single(data, data_search, w["q"], cls, k=k, threshold_dist=thr)
    assert dists.shape == (nq, k) and dists.dtype == np.float64 and anns.dtype == np.uint32
    assert O.compare_lists(ref_d, ref_a, dists, anns) == 0
    index = li._index
    classes = cls.astype(np.int32).reshape(-1, 1)
    _, d, pos, st = li._get_searcher(index).lists(None, _T(w["q"]), 1, k, classes=_T(classes))
    assert int(st.item()) == 0
    host = replay(classes, d.cpu().numpy(), pos.cpu().numpy(), k_round=k, k_final=k,
                  bucket_size=index.bucket_size, pos_to_id=index.pos_to_id, use_threshold=False,
                  thr_round0=thr)
    _equal((dists, anns), host, "search_single vs host twin on the scan's lists")


@pytest.mark.parametrize("dist", ["f32", "f64"])
def test_searcher_k_round_16_k_20(dist):
    """Searcher.search(k_round=16, k=20, R=3): k_final > k_round off
    k_round = 10, in both distance modes, against the oracle's
    bucket_lists + replay with test_gpu_parity.py's tolerances; the host
    replay of the same lists must agree bit for bit."""
    n, nq, R = 3000, 200, 3
    w = workloads.clustered(n=n, nq=nq, C=16, seed=62, label_mode="skewed")
    s = Searcher(DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=512), DeviceRouter(w["layers"]))
    classes = _spread_classes(62, nq, R, w["C"])
    # float16 operands make the oracle compute in float64 (sklearn's rule), as
    # dist="f64" does; the values are fp16-exact
    x, q = (w["x"], w["q"]) if dist == "f32" else (w["x"].astype(np.float16), w["q"].astype(np.float16))
    tol = {} if dist == "f32" else dict(atol=1e-12, tie=1e-12)
    for thr in (True, False):
        st = {}
        order, off = O.layout(w["labels"], w["C"])
        ld, lp = O.bucket_lists(w["labels"], x, q, classes, R, 16, w["C"])
        ref_d, ref_a = O.replay(classes, ld, lp, k_round=16, k_final=20, bucket_size=np.diff(off),
                                pos_to_id=np.arange(1, n + 1)[order], use_threshold=thr, stats=st)
        assert st["quirk0"] > 0 and (not thr or (st["quirk_thr"] > 0 and st["fillers"] > 0)), st
        kw = dict(k=20, k_round=16, use_threshold=thr, dist=dist)
        d, a = s.search(None, _T(w["q"]), R, classes=_T(classes.astype(np.int32)), **kw)
        assert d.shape == (nq, 20) and a.dtype == np.uint32
        assert O.compare_lists(ref_d, ref_a, d, a, **tol) == 0, (dist, thr)
        _equal(s.search(None, _T(w["q"]), R, classes=_T(classes.astype(np.int32)), replay_on="host",
                        **kw), (d, a),
               "host replay vs device replay")
