"""The scan in two launches over one tile queue (lmi_scan_set_join_workgroups,
LMI_Q_PHASE_SCAN_JOIN) and the batch stream built on it
(StreamedSearch(join_cus=j): the next scan starts behind the previous one on
CUs - j workgroups, the finish runs on the j CUs left free, j more workgroups
of the same kernel join behind it): whatever the grids and the order of the
two launches, the merged lists and status words are bitwise those of one
launch, the plan does not see the split grid, the scans that do not take the
join refuse it before they launch anything, and every streamed answer is
bitwise Searcher.search of its batch."""
import contextlib
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import workloads
from li import _lib
from li.index import DeviceIndex, DeviceRouter, Searcher, bucket_topk, bucket_topk_f64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
PLAN, SCAN, JOIN, MERGE = (_lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_SCAN_JOIN,
                           _lib.LMI_Q_PHASE_MERGE)
R = 3


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def setup():
    """20,000 rows of width 768 in 8 buckets (two empty, two with 3 and 5 rows),
    chunks of 256 rows (~80 chunks: tail-split tiles on every queue), 300
    queries x 3 probes; `cls`: every query's first probe is the largest bucket
    (300 pairs > the 256 of a tile: sibling tiles), the others two of the rest."""
    w = workloads.clustered(n=20_000, nq=300, C=8, seed=97, label_mode="skewed")
    ix = DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=256, device="cuda")
    s = Searcher(ix, DeviceRouter(w["layers"], device="cuda"))
    sizes = np.bincount(w["labels"], minlength=w["C"])
    assert 0 < sizes[sizes > 0].min() < 10 and int(ix.desc.n_chunks) >= 75
    big = int(np.argmax(sizes))
    rng = np.random.default_rng(5)
    rest = [c for c in range(w["C"]) if c != big]
    cls = np.stack([np.concatenate([[big], rng.permutation(rest)[:R - 1]]) for _ in range(300)]).astype(np.int32)
    assert np.bincount(cls.ravel(), minlength=w["C"]).max() > 256
    # a batch of few tiles (fewer than any join grid below): three queries on the small buckets
    small = [int(c) for c in np.argsort(sizes) if sizes[c] > 0][:R]
    few = np.tile(np.array(small, dtype=np.int32), (3, 1))
    return w, s, T(cls), T(few)


@contextlib.contextmanager
def _grid(wgs, j):
    """The thread's scan grid and join workgroups for the calls inside."""
    lib = _lib.load()
    prev_w, prev_j = lib.lmi_scan_set_workgroups(wgs), lib.lmi_scan_set_join_workgroups(j)
    try:
        yield
    finally:
        assert lib.lmi_scan_set_workgroups(prev_w) == wgs
        assert lib.lmi_scan_set_join_workgroups(prev_j) == j


# the three product list modes of the batch stream: scan3_kernel<10> (float32),
# the 15-entry lists, and the float64 mode's band lists (MODE 3)
MODES = {"k10": (bucket_topk, 10), "k15": (bucket_topk, 12), "band": (bucket_topk_f64, 10)}


def _run(ix, q, cls, mode, seeded, calls, ws=None):
    """The phase calls `calls` = [(phases, workgroups, join workgroups)] on
    fresh outputs -> (d, pos, status)."""
    fn, k = MODES[mode]
    nq = cls.shape[0]
    d = torch.full((nq, R, k), -7.0, dtype=torch.float64 if fn is bucket_topk_f64 else torch.float32,
                   device="cuda")
    p = torch.full((nq, R, k), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros((1,), dtype=torch.int32, device="cuda")
    if ws is None:
        lib = _lib.load()
        size = (lib.lmi_scan_f64_workspace_bytes if fn is bucket_topk_f64 else lib.lmi_scan_workspace_bytes)(
            C.byref(ix.desc_for(k)), nq, R, k, _lib.LMI_Q_F16)
        ws = torch.zeros(int(size), dtype=torch.uint8, device="cuda")
    for ph, wgs, j in calls:
        with _grid(wgs, j):
            fn(ix, q[:nq], cls, k, qmode=_lib.LMI_Q_F16, out=(d, p, st), ws=ws, seed_round0=seeded, phases=ph)
    torch.cuda.synchronize()
    return d, p, st


def _same(a, b, seeded=False):
    """Lists and status words bitwise equal.  Seeded (LMI_Q_SEED_ROUND0): the
    status words and the lists of r = 0 bitwise, and of every r >= 1 list the
    entries at or under round 0's k-th distance of its query -- the part the
    seed defines.  A seeded pair (q, r >= 1) starts from the bound pair (q, 0)
    has when its tile starts (round0_seed in lmi_scan3.hpp), so which entries
    it keeps above round 0's final k-th depends on the order the tiles ran in,
    already within one launch: one launch of this workload on 1, 2, 8 or 64
    workgroups differs from the same launch on every CU in 493, 493, 28 and 22
    entries of its seeded lists (all three modes but the 15-entry lists on 8
    and 64: 0), never in an entry at or under round 0's k-th."""
    if not torch.equal(a[2], b[2]):
        return False
    if not seeded:
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if not (torch.equal(a[0][:, 0], b[0][:, 0]) and torch.equal(a[1][:, 0], b[1][:, 0])):
        return False
    kth0 = b[0][:, 0, -1].reshape(-1, 1, 1)   # (+inf where round 0 has fewer than k)
    ma, mb = a[0] <= kth0, b[0] <= kth0
    return torch.equal(ma, mb) and torch.equal(torch.where(ma, a[0], 0), torch.where(mb, b[0], 0)) and \
        torch.equal(torch.where(ma, a[1], -1), torch.where(mb, b[1], -1))


def _grids():
    n = _cus()
    # (main, join) -> (workgroups, j): the main launch has workgroups - j
    return [(0, 1), (0, n // 2), (0, n - 1), (12, 4)]


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_lists_of_two_launches_equal_one_launch(setup, mode, seeded):
    """PLAN, SCAN on the main grid, SCAN_JOIN with j, MERGE, for (main, j) =
    (CUs - 1, 1), (CUs / 2, CUs / 2), (1, CUs - 1), (8, 4), and j larger than
    the number of tiles: lists and status words bitwise those of one launch
    (seeded: as far as the seed defines them, _same)."""
    w, s, cls, few = setup
    q = T(w["q"])
    ref = _run(s.index, q, cls, mode, seeded, [(0, 0, 0)])
    assert int(ref[2].item()) == 0 and bool((ref[1] >= 0).any())
    for wgs, j in _grids():
        got = _run(s.index, q, cls, mode, seeded, [(PLAN, wgs, j), (SCAN, wgs, j), (JOIN, wgs, j), (MERGE, wgs, j)])
        assert _same(got, ref, seeded), (wgs, j)
    # one call may hold both scan phases (the main launch, then the join)
    assert _same(_run(s.index, q, cls, mode, seeded, [(PLAN | SCAN | JOIN | MERGE, 0, 5)]), ref, seeded)
    ref_few = _run(s.index, q, few, mode, seeded, [(0, 0, 0)])
    j = _cus() - 1
    got = _run(s.index, q, few, mode, seeded, [(PLAN, 0, j), (SCAN, 0, j), (JOIN, 0, j), (MERGE, 0, j)])
    assert _same(got, ref_few, seeded)


@pytest.mark.parametrize("mode", list(MODES))
def test_join_launched_before_the_main_launch(setup, mode):
    """The join's workers take the head of the queue when they are launched
    first (same stream): the same lists, seeded or not."""
    w, s, cls, _ = setup
    q = T(w["q"])
    for seeded in (False, True):
        ref = _run(s.index, q, cls, mode, seeded, [(0, 0, 0)])
        for wgs, j in [(0, 3), (0, _cus() // 4), (12, 4)]:
            got = _run(s.index, q, cls, mode, seeded,
                       [(PLAN, wgs, j), (JOIN, wgs, j), (SCAN, wgs, j), (MERGE, wgs, j)])
            assert _same(got, ref, seeded), (wgs, j, seeded)


@pytest.mark.parametrize("mode", list(MODES))
def test_plan_does_not_see_the_split_grid(setup, mode):
    """The PLAN phase leaves the same workspace, byte for byte, whatever j
    (the tile list, the queues, the tail split keep the whole grid's shape)."""
    w, s, cls, _ = setup
    fn, k = MODES[mode]
    lib = _lib.load()
    size = (lib.lmi_scan_f64_workspace_bytes if fn is bucket_topk_f64 else lib.lmi_scan_workspace_bytes)(
        C.byref(s.index.desc_for(k)), 300, R, k, _lib.LMI_Q_F16)
    q = T(w["q"])
    out = []
    for j in (0, _cus() // 4, _cus() - 1):
        ws = torch.zeros(int(size), dtype=torch.uint8, device="cuda")
        _run(s.index, q, cls, mode, True, [(PLAN, 0, j)], ws=ws)
        out.append(ws)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])


def _timed_launches():
    """Scan launches recorded since the last read (lmi_timing)."""
    ms = (C.c_float * 64)()
    return int(_lib.load().lmi_timing_read(ms, 64))


def test_join_without_workgroups_is_a_no_op_and_launches_are_timed(setup):
    """j = 0: the SCAN_JOIN phase returns LMI_OK and launches nothing; j > 0:
    lmi_timing records the main launch and the join, one record each."""
    w, s, cls, _ = setup
    lib = _lib.load()
    q = T(w["q"])
    lib.lmi_timing_read(None, 0)
    lib.lmi_timing_enable(1)
    try:
        ref = _run(s.index, q, cls, "k10", True, [(0, 0, 0)])
        assert _timed_launches() == 1
        got = _run(s.index, q, cls, "k10", True, [(PLAN, 0, 0), (JOIN, 0, 0), (SCAN, 0, 0), (JOIN, 0, 0),
                                                   (MERGE, 0, 0)])
        assert _same(got, ref, True) and _timed_launches() == 1
        d, p, st = _run(s.index, q, cls, "band", True, [(JOIN, 0, 0)])
        assert _timed_launches() == 0 and bool((d == -7.0).all()) and bool((p == -7).all())
        _run(s.index, q, cls, "k10", True, [(PLAN, 0, 9), (SCAN, 0, 9), (JOIN, 0, 9), (MERGE, 0, 9)])
        assert _timed_launches() == 2
    finally:
        lib.lmi_timing_enable(0)
        lib.lmi_timing_read(None, 0)


@pytest.fixture(scope="module")
def refused(setup):
    """The scans that take no join workgroups: the split mode (a float32 corpus
    that is not fp16-exact), and the general kernel (an index of width 64)."""
    w, s, _, _ = setup
    x32, q32 = workloads.float32_inputs(dict(x=w["x"][:3000], q=w["q"][:40]), 97)
    split = DeviceIndex(x32, w["labels"][:3000], w["C"], chunk_rows=256, device="cuda")
    assert split.storage == "f32x"
    narrow = DeviceIndex(np.ascontiguousarray(w["x"][:3000, :64]), w["labels"][:3000], w["C"], chunk_rows=256,
                         device="cuda")
    return split, T(q32), narrow, T(np.ascontiguousarray(w["q"][:40, :64]))


@pytest.mark.parametrize("what", ["split", "split_f64", "wide", "general", "general_f64"])
def test_scans_without_a_join_refuse_it(setup, refused, what):
    """The split mode's scans, the wide path (k > 16) and the kernels of the
    other widths return the argument error for SCAN and SCAN_JOIN while j > 0
    and launch nothing (no timed launch, the outputs untouched); with j = 0
    their SCAN_JOIN phase is a no-op."""
    w, s, cls, _ = setup
    split, q32, narrow, q64w = refused
    lib = _lib.load()
    ix, q = {"split": (split, q32), "split_f64": (split, q32), "wide": (s.index, T(w["q"][:40])),
             "general": (narrow, q64w), "general_f64": (narrow, q64w)}[what]
    fn = bucket_topk_f64 if what.endswith("f64") else bucket_topk
    k = 20 if what == "wide" else 10
    c = cls[:40].contiguous()
    d = torch.full((40, R, k), -7.0, dtype=torch.float64 if fn is bucket_topk_f64 else torch.float32, device="cuda")
    p = torch.full((40, R, k), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros((1,), dtype=torch.int32, device="cuda")
    fn(ix, q, c, k, out=(d, p, st))                      # (sizes the index's workspace; j = 0)
    torch.cuda.synchronize()
    joinable = (lib.lmi_scan_f64_joinable if fn is bucket_topk_f64 else lib.lmi_scan_joinable)
    qm = _lib.LMI_Q_F16 if ix.storage == "f16" else _lib.LMI_Q_F32
    assert joinable(C.byref(ix.desc_for(k)), 40, R, k, qm) == 0
    d.fill_(-7.0)
    p.fill_(-7)
    st.zero_()
    lib.lmi_timing_read(None, 0)
    lib.lmi_timing_enable(1)
    try:
        # (the wide path takes no phase flags: its whole call is refused)
        for ph in ((0,) if what == "wide" else (SCAN, JOIN, SCAN | JOIN, PLAN | SCAN | MERGE)):
            with _grid(0, 16):
                with pytest.raises(_lib.LmiError) as e:
                    fn(ix, q, c, k, out=(d, p, st), phases=ph)
            assert e.value.rc == _lib.LMI_E_INVALID and "join workgroups" in str(e.value)
            assert b"join workgroups" in lib.lmi_last_error()
        with _grid(0, 0):
            fn(ix, q, c, k, out=(d, p, st), phases=JOIN)
        torch.cuda.synchronize()
        assert _timed_launches() == 0
        assert bool((d == -7.0).all()) and bool((p == -7).all()) and int(st.item()) == 0
    finally:
        lib.lmi_timing_enable(0)
        lib.lmi_timing_read(None, 0)
    assert lib.lmi_scan_set_join_workgroups(0) == 0


def test_the_stream_scans_are_joinable(setup):
    w, s, _, _ = setup
    lib = _lib.load()
    for k in (10, 15):
        assert lib.lmi_scan_joinable(C.byref(s.index.desc_for(k)), 300, R, k, _lib.LMI_Q_F16) == 1
    assert lib.lmi_scan_joinable(C.byref(s.index.desc_for(16)), 300, R, 16, _lib.LMI_Q_F16) == 0
    assert lib.lmi_scan_f64_joinable(C.byref(s.index.desc_for(10)), 300, R, 10, _lib.LMI_Q_F16) == 1
    assert lib.lmi_scan_f64_joinable(C.byref(s.index.desc_for(12)), 300, R, 12, _lib.LMI_Q_F16) == 0


# ---------------------------------------------------------------------------
# the batch stream
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(setup):
    """Six distinct batches and Searcher.search of each, per arithmetic."""
    w, s, _, _ = setup
    bs = []
    for i in range(6):
        p = np.random.default_rng(300 + i).permutation(w["q"].shape[0])
        bs.append((w["qn"][p], w["q"][p]))
    ref = {dd: [s.search(T(a), T(b), R, k=10, dist=dd) for a, b in bs] for dd in ("f32", "f64")}
    return bs, ref


def _eight_launches(st, bs, ref):
    """Eight launches over the six batches: launch t stages batch t mod 6 and
    finishes the batch staged three launches earlier (the first three: the
    batch the stream was built with, batch 0)."""
    staged = []
    for t in range(8):
        st.stage(*bs[t % 6])
        staged.append(t % 6)
        d, a = st.step()
        i = staged[t - 3] if t >= 3 else 0
        np.testing.assert_array_equal(d, ref[i][0], err_msg=f"launch {t}")
        np.testing.assert_array_equal(a, ref[i][1], err_msg=f"launch {t}")


@pytest.mark.parametrize("lookahead", [True, False])
@pytest.mark.parametrize("dist", ["f32", "f64"])
@pytest.mark.parametrize("j", ["1", "quarter", "all_but_one"])
def test_stream_with_a_late_joining_scan_equals_search(setup, batches, j, dist, lookahead):
    w, s, _, _ = setup
    bs, ref = batches
    j = {"1": 1, "quarter": _cus() // 4, "all_but_one": _cus() - 1}[j]
    st = s.streamed(*bs[0], R, k=10, dist=dist, lookahead=lookahead, join_cus=j)
    assert st.join_cus == j and ("SJ", 0) in st.graphs and not st.overlap
    _eight_launches(st, bs, ref[dist])
    st.close()
    # stream(): the pipeline's fill and drain scan eagerly, join included
    st = s.streamed(*bs[0], R, k=10, dist=dist, lookahead=lookahead, join_cus=j)
    for (d, a), (d0, a0) in zip(st.stream(bs), ref[dist]):
        np.testing.assert_array_equal(d, d0)
        np.testing.assert_array_equal(a, a0)
    st.close()
    lib = _lib.load()
    assert lib.lmi_scan_set_join_workgroups(0) == 0 and lib.lmi_scan_set_workgroups(0) == 0


def test_stream_stages_launched_eagerly_with_a_join(setup, batches):
    """capture=False (the form the gloo rehearsal runs): the same stages,
    launched from the host."""
    w, s, _, _ = setup
    bs, ref = batches
    st = s.streamed(*bs[0], R, k=10, capture=False, join_cus=_cus() // 4)
    assert st.graphs is None
    _eight_launches(st, bs, ref["f32"])
    st.close()


def test_join_default_and_exclusive_options(setup, batches):
    """join_cus with reserve_cus raises; so do a j outside [0, CUs) and a scan
    that takes no join; join_cus=0 is the stream without a join; the default
    is the measured fraction of the CUs where the scan takes it."""
    from li import stream
    w, s, _, _ = setup
    bs, ref = batches
    n = _cus()
    with pytest.raises(ValueError, match="exclusive"):
        s.streamed(*bs[0], R, k=10, join_cus=8, reserve_cus=8)
    for bad in (-1, n):
        with pytest.raises(ValueError):
            s.streamed(*bs[0], R, k=10, join_cus=bad)
    with pytest.raises(ValueError, match="8-wave ring"):
        s.streamed(*bs[0], R, k=16, k_round=16, join_cus=8)
    st = s.streamed(*bs[0], R, k=10, join_cus=0)
    assert st.join_cus == 0 and ("SJ", 0) not in st.graphs
    _eight_launches(st, bs, ref["f32"])
    st.close()
    # (the default: only where the scan is long enough to pay, JOIN_MIN_WORK)
    st = s.streamed(*bs[0], R, k=10)
    assert st.join_cus == 0
    st.close()
    floor, stream.JOIN_MIN_WORK = stream.JOIN_MIN_WORK, 0.0
    try:
        st = s.streamed(*bs[0], R, k=10)
    finally:
        stream.JOIN_MIN_WORK = floor
    assert st.join_cus == stream.stream_join(n) == int(n * stream.JOIN_CUS_FRACTION)
    _eight_launches(st, bs, ref["f32"])
    st.close()
    st = s.streamed(*bs[0], R, k=10, reserve_cus=8)
    assert st.join_cus == 0 and st.overlap
    st.close()


def test_stream_dropped_with_its_join_in_flight(setup, batches):
    """A StreamedSearch dropped right after step(), its lookahead scan and
    that scan's join still queued, and a new one on the very same streams (the
    pattern of test_stream_objects_dropped_with_work_in_flight): the old
    object waits for its work before its graphs go."""
    w, s, _, _ = setup
    bs, ref = batches
    saved = None
    for rep in range(2):
        st = s.streamed(*bs[0], R, k=10, lookahead=True, join_cus=_cus() // 4)
        if saved is not None:
            st._fs, st._ps, st._rs = saved   # the streams deliberately shared
            st._cs = st._rs
        _eight_launches(st, bs, ref["f32"])
        st.stage(*bs[1])
        st.step()                            # leaves a scan and its join in flight
        saved = (st._fs, st._ps, st._rs)
        del st
        gc.collect()                         # (the stage closures hold a cycle)


@pytest.mark.timeout(300)
def test_stream_join_under_forced_exchange():
    """Once under LMI_FORCE_EXCHANGE=1 (a one-rank RCCL group, the G > 1
    branch: the join behind F2), in its own process: the pytest process keeps
    no process group (tests/stream_join_worker.py)."""
    env = dict(os.environ, LMI_FORCE_EXCHANGE="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               LMI_DIST_TIMEOUT_S="120")
    env.pop("MASTER_PORT", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "stream_join_worker.py")], env=env,
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "stream join under forced exchange OK" in p.stdout
