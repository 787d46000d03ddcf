"""K8 on the GPU: DeviceIndex.relabel (csrc/lmi_rebucket.hip) against the
invariant of the feature -- the index a relabel returns is bitwise, in every
array, the index a construction from scratch over the same row sequence with
the new labels gives -- the sort and gather kernels at their edges, and the
layers above (Searcher.with_index, LearnedIndex.rebucket).  Comparisons are
np.array_equal / torch.equal, never a tie window."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from li import _lib, synth
from test_gpu_index_update import ARRAYS, HOST, _frames, _nn, _same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, EXTRA, C = 3000, 300, 16
CAP = _lib.LMI_REBUCKET_MAX_BUCKETS
MAX_WAVES = _lib.LMI_REBUCKET_MAX_WAVES


@functools.lru_cache(maxsize=None)
def _w(d, mode):
    return workloads.clustered(n=N + EXTRA, d=d, nq=64, C=C, seed=11, label_mode=mode)


@functools.lru_cache(maxsize=None)
def _router2():
    """A second, differently seeded router over the same navigation vectors
    and its labels of the workload's rows (the labels of a retrained model)."""
    w = _w(768, "skewed")
    layers = synth.np_router_layers(synth.ARCHS["MLP"], C, 1234)
    return layers, np.asarray(O.predict(w["xn"], layers), np.int64)


def _index(x, labels, ids, chunk_rows, n_buckets=C, **kw):
    from li.index import DeviceIndex
    return DeviceIndex(x, labels, n_buckets, ids=ids, chunk_rows=chunk_rows, device=DEV, **kw)


class _Seq:
    """The row sequence of an index (rows, labels, ids in sequence order),
    updated beside the index and rebuilt from scratch for the comparison."""

    def __init__(self, x, labels, ids, chunk_rows, n_buckets=C, index=None):
        self.x, self.labels, self.ids = x, np.asarray(labels, np.int64), ids
        self.chunk_rows, self.C = chunk_rows, n_buckets
        self.index = index if index is not None else _index(x, labels, ids, chunk_rows, n_buckets)

    def check(self):
        assert self.index.n_buckets == self.C and self.index.layout.n_buckets == self.C
        _same(self.index, _index(self.x, self.labels, self.ids, self.chunk_rows, self.C, storage="f16"))

    def relabel(self, labels, n_buckets=None, how="numpy"):
        labels = np.asarray(labels, np.int64)
        given = {"numpy": lambda: labels,                                   # int64 on the host
                 "list": lambda: labels.tolist(),
                 "torch": lambda: torch.from_numpy(labels.copy()),          # a host tensor
                 "dev32": lambda: torch.from_numpy(labels.astype(np.int32)).to(DEV),
                 "dev64": lambda: torch.from_numpy(labels.copy()).to(DEV)}[how]()
        old = self.index
        self.index = old.relabel(given) if n_buckets is None else old.relabel(given, n_buckets)
        assert self.index is not old
        if old.n_rows:
            for k in ("corpus", "inv_norm", "bucket_off_local"):            # new buffers
                assert getattr(self.index, k).data_ptr() != getattr(old, k).data_ptr(), k
        self.labels = labels
        if n_buckets is not None:
            self.C = n_buckets
        self.check()

    def add(self, x, labels, ids):
        self.index = self.index.add(torch.from_numpy(x).half().to(DEV), labels, ids)
        self.x = np.concatenate([self.x, x])
        self.labels = np.concatenate([self.labels, labels])
        self.ids = np.concatenate([self.ids, ids])
        self.check()

    def remove(self, ids):
        self.index = self.index.remove(ids)
        keep = ~np.isin(self.ids, ids)
        self.x, self.labels, self.ids = self.x[keep], self.labels[keep], self.ids[keep]
        self.check()


@pytest.mark.parametrize("chunk_rows", [1024, None], ids=["chunk1024", "chunkdefault"])
@pytest.mark.parametrize("mode", ["router", "skewed"])
@pytest.mark.parametrize("d", [8, 100, 768])
def test_relabel_equals_rebuild(d, mode, chunk_rows):
    from li.index import DeviceIndex
    w = _w(d, mode)
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64) * 3 + 1           # (not the default ids)
    rng = np.random.Generator(np.random.PCG64(100 + d))
    s = _Seq(x[:N], lab[:N], ids[:N], chunk_rows)
    s.check()
    # the same labels: nothing moves, yet a new index with new buffers
    s.relabel(lab[:N])
    # a permutation of the bucket names
    s.relabel(rng.permutation(C)[lab[:N]], how="dev64")
    # uniformly random labels: every row moves
    s.relabel(rng.integers(0, C, N), how="dev32")
    # every row into one bucket: the first, then the last
    s.relabel(np.zeros(N, np.int64), how="torch")
    s.relabel(np.full(N, C - 1), how="list")
    # labels that leave the first, a middle and the last bucket empty
    live = np.setdiff1d(np.arange(C), [0, C // 2, C - 1])
    s.relabel(rng.choice(live, N), how="dev32")
    assert not s.index.bucket_size[[0, C // 2, C - 1]].any()
    # more buckets, then one
    s.relabel(rng.integers(0, 122, N), 122, how="numpy")
    s.relabel(np.zeros(N, np.int64), 1, how="dev64")
    s.relabel(lab[:N], C)
    # relabel -> add -> remove -> relabel
    s.add(x[N:N + 257], lab[N:N + 257], ids[N:N + 257])
    s.remove(rng.choice(s.ids, 150, replace=False))
    assert s.index.n_rows == N + 257 - 150
    s.relabel(rng.integers(0, C, s.index.n_rows), how="dev32")
    s.add(x[N + 257:], lab[N + 257:], ids[N + 257:])
    # an index that never saw host rows: empty().add(all rows).relabel(...)
    filled = DeviceIndex.empty(d, C, device=DEV, chunk_rows=chunk_rows).add(
        torch.from_numpy(x).half().to(DEV), torch.from_numpy(lab).to(DEV), ids)
    e = _Seq(x, lab, ids, chunk_rows, index=filled)
    e.check()
    e.relabel(rng.integers(0, C, N + EXTRA), how="dev64")
    # ... and an index of no rows
    z = _Seq(x[:0], lab[:0], ids[:0], chunk_rows)
    z.relabel(lab[:0], 5)


# ---- the sort at the ABI level ---------------------------------------------------
def _sort(labels: torch.Tensor, n_buckets: int):
    """lmi_bucket_sort_labels over device labels: (order, bucket_off, status);
    `order` starts as -1 everywhere (rows the sort did not write stay -1)."""
    lib = _lib.load()
    n = int(labels.numel())
    order = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    off = torch.full((n_buckets + 1,), -1, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.lmi_bucket_sort_labels_ws_bytes(n, n_buckets)
    ws = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=DEV)
    rc = lib.lmi_bucket_sort_labels(_lib.ptr(labels), labels.element_size(), n, n_buckets, _lib.ptr(off),
                                    _lib.ptr(order), _lib.ptr(status), _lib.ptr(ws), need,
                                    _lib.stream_handle(DEV))
    _lib.check("lmi_bucket_sort_labels", rc)
    torch.cuda.synchronize()
    return order.cpu().numpy(), off.cpu().numpy(), int(status.item())


def _check_sort(lab: np.ndarray, n_buckets: int):
    from li.index import BucketLayout
    want = BucketLayout.from_labels(lab, n_buckets)
    for dt in (np.int32, np.int64):
        order, off, st = _sort(torch.from_numpy(lab.astype(dt)).to(DEV), n_buckets)
        assert st == 0
        assert off.dtype == want.bucket_off.dtype and np.array_equal(off, want.bucket_off), (dt, n_buckets)
        assert order.dtype == want.order.dtype and np.array_equal(order, want.order), (dt, n_buckets)


@pytest.mark.parametrize("n_buckets", [1, 122, CAP])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 64 * 5, 64 * 9 + 1])
def test_sort_equals_from_labels(n, n_buckets):
    """n = 64 * 5: five groups on two workgroups of four waves, so the last
    three waves own no row; 64 * 9 + 1: ten waves of twelve, one row in the
    last group."""
    rng = np.random.Generator(np.random.PCG64(n * 7 + n_buckets))
    _check_sort(rng.integers(0, n_buckets, n), n_buckets)
    if n_buckets > 1 and n:
        _check_sort(np.full(n, n_buckets - 1), n_buckets)                 # one bucket: the last


def test_sort_patterns_inside_one_group():
    """64 equal labels, 64 distinct labels and two alternating labels inside
    one group of 64: alone, between two random groups (one group per wave),
    and inside intervals of two groups (more groups than waves)."""
    rng = np.random.Generator(np.random.PCG64(3))
    for mid in (np.full(64, 7), rng.permutation(64) + 20, np.tile([90, 3], 32), np.tile([3, 90], 32)):
        lab = np.concatenate([rng.integers(0, 122, 64), mid, rng.integers(0, 122, 64)]).astype(np.int64)
        _check_sort(lab, 122)
        _check_sort(mid.astype(np.int64), 122)
    # the same patterns inside intervals of several groups
    n = (MAX_WAVES + 3) * 64 + 5
    lab = rng.integers(0, 122, n)
    lab[64 * 2:64 * 3] = 7
    lab[64 * 3:64 * 4] = rng.permutation(64) + 20
    lab[64 * 5:64 * 6] = np.tile([90, 3], 32)
    _check_sort(lab, 122)


def test_sort_intervals_longer_than_one_group():
    """More rows than waves x 64: every wave's interval holds two groups, and
    the waves past ceil(groups / 2) own no row."""
    n = (MAX_WAVES + 4) * 64 + 37
    assert n > MAX_WAVES * 64
    rng = np.random.Generator(np.random.PCG64(17))
    _check_sort(rng.integers(0, 122, n), 122)
    _check_sort(rng.integers(0, 3, n), CAP)                               # most buckets empty
    _check_sort(np.sort(rng.integers(0, 122, n)), 122)                    # already sorted
    _check_sort(np.sort(rng.integers(0, 122, n))[::-1].copy(), 122)       # every row moves far


@pytest.mark.parametrize("bad", [-1, C])
def test_bad_label_raises_status_and_value_error(bad):
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    lab = w["labels"][:N].copy()
    lab[1234] = bad
    for dt in (np.int32, np.int64):
        order, off, st = _sort(torch.from_numpy(lab.astype(dt)).to(DEV), C)
        assert st & _lib.LMI_STATUS_BAD_LABEL
        # nothing is written for the row: one position of its would-be range stays unwritten
        assert (order == 1234).sum() == 0 and (order == -1).sum() == 1
    ids = np.arange(1, N + 1, dtype=np.int64)
    old = _index(w["x"][:N], w["labels"][:N], ids, 1024)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    for given in (lab, torch.from_numpy(lab.astype(np.int32)).to(DEV)):
        with pytest.raises(ValueError, match="labels must lie in"):
            old.relabel(given)
    big = lab.copy()
    big[1234] = -1 if bad < 0 else CAP + 1
    with pytest.raises(ValueError, match="labels must lie in"):           # the fallback's check
        old.relabel(big, CAP + 1)
    after = s.search(qn, q, 3, k=10, use_threshold=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_more_buckets_than_the_cap_take_the_fallback():
    """C = cap + 1 is refused by the kernel (LMI_E_UNSUPPORTED) and served by
    relabel through torch.sort(stable=True): the same tables."""
    lib = _lib.load()
    w = _w(100, "skewed")
    ids = np.arange(1, N + 1, dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(8))
    lab = torch.from_numpy(rng.integers(0, CAP + 1, N)).to(DEV)
    off = torch.zeros(CAP + 2, dtype=torch.int64, device=DEV)
    order = torch.zeros(N, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
    rc = lib.lmi_bucket_sort_labels(_lib.ptr(lab), 8, N, CAP + 1, _lib.ptr(off), _lib.ptr(order),
                                    _lib.ptr(status), _lib.ptr(ws), ws.numel() * 8, _lib.stream_handle(DEV))
    assert rc == _lib.LMI_E_UNSUPPORTED
    s = _Seq(w["x"][:N], w["labels"][:N], ids, 1024)
    labels = lab.cpu().numpy()
    labels[:2] = [CAP, 0]                                                 # the last bucket is in use
    s.relabel(labels, CAP + 1, how="dev64")
    s.relabel(labels.astype(np.int64) % CAP, CAP, how="dev32")            # the cap itself: the kernel
    s.relabel(labels, CAP + 1, how="dev32")


def test_gather_grid_strides_over_more_rows_than_one_pass():
    """70 000 rows of d = 32 are more than one pass of the gather's capped
    grid writes, so the last rows are written in a second pass of the first
    workgroups."""
    n = 70_000
    assert n > _lib.LMI_GATHER_MAX_GRID * _lib.LMI_GATHER_TILE_ROWS
    from li.index import DeviceIndex
    w = workloads.clustered(n=n, d=32, nq=1, C=4, seed=5, label_mode="router")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, n + 1, dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(2))
    new_lab = rng.integers(0, 4, n)
    got = DeviceIndex(x, lab, 4, ids=ids, device=DEV).relabel(new_lab)
    _same(got, DeviceIndex(x, new_lab, 4, ids=ids, device=DEV))


def test_byte_offsets_past_4_gib():
    """2 900 000 x 768 fp16 = 4.45 GB: the smallest corpus whose byte offsets
    pass 2^32 (and whose element offsets pass 2^31).  Everything stays on the
    device: empty().add(rows), then relabel(random labels), checked against
    rows[stable sort order of the new labels] and _inv_norm of those rows."""
    from li.index import DeviceIndex, _inv_norm
    n, d = 2_900_000, 768
    assert n * d * 2 > 2 ** 32 and n * d > 2 ** 31
    g = torch.Generator(device=DEV)
    g.manual_seed(31)
    rows = torch.empty((n, d), dtype=torch.float16, device=DEV)
    step = 1 << 18
    for a in range(0, n, step):                          # ||y||^2 ~ 1
        rows[a:a + step] = torch.randn((min(step, n - a), d), generator=g, device=DEV,
                                       dtype=torch.float32).mul_(d ** -0.5).half()
    labels = torch.randint(0, C, (n,), generator=g, device=DEV)
    new_labels = torch.randint(0, C, (n,), generator=g, device=DEV)
    index = DeviceIndex.empty(d, C, device=DEV).add(rows, labels).relabel(new_labels)
    order = torch.sort(new_labels, stable=True).indices
    assert index.n_rows == n
    assert np.array_equal(index.layout.order, order.cpu().numpy())
    assert np.array_equal(index.pos_to_id, (order + 1).cpu().numpy())
    assert np.array_equal(index.bucket_size, np.bincount(new_labels.cpu().numpy(), minlength=C))
    for a in range(0, n, step):
        want = rows.index_select(0, order[a:a + step])
        assert torch.equal(index.corpus[a:a + step], want), a
        assert torch.equal(index.inv_norm[a:a + step], _inv_norm(want)), a


def _arrays(index):
    return {k: getattr(index, k).clone() for k in ARRAYS}, \
        {k: getattr(index, k).copy() for k in HOST}


def test_old_index_is_untouched_by_a_relabel():
    from li.index import DeviceRouter, Searcher
    w = _w(768, "skewed")                                # (the batch stream takes 768-wide rows)
    ids = np.arange(1, N + 1, dtype=np.int64)
    old = _index(w["x"][:N], w["labels"][:N], ids, 1024)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    st = s.streamed(w["qn"], w["q"], 3, k=10)
    first = st.step()
    assert np.array_equal(first[0], before[0]) and np.array_equal(first[1], before[1])
    dev0, host0 = _arrays(old)
    order0, off0 = old.layout.order.copy(), old.layout.bucket_off.copy()
    ptrs = {k: getattr(old, k).data_ptr() for k in ARRAYS}
    rng = np.random.Generator(np.random.PCG64(4))
    new = old.relabel(rng.integers(0, C, N))
    new2 = new.relabel(rng.integers(0, 40, N), 40)
    assert new.n_buckets == C and new2.n_buckets == 40 and old.n_buckets == C
    for k in ARRAYS:
        assert getattr(old, k).data_ptr() == ptrs[k] and torch.equal(getattr(old, k), dev0[k]), k
        assert getattr(new, k).data_ptr() != ptrs[k], k
    for k in HOST:
        assert np.array_equal(getattr(old, k), host0[k]), k
    assert np.array_equal(old.layout.order, order0) and np.array_equal(old.layout.bucket_off, off0)
    after = s.search(qn, q, 3, k=10, use_threshold=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for _ in range(2):                                   # the captured stages still read the old buffers
        got = st.step()
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1])


@pytest.mark.parametrize("R,how", [(1, "search"), (3, "search"), (3, "f64"), (3, "streamed")])
def test_searches_over_the_relabelled_index_equal_the_rebuilt_one(R, how):
    """The real flow: the new labels are those of a second, differently seeded
    router, and that router routes the queries."""
    from li.index import DeviceRouter, Searcher
    w = _w(768, "skewed")
    x, lab = w["x"], w["labels"]
    n = N + EXTRA
    ids = np.arange(1, n + 1, dtype=np.int64)
    layers2, lab2 = _router2()
    router2 = DeviceRouter(layers2, device=DEV)
    s_old = Searcher(_index(x, lab, ids, None), router2)
    relabelled = s_old.index.relabel(lab2)
    s_new = s_old.with_index(relabelled)
    assert s_new.router is router2 and s_new.index is relabelled and s_old.index is not relabelled
    s_ref = Searcher(_index(x, lab2, ids, None), router2)
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    if how == "streamed":
        st_new, st_ref = (s.streamed(w["qn"], w["q"], R, k=10) for s in (s_new, s_ref))
        eager = s_ref.search(qn, q, R, k=10, use_threshold=True)
        for _ in range(2):
            got, want = st_new.step(), st_ref.step()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
        return
    kw = dict(k=10, use_threshold=True, dist="f64" if how == "f64" else "f32")
    got, want = s_new.search(qn, q, R, **kw), s_ref.search(qn, q, R, **kw)
    assert got[0].dtype == np.float64 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if R == 3 and how == "search":
        # the oracle over the same rows with the new labels and the new router
        classes = O.rank_classes(O.mlp_forward(w["qn"], layers2))
        ref_d, ref_a = O.search_via_lists(lab2, ids, x, w["q"], classes, C, R, k=10, use_threshold=True)
        assert O.compare_lists(ref_d, ref_a, got[0], got[1]) == 0


def test_learned_index_rebucket(monkeypatch):
    import li.index
    from li.LearnedIndex import LearnedIndex
    from li.model import data_X_to_torch
    w = _w(768, "router")
    x, xn, lab = w["x"], w["xn"], w["labels"]
    M = 120
    model = _nn(w["layers"], "MLP", C)
    layers2, _ = _router2()
    model2 = _nn(layers2, "MLP", C)
    li_ = LearnedIndex()
    li_.model = model
    nav, ds = _frames(xn[:N], x[:N], 1)
    labels = lab[:N].copy()
    li_.attach(nav, ds, labels)

    built = []
    init = li.index.DeviceIndex.__init__

    def counting(self, *a, **kw):
        built.append(1)
        return init(self, *a, **kw)

    monkeypatch.setattr(li.index.DeviceIndex, "__init__", counting)
    nav1, ds1, labels1 = li_.insert(nav, ds, labels, *_frames(xn[N:N + M], x[N:N + M], N + 1))
    li_.model = model2                                   # the retrained router
    nav2, ds2, labels2 = li_.rebucket(nav1, ds1, labels1)
    assert ds2 is ds1 and labels2.shape == (N + M,) and labels2.dtype == np.int64
    want_labels = model2.predict(data_X_to_torch(nav1.drop(columns="category")))
    assert np.array_equal(labels2, want_labels) and not np.array_equal(labels2, labels1)
    assert np.array_equal(np.asarray(nav2["category"]), labels2)
    assert np.array_equal(np.asarray(nav2.index), np.arange(1, N + M + 1))
    got = li_.search(nav2, w["qn"], ds2, w["q"], labels2, n_buckets=3, k=10, use_threshold=True)
    cls = model2.predict(data_X_to_torch(w["qn"]))
    got1 = li_.search_single(nav2, ds2, w["q"], cls, k=10)
    # explicit labels over more buckets than the model has classes
    rng = np.random.Generator(np.random.PCG64(21))
    wide = rng.integers(0, 40, N + M)
    wide[:C] = np.arange(C)
    nav3, ds3, labels3 = li_.rebucket(nav2, ds2, labels2, wide)
    assert li_._index.n_buckets == 40 and np.array_equal(labels3, wide) and labels3 is not wide
    got3 = li_.search(nav3, w["qn"], ds3, w["q"], labels3, n_buckets=3, k=10, use_threshold=True)
    cls3 = rng.integers(0, 40, w["q"].shape[0])
    got3s = li_.search_single(nav3, ds3, w["q"], cls3, k=10)
    assert built == [], "a rebucket or a search after it constructed a DeviceIndex from host rows"
    monkeypatch.setattr(li.index.DeviceIndex, "__init__", init)

    # a fresh LearnedIndex with the second model over the concatenated frames
    for lab_ref, c_ref, g, g1 in ((want_labels, cls, got, got1), (wide, cls3, got3, got3s)):
        ref = LearnedIndex()
        ref.model = model2
        rnav, rds = _frames(xn[:N + M], x[:N + M], 1)
        want = ref.search(rnav, w["qn"], rds, w["q"], lab_ref.copy(), n_buckets=3, k=10, use_threshold=True)
        want1 = ref.search_single(rnav, rds, w["q"], c_ref, k=10)
        for a, b in ((g, want), (g1, want1)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        li_.rebucket(nav3, ds3, labels3, wide[:-1])


def test_relabel_refusals():
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + 1, dtype=np.int64)
    ok = _index(x[:N], lab[:N], ids, 64)
    for wrong in (lab[:N - 1], lab[:N + 1], torch.from_numpy(lab[:N + 1]).to(DEV)):
        with pytest.raises(ValueError, match="one entry per row"):
            ok.relabel(wrong)
    with pytest.raises(ValueError):
        ok.relabel(lab[:N], 0)
    for kw, word in ((dict(storage="f32"), "storage"), (dict(rank=0, world=2), "striped"),
                     (dict(subcluster=True), "sub-cluster")):
        other = _index(x[:N], lab[:N], ids, 64, **kw)
        with pytest.raises(ValueError, match=word):
            other.relabel(lab[:other.n_total])
    x64, _ = workloads.float64_inputs(w, 3)
    other = _index(x64[:N], lab[:N], ids, 64)
    assert other.corpus64 is not None
    with pytest.raises(ValueError, match="corpus64"):
        other.relabel(lab[:N])
