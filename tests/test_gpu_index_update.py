"""K7 on the GPU: DeviceIndex.add / remove (csrc/lmi_update.hip) against the
invariant of the feature -- the index an update returns is bitwise, in every
array, the index a construction from scratch over the updated row sequence
gives -- and the layers above it (Searcher.with_index, LearnedIndex.insert /
delete).  Comparisons are np.array_equal / torch.equal, never a tie window."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import lmi_oracle as O
import workloads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, EXTRA, C = 3000, 300, 16
ARRAYS = ("corpus", "inv_norm", "gpos", "bucket_off_local", "bucket_rows", "chunk_first")
SCALARS = ("n_rows", "n_total", "d", "d_pad", "storage", "chunk_rows", "n_chunks", "max_chunks")
HOST = ("pos_to_id", "bucket_size")
# the move kernel's grid: at most MOVE_MAX_GRID workgroups of MOVE_TILE_ROWS
# rows per pass (csrc/lmi_update.hip: kMoveMaxGrid, kMoveTileRows)
MOVE_MAX_GRID, MOVE_TILE_ROWS = 2048, 32


@functools.lru_cache(maxsize=None)
def _w(d, mode):
    """N base rows and EXTRA rows to add, one seeded workload per (d, mode)."""
    return workloads.clustered(n=N + EXTRA, d=d, nq=64, C=C, seed=11, label_mode=mode)


def _index(x, labels, ids, chunk_rows, **kw):
    from li.index import DeviceIndex
    return DeviceIndex(x, labels, C, ids=ids, chunk_rows=chunk_rows, device=DEV, **kw)


def _same(a, b):
    """Every array, scalar and host table of the invariant."""
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, k
        assert torch.equal(x, y), k
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))
    for k in HOST:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    assert np.array_equal(a.layout.order, b.layout.order)
    assert np.array_equal(a.layout.bucket_off, b.layout.bucket_off)
    # zero padding up to d_pad, and the layout the scan relies on
    assert not a.corpus[:, a.d:].any()
    assert a.corpus.is_contiguous() and a.corpus64 is None and a.chunk_centroid is None


class _Seq:
    """The row sequence of an index (rows, labels, ids in constructor order),
    updated beside the index and rebuilt from scratch for the comparison."""

    def __init__(self, x, labels, ids, chunk_rows):
        self.x, self.labels, self.ids, self.chunk_rows = x, labels, ids, chunk_rows
        self.index = _index(x, labels, ids, chunk_rows)

    def check(self):
        _same(self.index, _index(self.x, self.labels, self.ids, self.chunk_rows, storage="f16"))

    def add(self, x, labels, ids, *, as_f16=False, on_device=False, default_ids=False):
        rows = torch.from_numpy(x).half() if as_f16 else torch.from_numpy(x)
        lab = torch.from_numpy(np.asarray(labels))
        if on_device:
            rows, lab = rows.to(DEV), lab.to(DEV)
        elif not as_f16:
            rows, lab = x, labels                       # plain numpy
        self.index = self.index.add(rows, lab, None if default_ids else ids)
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
def test_update_equals_rebuild(d, mode, chunk_rows):
    w = _w(d, mode)
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)   # the constructor's default ids
    rng = np.random.Generator(np.random.PCG64(d))
    s = _Seq(x[:N], lab[:N], ids[:N], chunk_rows)
    s.check()
    sizes = np.bincount(lab[:N], minlength=C)
    big = int(np.argmax(sizes))
    small = int(np.argmin(np.where(sizes > 0, sizes, N + 1)))   # the smallest bucket with rows
    a = N
    # add m = 1 (default ids continue after the largest), fp32 host rows
    s.add(x[a:a + 1], lab[a:a + 1], ids[a:a + 1], default_ids=True)
    a += 1
    # add m = 257, fp16 rows on the device, labels on the device
    s.add(x[a:a + 257], lab[a:a + 257], ids[a:a + 257], as_f16=True, on_device=True)
    a += 257
    # rows all into one bucket: fp32 rows on the device
    s.add(x[a:a + 10], np.full(10, big), ids[a:a + 10], on_device=True)
    a += 10
    # remove 1, remove a whole bucket, then add into the bucket that is now empty (fp16 host rows)
    s.remove(ids[:1])
    s.remove(s.ids[s.labels == small])
    assert s.index.bucket_size[small] == 0
    s.add(x[a:a + 5], np.full(5, small), ids[a:a + 5], as_f16=True)
    a += 5
    never = np.flatnonzero(sizes == 0)
    if never.size:                                      # a bucket that never held a row
        s.add(x[a:a + 3], np.full(3, never[0]), ids[a:a + 3])
        a += 3
    # m = 0 and r = 0 give an equal index
    s.add(x[:0], lab[:0], ids[:0])
    s.remove(ids[:0])
    # remove + add chained three times, ids that come back after their removal included
    for j in range(3):
        gone = rng.choice(s.ids, 150 + 50 * j, replace=False)
        back = np.isin(ids[:N], gone)
        s.remove(gone)
        m = 4 + j
        s.add(np.concatenate([x[:N][back], x[a:a + m]]), np.concatenate([lab[:N][back], lab[a:a + m]]),
              np.concatenate([ids[:N][back], ids[a:a + m]]), on_device=bool(j & 1))
        a += m
    assert a <= N + EXTRA
    # remove every row: the empty index of a fresh construction, and of empty()
    from li.index import DeviceIndex
    s.remove(s.ids)
    assert s.index.n_rows == 0
    _same(s.index, DeviceIndex.empty(d, C, device=DEV, chunk_rows=chunk_rows))
    # ... which takes every row back: built as empty().add(all rows), no host sort
    s.add(x, lab, ids, on_device=True)


def test_inv_norm_of_zero_and_subnormal_rows_is_inv_norms():
    from li.index import _inv_norm
    w = _w(100, "skewed")
    x = w["x"][N:N + 6].copy()
    x[1] = 0.0                                           # norm 0 -> 1 (the zero rule)
    x[2] = 2.0 ** -22                                    # fp16 subnormals everywhere, norm 10 * 2^-22
    x[3] = 0.0
    x[3, 7] = 2.0 ** -24                                 # norm 2^-24 < 10 eps: the zero rule
    x[4] = 0.0
    x[4, :3] = [2.0 ** -15, -2.0 ** -24, 3 * 2.0 ** -24]  # subnormals, norm above 10 eps
    lab = np.array([0, 3, 3, 5, 5, 9])
    ids = np.arange(1, N + 7, dtype=np.int64)
    for rows in (x, torch.from_numpy(x).half().to(DEV)):
        s = _Seq(w["x"][:N], w["labels"][:N], ids[:N], 1024)
        s.index = s.index.add(rows, lab, ids[N:])
        at = np.array([int(np.flatnonzero(s.index.pos_to_id == i)[0]) for i in ids[N:]])
        stored = s.index.corpus[torch.from_numpy(at).to(DEV)]
        assert torch.equal(stored[:, :100].float().cpu(), torch.from_numpy(x))
        got = s.index.inv_norm[torch.from_numpy(at).to(DEV)]
        assert torch.equal(got, _inv_norm(stored))
        assert got[1].item() == 1.0 and got[3].item() == 1.0
        assert got[2].item() != 1.0 and got[4].item() != 1.0
        s.x, s.labels, s.ids = np.concatenate([s.x, x]), np.concatenate([s.labels, lab]), ids
        s.check()


def test_move_grid_strides_over_more_rows_than_one_pass():
    """70 000 rows of d = 32 are more than one pass of the capped grid covers
    (2048 workgroups x 32 rows = 65 536), so the last rows move in a second
    pass of the first workgroups."""
    n, m = 70_000, 5_000
    assert n > MOVE_MAX_GRID * MOVE_TILE_ROWS
    from li.index import DeviceIndex
    w = workloads.clustered(n=n + m, d=32, nq=1, C=4, seed=5, label_mode="router")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, n + m + 1, dtype=np.int64)
    base = DeviceIndex(x[:n], lab[:n], 4, ids=ids[:n], device=DEV)
    got = base.add(x[n:], lab[n:], ids[n:])
    _same(got, DeviceIndex(x, lab, 4, ids=ids, device=DEV))
    gone = ids[np.random.Generator(np.random.PCG64(1)).choice(n + m, m, replace=False)]
    keep = ~np.isin(ids, gone)
    _same(got.remove(gone), DeviceIndex(x[keep], lab[keep], 4, ids=ids[keep], device=DEV))


def test_byte_offsets_past_4_gib():
    """2 900 000 x 768 fp16 = 4.45 GB: the smallest corpus whose byte offsets
    pass 2^32 (and whose element offsets pass 2^31).  Everything stays on the
    device: the index is built as empty().add(all rows) and checked against
    rows_all[stable sort order of the labels] and _inv_norm of those rows."""
    from li.index import DeviceIndex, _inv_norm
    n, d, m = 2_900_000, 768, 1_000
    assert n * d * 2 > 2 ** 32 and n * d > 2 ** 31
    g = torch.Generator(device=DEV)
    g.manual_seed(29)
    rows = torch.empty((n + m, d), dtype=torch.float16, device=DEV)
    step = 1 << 18
    for a in range(0, n + m, step):                      # ||y||^2 ~ 1
        rows[a:a + step] = torch.randn((min(step, n + m - a), d), generator=g, device=DEV,
                                       dtype=torch.float32).mul_(d ** -0.5).half()
    labels = torch.randint(0, C, (n + m,), generator=g, device=DEV)

    def check(index, keep):
        """index against the kept rows of `rows`, bucket-sorted on the device."""
        src = torch.arange(n + m, device=DEV)[keep]
        order = src[torch.sort(labels[keep], stable=True).indices]
        assert index.n_rows == order.numel()
        assert np.array_equal(index.pos_to_id, (order + 1).cpu().numpy())
        assert np.array_equal(index.bucket_size, np.bincount(labels[keep].cpu().numpy(), minlength=C))
        for a in range(0, index.n_rows, step):
            want = rows.index_select(0, order[a:a + step])
            assert torch.equal(index.corpus[a:a + step], want), a
            assert torch.equal(index.inv_norm[a:a + step], _inv_norm(want)), a

    keep = torch.zeros(n + m, dtype=torch.bool, device=DEV)
    keep[:n] = True
    index = DeviceIndex.empty(d, C, device=DEV).add(rows[:n], labels[:n])
    check(index, keep)
    index = index.add(rows[n:], labels[n:])              # default ids: n + 1 ...
    keep[n:] = True
    check(index, keep)
    gone = torch.randperm(n + m, generator=g, device=DEV)[:1000]
    gone[0], gone[1] = 0, n + m - 1                       # the first and the last row
    gone = torch.unique(gone)
    index = index.remove((gone + 1).cpu().numpy())
    keep[gone] = False
    check(index, keep)


def _arrays(index):
    return {k: getattr(index, k).clone() for k in ARRAYS}, \
        {k: getattr(index, k).copy() for k in HOST}


def test_old_index_is_untouched_by_updates():
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    old = _index(w["x"][:N], w["labels"][:N], ids[:N], 1024)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    dev0, host0 = _arrays(old)
    ptrs = {k: getattr(old, k).data_ptr() for k in ARRAYS}
    new = old.add(w["x"][N:], w["labels"][N:], ids[N:])
    new2 = new.remove(ids[5:900])
    assert new.n_rows == N + EXTRA and new2.n_rows == N + EXTRA - 895 and old.n_rows == N
    for k in ARRAYS:
        assert getattr(old, k).data_ptr() == ptrs[k] and torch.equal(getattr(old, k), dev0[k]), k
        assert getattr(new, k).data_ptr() != ptrs[k], k
    for k in HOST:
        assert np.array_equal(getattr(old, k), host0[k]), k
    after = s.search(qn, q, 3, k=10, use_threshold=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("R,how", [(1, "search"), (3, "search"), (3, "f64"), (3, "streamed")])
def test_searches_over_the_updated_index_equal_the_rebuilt_one(R, how):
    from li.index import DeviceRouter, Searcher
    w = _w(768, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    router = DeviceRouter(w["layers"], device=DEV)
    s_old = Searcher(_index(x[:N], lab[:N], ids[:N], None), router)
    gone = ids[100:400]
    keep = ~np.isin(ids, gone)
    updated = s_old.index.add(x[N:], lab[N:], ids[N:]).remove(gone)
    s_new = s_old.with_index(updated)
    assert s_new.router is router and s_new.index is updated and s_old.index is not updated
    s_ref = Searcher(_index(x[keep], lab[keep], ids[keep], None), router)
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
        # the oracle over the updated row sequence (survivors, then the batch)
        classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
        ref_d, ref_a = O.search_via_lists(lab[keep], ids[keep], x[keep], w["q"], classes, C, R, k=10,
                                          use_threshold=True)
        assert O.compare_lists(ref_d, ref_a, got[0], got[1]) == 0


def test_refusals_leave_the_old_index_in_use():
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    old = _index(x[:N], lab[:N], ids[:N], 1024)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    bad = (x[N:N + 40].astype(np.float64) * (1.0 + 2.0 ** -13)).astype(np.float32)
    assert not np.array_equal(bad.astype(np.float16).astype(np.float32), bad)
    for rows in (bad, torch.from_numpy(bad).to(DEV)):
        with pytest.raises(ValueError, match="fp16"):
            old.add(rows, lab[N:N + 40], ids[N:N + 40])
    after = s.search(qn, q, 3, k=10, use_threshold=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    ref_d, ref_a = O.search_via_lists(lab[:N], ids[:N], x[:N], w["q"], classes, C, 3, k=10,
                                      use_threshold=True)
    assert O.compare_lists(ref_d, ref_a, after[0], after[1]) == 0
    with pytest.raises(ValueError, match="duplicate"):
        old.add(x[N:N + 2], lab[N:N + 2], [N + 1, N + 1])
    with pytest.raises(ValueError, match="already"):
        old.add(x[N:N + 2], lab[N:N + 2], [N + 1, 7])
    with pytest.raises(ValueError):
        old.add(x[N:N + 2], lab[N:N + 3], [N + 1, N + 2])          # one label too many
    with pytest.raises(ValueError):
        old.add(x[N:N + 2], [0, C], [N + 1, N + 2])                # a label out of range
    with pytest.raises(ValueError):
        old.add(x[N:N + 2, :50], lab[N:N + 2])                     # rows of another width
    with pytest.raises(KeyError):
        old.remove([3, N + 1])
    for kw, word in ((dict(storage="f32"), "storage"), (dict(rank=0, world=2), "striped"),
                     (dict(subcluster=True), "sub-cluster")):
        other = _index(x[:N], lab[:N], ids[:N], 64, **kw)
        with pytest.raises(ValueError, match=word):
            other.add(x[N:N + 2], lab[N:N + 2])
        with pytest.raises(ValueError, match=word):
            other.remove([other.pos_to_id[0]])
    x64, _ = workloads.float64_inputs(w, 3)
    other = _index(x64[:N], lab[:N], ids[:N], 64)
    assert other.corpus64 is not None
    with pytest.raises(ValueError):
        other.remove([1])


def _nn(layers, arch, n_classes):
    from li.model import NeuralNetwork
    nn = NeuralNetwork(input_dim=96, output_dim=n_classes, lr=0.009, model_type=arch)
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, layers):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    return nn


def _frames(xn, x, first_id):
    nav, ds = pd.DataFrame(xn), pd.DataFrame(x)
    nav.index += first_id
    ds.index += first_id
    return nav, ds


def test_learned_index_insert_and_delete(monkeypatch):
    import li.index
    from li.LearnedIndex import LearnedIndex
    from li.model import data_X_to_torch
    w = _w(768, "router")
    x, xn, lab = w["x"], w["xn"], w["labels"]
    M = 120
    model = _nn(w["layers"], "MLP", C)
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
    new_nav, new_ds = _frames(xn[N:N + M], x[N:N + M], N + 1)
    nav2, ds2, labels2 = li_.insert(nav, ds, labels, new_nav, new_ds)
    assert nav2.shape[0] == N + M and ds2.shape[0] == N + M and labels2.shape == (N + M,)
    assert np.array_equal(labels2[:N], labels)
    assert np.array_equal(labels2[N:], model.predict(data_X_to_torch(new_nav)))
    assert np.array_equal(labels2[N:], lab[N:N + M])        # (router-mode labels: O.predict)
    got = li_.search(nav2, w["qn"], ds2, w["q"], labels2, n_buckets=3, k=10, use_threshold=True)
    cls = model.predict(data_X_to_torch(w["qn"]))
    got1 = li_.search_single(nav2, ds2, w["q"], cls, k=10)
    # delete: some old objects and some of the inserted ones
    gone = np.concatenate([np.arange(40, 140), np.arange(N + 3, N + 30)])
    nav3, ds3, labels3 = li_.delete(nav2, ds2, labels2, gone)
    got3 = li_.search(nav3, w["qn"], ds3, w["q"], labels3, n_buckets=3, k=10, use_threshold=True)
    got3s = li_.search_single(nav3, ds3, w["q"], cls, k=10)
    assert built == [], "an update or a search after it constructed a DeviceIndex from host rows"
    monkeypatch.setattr(li.index.DeviceIndex, "__init__", init)

    # a fresh LearnedIndex with the same model over the concatenated frames
    ref = LearnedIndex()
    ref.model = model
    rnav, rds = _frames(xn[:N + M], x[:N + M], 1)
    want = ref.search(rnav, w["qn"], rds, w["q"], labels2.copy(), n_buckets=3, k=10, use_threshold=True)
    want1 = ref.search_single(rnav, rds, w["q"], cls, k=10)
    for g, r in ((got, want), (got1, want1)):
        assert np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1])
    keep = ~np.isin(np.arange(1, N + M + 1), gone)
    ref3 = LearnedIndex()
    ref3.model = model
    rnav3, rds3 = rnav[keep].drop(columns="category"), rds[keep]
    want3 = ref3.search(rnav3, w["qn"], rds3, w["q"], labels2[keep], n_buckets=3, k=10,
                        use_threshold=True)
    want3s = ref3.search_single(rnav3, rds3, w["q"], cls, k=10)
    for g, r in ((got3, want3), (got3s, want3s)):
        assert np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1])
    # ids that collide, unknown ids
    with pytest.raises(ValueError):
        li_.insert(nav3, ds3, labels3, *_frames(xn[:2], x[:2], 1))
    with pytest.raises(KeyError):
        li_.delete(nav3, ds3, labels3, [45])
