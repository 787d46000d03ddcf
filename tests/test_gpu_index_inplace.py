"""K9 on the GPU: DeviceIndex.add / remove with inplace=True
(lmi_index_move_rows_inplace, csrc/lmi_update.hip) on an index built with a
capacity.  The invariant is K7's: the index an update returns is bitwise, in
every array, scalar and host table, the index a construction from scratch over
the updated row sequence gives -- here inside the SAME store, with the old
object consumed.  Comparisons are np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

import lmi_oracle as O
import workloads
from test_gpu_index_update import (ARRAYS, C, DEV, EXTRA, HOST, MOVE_MAX_GRID, MOVE_TILE_ROWS, N, _arrays,
                                   _frames, _index, _nn, _same, _Seq, _w)

pytestmark = pytest.mark.gpu

PLANS = {"staged": dict(direct_rows=10 ** 9, slab_rows=33),   # 33: no multiple of the 32-row tile
         "direct": dict(direct_rows=1, slab_rows=256),        # direct whenever legal
         "default": {}}


class _SeqInplace(_Seq):
    """_Seq whose updates run in place: after every step the from-scratch
    comparison, the same store, and the previous object consumed."""

    def __init__(self, x, labels, ids, chunk_rows, capacity, plan):
        self.x, self.labels, self.ids, self.chunk_rows = x, labels, ids, chunk_rows
        self.plan = plan
        self.index = _index(x, labels, ids, chunk_rows, capacity=capacity)
        assert self.index.capacity == capacity and self.index.n_rows == len(ids)
        self.ptrs = (self.index.corpus.data_ptr(), self.index.inv_norm.data_ptr())

    def _after(self, old):
        new = self.index
        assert new is not old and old.consumed and not new.consumed
        assert old.corpus is None and old.inv_norm is None and old.bucket_off_local is None
        assert new.capacity == old.capacity
        if new.capacity:
            assert (new._store.data_ptr(), new._store_inv.data_ptr()) == self.ptrs
        if new.n_rows:
            assert (new.corpus.data_ptr(), new.inv_norm.data_ptr()) == self.ptrs
        self.check()

    def add(self, x, labels, ids, *, as_f16=False, on_device=False, default_ids=False):
        rows = torch.from_numpy(x).half() if as_f16 else torch.from_numpy(x)
        lab = torch.from_numpy(np.asarray(labels))
        if on_device:
            rows, lab = rows.to(DEV), lab.to(DEV)
        elif not as_f16:
            rows, lab = x, labels                       # plain numpy
        old = self.index
        self.index = old.add(rows, lab, None if default_ids else ids, inplace=True, **self.plan)
        self.x = np.concatenate([self.x, x])
        self.labels = np.concatenate([self.labels, labels])
        self.ids = np.concatenate([self.ids, ids])
        self._after(old)

    def remove(self, ids):
        old = self.index
        self.index = old.remove(ids, inplace=True, **self.plan)
        keep = ~np.isin(self.ids, ids)
        self.x, self.labels, self.ids = self.x[keep], self.labels[keep], self.ids[keep]
        self._after(old)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("d", [8, 100, 768])
def test_inplace_chain_equals_rebuild(d, plan):
    w = _w(d, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(d))
    s = _SeqInplace(x[:N], lab[:N], ids[:N], 1024, N + EXTRA, PLANS[plan])
    s.check()
    sizes = np.bincount(lab[:N], minlength=C)
    big = int(np.argmax(sizes))
    small = int(np.argmin(np.where(sizes > 0, sizes, N + 1)))   # the smallest bucket with rows
    last = int(np.flatnonzero(sizes)[-1])                        # the last bucket with rows
    a = N
    s.add(x[a:a + 1], lab[a:a + 1], ids[a:a + 1], default_ids=True)
    a += 1
    s.add(x[a:a + 257], lab[a:a + 257], ids[a:a + 257], as_f16=True, on_device=True)
    a += 257
    s.add(x[a:a + 10], np.full(10, big), ids[a:a + 10], on_device=True)
    a += 10
    # bucket 0 only: every row of the corpus moves, by a small shift
    s.add(x[a:a + 6], np.full(6, 0), ids[a:a + 6])
    a += 6
    # the last non-empty bucket only: no old row moves
    s.add(x[a:a + 4], np.full(4, last), ids[a:a + 4], as_f16=True)
    a += 4
    s.remove(ids[:1])
    s.remove(s.ids[s.labels == small])
    assert s.index.bucket_size[small] == 0
    s.add(x[a:a + 5], np.full(5, small), ids[a:a + 5], as_f16=True)
    a += 5
    # m = 0 and r = 0 give an equal index (and consume the old object all the same)
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
    # remove every row, then add every row back: the store is filled to its capacity
    from li.index import DeviceIndex
    s.remove(s.ids)
    assert s.index.n_rows == 0 and s.index.capacity == N + EXTRA
    _same(s.index, DeviceIndex.empty(d, C, device=DEV, chunk_rows=1024))
    s.add(x, lab, ids, on_device=True)
    assert s.index.n_rows == s.index.capacity


def test_capacity_reserve_and_copying_updates_keep_the_capacity():
    from li.index import DeviceIndex
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    plain = _index(x[:N], lab[:N], ids[:N], 1024)
    assert plain.capacity == N and plain._store.shape[0] == N      # today's allocation
    assert plain.corpus.data_ptr() == plain._store.data_ptr()
    with pytest.raises(ValueError, match="capacity"):
        plain.add(x[N:N + 1], lab[N:N + 1], inplace=True)
    assert not plain.consumed
    big = plain.reserve(N + 50)
    assert big.capacity == N + 50 and not plain.consumed and big.corpus.data_ptr() != plain.corpus.data_ptr()
    _same(big, plain)
    with pytest.raises(ValueError):
        plain.reserve(N - 1)
    # the copying calls: a new store of max(capacity, n_new) rows, the old index untouched
    grown = big.add(x[N:N + 20], lab[N:N + 20], ids[N:N + 20])
    assert grown.capacity == N + 50 and not big.consumed
    assert grown.add(x[N + 20:N + 100], lab[N + 20:N + 100], ids[N + 20:N + 100]).capacity == N + 100
    assert grown.remove(ids[:10]).capacity == N + 50
    assert grown.relabel(np.roll(np.concatenate([lab[:N], lab[N:N + 20]]), 1)).capacity == N + 50
    _same(grown, _index(x[:N + 20], lab[:N + 20], ids[:N + 20], 1024))
    _same(grown.add(x[N + 20:N + 50], lab[N + 20:N + 50], ids[N + 20:N + 50], inplace=True),
          _index(x[:N + 50], lab[:N + 50], ids[:N + 50], 1024))
    # a capacity below the row count, or on a kind an update refuses
    with pytest.raises(ValueError, match="capacity"):
        _index(x[:N], lab[:N], ids[:N], 1024, capacity=N - 1)
    for kw in (dict(storage="f32"), dict(rank=0, world=2), dict(subcluster=True)):
        with pytest.raises(ValueError, match="capacity"):
            _index(x[:N], lab[:N], ids[:N], 64, capacity=N + 10, **kw)
    x64, _ = workloads.float64_inputs(w, 3)
    with pytest.raises(ValueError, match="capacity"):
        _index(x64[:N], lab[:N], ids[:N], 64, capacity=N + 10)
    e = DeviceIndex.empty(100, C, device=DEV, capacity=7)
    assert e.capacity == 7 and e.n_rows == 0 and e.corpus.shape == (0, 128)


def test_staged_slab_grid_strides_over_more_rows_than_one_pass():
    """One staged slab of 70 000 rows of d = 32: more than one pass of the
    capped grid (2048 workgroups x 32 rows = 65 536) in the copy to the
    staging buffer and in the move out of it."""
    n, m = 70_000, 5_000
    assert n > MOVE_MAX_GRID * MOVE_TILE_ROWS
    from li.index import DeviceIndex
    w = workloads.clustered(n=n + m, d=32, nq=1, C=4, seed=5, label_mode="router")
    x = w["x"]
    ids = np.arange(1, n + m + 1, dtype=np.int64)
    plan = dict(slab_rows=n + m, direct_rows=10 ** 9)
    # five buckets, the first one empty: every new row goes there, so all n
    # rows move, in one staged slab
    lab0 = np.concatenate([w["labels"][:n] + 1, np.zeros(m, w["labels"].dtype)])
    base = DeviceIndex(x[:n], lab0[:n], 5, ids=ids[:n], device=DEV, capacity=n + m)
    t = {}
    got = base.add(x[n:], lab0[n:], ids[n:], inplace=True, timings=t, **plan)
    assert t["staged_slabs"] == 1 and t["direct_slabs"] == 0 and t["moved_rows"] == n
    _same(got, DeviceIndex(x, lab0, 5, ids=ids, device=DEV))
    gone = ids[np.random.Generator(np.random.PCG64(1)).choice(n + m, m, replace=False)]
    gone = np.union1d(gone, got.pos_to_id[:1])             # the first row: every survivor moves
    keep = ~np.isin(ids, gone)
    t = {}
    got = got.remove(gone, inplace=True, timings=t, **plan)
    assert t["staged_slabs"] == 1 and t["direct_slabs"] == 0
    assert t["moved_rows"] > MOVE_MAX_GRID * MOVE_TILE_ROWS
    _same(got, DeviceIndex(x[keep], lab0[keep], 5, ids=ids[keep], device=DEV))


def test_inplace_byte_offsets_past_4_gib():
    """2 900 000 x 768 fp16 = 4.45 GB in a store of 1 000 rows more: byte
    offsets pass 2^32 and element offsets 2^31 inside ONE buffer.  Built as
    empty(capacity=...) plus an in-place add of everything; checked, as
    test_byte_offsets_past_4_gib checks, against rows sorted on the device."""
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
        src = torch.arange(n + m, device=DEV)[keep]
        order = src[torch.sort(labels[keep], stable=True).indices]
        assert index.n_rows == order.numel() and index.capacity == n + m
        assert index.corpus.data_ptr() == ptr0
        assert np.array_equal(index.pos_to_id, (order + 1).cpu().numpy())
        assert np.array_equal(index.bucket_size, np.bincount(labels[keep].cpu().numpy(), minlength=C))
        for a in range(0, index.n_rows, step):
            want = rows.index_select(0, order[a:a + step])
            assert torch.equal(index.corpus[a:a + step], want), a
            assert torch.equal(index.inv_norm[a:a + step], _inv_norm(want)), a

    keep = torch.zeros(n + m, dtype=torch.bool, device=DEV)
    keep[:n] = True
    index = DeviceIndex.empty(d, C, device=DEV, capacity=n + m)
    ptr0 = index._store.data_ptr()
    index = index.add(rows[:n], labels[:n], inplace=True)
    check(index, keep)
    t = {}
    index = index.add(rows[n:], labels[n:], inplace=True, timings=t)   # default ids: n + 1 ...
    assert t["direct_slabs"] + t["staged_slabs"] > 1
    keep[n:] = True
    check(index, keep)
    gone = torch.randperm(n + m, generator=g, device=DEV)[:1000]
    gone[0], gone[1] = 0, n + m - 1                       # the first and the last row
    gone = torch.unique(gone)
    index = index.remove((gone + 1).cpu().numpy(), inplace=True)
    keep[gone] = False
    check(index, keep)


def test_inplace_add_allocates_no_second_corpus():
    """The rise of the allocator's peak over an in-place add stays below half
    the corpus (staging buffer, batch and tables total under 1 MB against
    6.3 MB); over the copying add of the same batch it is at least the corpus."""
    w = workloads.clustered(n=4096 + 64, d=768, nq=1, C=C, seed=3, label_mode="skewed")
    x, lab = w["x"], w["labels"]
    n = 4096
    rows, labn = torch.from_numpy(x[n:]).half().to(DEV), lab[n:]
    index = _index(x[:n], lab[:n], None, 1024, capacity=n + 64)
    corpus_bytes = n * 768 * 2
    torch.cuda.synchronize()

    def rise(fn):
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = fn()
        return out, torch.cuda.max_memory_allocated(DEV) - base

    copied, up_copy = rise(lambda: index.add(rows, labn))
    assert up_copy >= corpus_bytes, up_copy
    del copied
    new, up_inplace = rise(lambda: index.add(rows, labn, inplace=True, slab_rows=256))
    assert up_inplace < corpus_bytes // 2, up_inplace
    _same(new, _index(x, lab, None, 1024))


@pytest.mark.parametrize("R,how", [(1, "search"), (3, "search"), (3, "f64"), (3, "streamed")])
def test_searches_over_the_inplace_updated_index_equal_the_rebuilt_one(R, how):
    from li.index import DeviceRouter, Searcher
    w = _w(768, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    router = DeviceRouter(w["layers"], device=DEV)
    s_old = Searcher(_index(x[:N], lab[:N], ids[:N], None, capacity=N + EXTRA), router)
    gone = ids[100:400]
    keep = ~np.isin(ids, gone)
    updated = s_old.index.add(x[N:], lab[N:], ids[N:], inplace=True).remove(gone, inplace=True)
    s_new = s_old.with_index(updated)
    assert s_new.router is router and s_new.index is updated and s_old.index.consumed
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
        classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
        ref_d, ref_a = O.search_via_lists(lab[keep], ids[keep], x[keep], w["q"], classes, C, R, k=10,
                                          use_threshold=True)
        assert O.compare_lists(ref_d, ref_a, got[0], got[1]) == 0


def test_consumed_objects_refuse_before_any_launch():
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    old = _index(x[:N], lab[:N], ids[:N], 1024, capacity=N + EXTRA)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    st = s.streamed(w["qn"], w["q"], 3, k=10)
    st.prime()
    gs = s.graph(w["qn"], w["q"], 3, k=10)
    gs.run()
    new = old.add(x[N:], lab[N:], ids[N:], inplace=True)
    assert old.consumed and not new.consumed
    for call in (lambda: old.add(x[:1], lab[:1], [N + EXTRA + 1]),
                 lambda: old.add(x[:1], lab[:1], [N + EXTRA + 1], inplace=True),
                 lambda: old.remove(ids[:1]),
                 lambda: old.remove(ids[:1], inplace=True),
                 lambda: old.relabel(lab[:N]),
                 lambda: old.reserve(N + EXTRA),
                 lambda: old.desc,
                 lambda: s.search(qn, q, 3, k=10, use_threshold=True),
                 lambda: s.lists(qn, q, 3, 10),
                 lambda: st.step(),
                 lambda: st.stage(w["qn"], w["q"]),
                 lambda: st.prime(),
                 lambda: gs.run(),
                 lambda: gs.stage(w["qn"], w["q"]),
                 lambda: s.streamed(w["qn"], w["q"], 3, k=10),
                 lambda: s.graph(w["qn"], w["q"], 3, k=10)):
        with pytest.raises(RuntimeError, match="in place"):
            call()
    st.close()
    gs.close()
    # with_index(new) is the way on
    got = s.with_index(new).search(qn, q, 3, k=10, use_threshold=True)
    want = Searcher(_index(x, lab, ids, 1024), s.router).search(qn, q, 3, k=10, use_threshold=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    classes = O.rank_classes(O.mlp_forward(w["qn"], w["layers"]))
    ref_d, ref_a = O.search_via_lists(lab, ids, x, w["q"], classes, C, 3, k=10, use_threshold=True)
    assert O.compare_lists(ref_d, ref_a, got[0], got[1]) == 0


def test_inplace_refusals_leave_the_index_in_use():
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    cap = N + 40
    old = _index(x[:N], lab[:N], ids[:N], 1024, capacity=cap)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    dev0, host0 = _arrays(old)
    ptrs = {k: getattr(old, k).data_ptr() for k in ARRAYS}
    bad = (x[N:N + 40].astype(np.float64) * (1.0 + 2.0 ** -13)).astype(np.float32)
    assert not np.array_equal(bad.astype(np.float16).astype(np.float32), bad)

    def unchanged():
        assert not old.consumed and old.capacity == cap and old.n_rows == N
        for k in ARRAYS:
            assert getattr(old, k).data_ptr() == ptrs[k] and torch.equal(getattr(old, k), dev0[k]), k
        for k in HOST:
            assert np.array_equal(getattr(old, k), host0[k]), k
        after = s.search(qn, q, 3, k=10, use_threshold=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

    with pytest.raises(ValueError, match="capacity") as e:
        old.add(x[N:N + 41], lab[N:N + 41], ids[N:N + 41], inplace=True)   # one row too many
    assert "reserve" in str(e.value)
    unchanged()
    for rows in (bad, torch.from_numpy(bad).to(DEV)):
        with pytest.raises(ValueError, match="fp16"):
            old.add(rows, lab[N:N + 40], ids[N:N + 40], inplace=True)
        unchanged()
    with pytest.raises(ValueError, match="duplicate"):
        old.add(x[N:N + 2], lab[N:N + 2], [N + 1, N + 1], inplace=True)
    with pytest.raises(ValueError, match="already"):
        old.add(x[N:N + 2], lab[N:N + 2], [N + 1, 7], inplace=True)
    with pytest.raises(ValueError):
        old.add(x[N:N + 2], [0, C], [N + 1, N + 2], inplace=True)          # a label out of range
    with pytest.raises(ValueError, match="duplicate"):
        old.remove([3, 3], inplace=True)
    with pytest.raises(KeyError):
        old.remove([3, N + 1], inplace=True)
    with pytest.raises(ValueError):
        old.add(x[N:N + 2], lab[N:N + 2], inplace=True, slab_rows=0)
    unchanged()
    for kw, word in ((dict(storage="f32"), "storage"), (dict(rank=0, world=2), "striped"),
                     (dict(subcluster=True), "sub-cluster")):
        other = _index(x[:N], lab[:N], ids[:N], 64, **kw)
        with pytest.raises(ValueError, match=word):
            other.add(x[N:N + 2], lab[N:N + 2], inplace=True)
        with pytest.raises(ValueError, match=word):
            other.remove([other.pos_to_id[0]], inplace=True)
        with pytest.raises(ValueError, match=word):
            other.reserve(N + 10)
        assert not other.consumed
    x64, _ = workloads.float64_inputs(w, 3)
    other = _index(x64[:N], lab[:N], ids[:N], 64)
    assert other.corpus64 is not None
    with pytest.raises(ValueError):
        other.remove([1], inplace=True)
    assert not other.consumed
    # ... and the index still takes the update it has room for
    new = old.add(x[N:N + 40], lab[N:N + 40], ids[N:N + 40], inplace=True)
    _same(new, _index(x[:N + 40], lab[:N + 40], ids[:N + 40], 1024))


def test_learned_index_insert_and_delete_in_place():
    from li.LearnedIndex import LearnedIndex
    w = _w(768, "router")
    x, xn, lab = w["x"], w["xn"], w["labels"]
    M = 120
    model = _nn(w["layers"], "MLP", C)
    gone = np.concatenate([np.arange(40, 140), np.arange(N + 3, N + 30)])
    out = {}
    for inplace in (False, True):
        li_ = LearnedIndex()
        li_.model = model
        nav, ds = _frames(xn[:N], x[:N], 1)
        labels = lab[:N].copy()
        index0 = li_.attach(nav, ds, labels, capacity=N + M if inplace else None)
        assert index0.capacity == (N + M if inplace else N)
        ptr0 = index0.corpus.data_ptr()
        new_nav, new_ds = _frames(xn[N:N + M], x[N:N + M], N + 1)
        nav2, ds2, labels2 = li_.insert(nav, ds, labels, new_nav, new_ds, inplace=inplace)
        assert index0.consumed == inplace
        index1 = li_._index
        assert (index1.corpus.data_ptr() == ptr0) == inplace
        got = li_.search(nav2, w["qn"], ds2, w["q"], labels2, n_buckets=3, k=10, use_threshold=True)
        nav3, ds3, labels3 = li_.delete(nav2, ds2, labels2, gone, inplace=inplace)
        assert index1.consumed == inplace and li_._index is not index1
        got3 = li_.search(nav3, w["qn"], ds3, w["q"], labels3, n_buckets=3, k=10, use_threshold=True)
        out[inplace] = (nav2, ds2, labels2, got, nav3, ds3, labels3, got3)
        if inplace:
            with pytest.raises(ValueError, match="capacity"):
                li_.insert(nav3, ds3, labels3, *_frames(xn[:200], x[:200], 10 ** 6), inplace=True)
            again = li_.search(nav3, w["qn"], ds3, w["q"], labels3, n_buckets=3, k=10, use_threshold=True)
            assert np.array_equal(again[0], got3[0]) and np.array_equal(again[1], got3[1])
    a, b = out[False], out[True]
    for i in (0, 1, 4, 5):
        assert a[i].equals(b[i]), i
    for i in (2, 6):
        assert np.array_equal(a[i], b[i]), i
    for i in (3, 7):
        assert np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]), i


@pytest.mark.parametrize("d", [32, 40], ids=["d32", "d40pad64"])
def test_mixed_chain_of_updates_equals_rebuild_in_every_table(d):
    """One tagged index with a capacity and a low-norm row through add, remove,
    relabel and reserve, copying and in place in turn: after every step the
    from-scratch construction over the row sequence, and beside _same what the
    successor and the store hand-over set -- tags, inv_norm64, the capacity
    rule, the store pointers, the predecessor consumed or still intact."""
    from li.index import DeviceIndex, DeviceRouter, Searcher
    n0, cap0, plan = 300, 400, dict(slab_rows=16, direct_rows=8)
    w = workloads.clustered(n=n0 + 60, d=d, nq=16, C=7, seed=21, label_mode="router")
    rng = np.random.Generator(np.random.PCG64(d))
    pool = w["x"].copy()
    pool[5] = 0
    pool[5, 3] = 2.0 ** -24                        # norm below 10 eps(float32): inv_norm64 exists
    pool[n0] = 0
    pool[n0, d - 1] = 2.0 ** -24                   # ... and the first batch brings another

    def labels(n, C_=7):                           # seven buckets, bucket 3 stays empty; five, bucket 2
        return rng.choice(np.array([0, 1, 2, 4, 5, 6] if C_ == 7 else [0, 1, 3, 4]), n)

    seq = dict(x=pool[:n0], labels=labels(n0), ids=np.arange(1, n0 + 1, dtype=np.int64),
               tags=rng.integers(0, 1 << 32, n0, dtype=np.uint64).astype(np.uint32))

    def rebuild(C_=7):
        return DeviceIndex(seq["x"], seq["labels"], C_, ids=seq["ids"], tags=seq["tags"], device=DEV)

    last = {}                                      # the rebuild the index in hand was last compared with

    def check(got, capacity, C_=None):
        want = last["want"] = rebuild(C_) if C_ else last["want"]
        _same(got, want)
        assert got.tags.dtype == want.tags.dtype and torch.equal(got.tags, want.tags)
        assert got.tags_by_pos.dtype == np.uint32 and np.array_equal(got.tags_by_pos, want.tags_by_pos)
        assert want.inv_norm64 is not None and torch.equal(got.inv_norm64, want.inv_norm64)
        assert got.capacity == capacity == got._store.shape[0] == got._store_inv.shape[0]
        assert not got.consumed

    def step(index, call, capacity, C_=7, inplace=False):
        ptrs = (index._store.data_ptr(), index._store_inv.data_ptr())
        new = call(index)
        if inplace:
            assert index.consumed and index._store is None and index.corpus is None
            assert (new._store.data_ptr(), new._store_inv.data_ptr()) == ptrs
        else:                                      # the predecessor: live, and still its own rebuild
            check(index, index.capacity)
            assert (index._store.data_ptr(), index._store_inv.data_ptr()) == ptrs
            assert new._store.data_ptr() != ptrs[0]
        check(new, capacity, C_)
        return new

    def added(a, b, C_=7):
        lab, tags = labels(b - a, C_), rng.integers(0, 1 << 32, b - a, dtype=np.uint64).astype(np.uint32)
        ids = np.arange(1000 + a, 1000 + b, dtype=np.int64)
        for k, v in (("x", pool[a:b]), ("labels", lab), ("ids", ids), ("tags", tags)):
            seq[k] = np.concatenate([seq[k], v])
        return pool[a:b], lab, ids, tags

    def removed(count):
        gone = rng.choice(seq["ids"][(seq["ids"] != 6) & (seq["ids"] != 1000 + n0)], count, replace=False)
        keep = ~np.isin(seq["ids"], gone)
        for k in seq:
            seq[k] = seq[k][keep]
        return gone

    def relabelled(C_):
        seq["labels"] = labels(len(seq["ids"]), C_)
        return seq["labels"]

    index = rebuild()
    assert index.capacity == n0
    index = DeviceIndex(seq["x"], seq["labels"], 7, ids=seq["ids"], tags=seq["tags"], device=DEV, capacity=cap0)
    check(index, cap0, 7)
    searcher = Searcher(index, DeviceRouter(w["layers"], device=DEV))
    t = {}
    batch = added(n0, n0 + 20)
    index = step(index, lambda ix: ix.add(*batch, inplace=True, timings=t, **plan), cap0, inplace=True)
    assert t["staged_slabs"] > 0 and t["direct_slabs"] > 0 and t["move_ms"] >= 0 and t["staging_rows"] <= 16
    batch = added(0, 0)                            # a batch of 0 rows
    index = step(index, lambda ix: ix.add(*batch, inplace=True, **plan), cap0, inplace=True)
    lab = relabelled(7)
    index = step(index, lambda ix: ix.relabel(torch.from_numpy(lab).to(DEV), inplace=True), cap0, inplace=True)
    gone = removed(37)
    index = step(index, lambda ix: ix.remove(gone), cap0)
    gone = removed(0)                              # removes 0 ids
    index = step(index, lambda ix: ix.remove(gone), cap0)
    lab = relabelled(5)                            # to another bucket count
    index = step(index, lambda ix: ix.relabel(lab, 5), cap0, C_=5)
    batch = added(n0 + 20, n0 + 45, 5)
    index = step(index, lambda ix: ix.add(*batch), cap0, C_=5)
    gone = removed(60)
    index = step(index, lambda ix: ix.remove(gone, inplace=True, **plan), cap0, C_=5, inplace=True)
    index = step(index, lambda ix: ix.reserve(cap0 + 50), cap0 + 50, C_=5)
    t = {}
    lab = relabelled(7)                            # ... and back, for the router's seven classes
    index = step(index, lambda ix: ix.relabel(lab, 7, inplace=True, timings=t), cap0 + 50, inplace=True)
    assert {"sort", "tables", "host", "plan", "swap", "plan_ms", "plan_rounds", "swap_ms", "swapped_rows"} <= set(t)
    assert "gather" not in t and len(t["swap_ms"]) == 2 and index.bucket_size[3] == 0
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    got = searcher.with_index(index).search(qn, q, 3, k=10, use_threshold=True, want=1)
    want = searcher.with_index(rebuild()).search(qn, q, 3, k=10, use_threshold=True, want=1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
