"""K10 on the GPU: DeviceIndex.relabel(inplace=True) -- the gather of a relabel
as two passes of disjoint row swaps inside the index's own store
(lmi_perm_involutions, lmi_index_swap_rows; csrc/lmi_rebucket.hip).  The plan
is compared bit for bit with its numpy restatement below, the swap kernel with
torch.index_select on raw 16-bit patterns, and the index with what relabel()
and a construction from scratch give (K8's invariant, in the SAME store, with
the old object consumed).  Comparisons are np.array_equal / torch.equal."""
import functools

import numpy as np
import pytest
import torch

import lmi_oracle as O
from li import _lib
from test_gpu_index_rebucket import C, DEV, EXTRA, N, _index, _router2, _w
from test_gpu_index_update import ARRAYS, HOST, _arrays, _frames, _nn, _same

pytestmark = pytest.mark.gpu

MAX_GRID, TILE_ROWS = _lib.LMI_GATHER_MAX_GRID, _lib.LMI_GATHER_TILE_ROWS


# ---- the plan ----------------------------------------------------------------------
def plan_np(sigma):
    """The plan of include/lmi_hip.h, restated: on every cycle of sigma with
    e_0 = its smallest position, e_(t+1) = sigma(e_t) and length m,
    partner1[e_t] = e_((m - t) mod m) and partner2[e_t] = e_(m - 1 - t)."""
    n = len(sigma)
    p1, p2 = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    seen = np.zeros(n, bool)
    nxt = sigma.tolist()
    for L in range(n):
        if seen[L]:
            continue
        e, q = [L], nxt[L]
        while q != L:
            e.append(q)
            q = nxt[q]
        e = np.asarray(e, np.int64)
        seen[e] = True
        m, t = e.size, np.arange(e.size)
        p1[e] = e[(m - t) % m]
        p2[e] = e[m - 1 - t]
    return p1, p2


def swaps_np(rows, partner):
    out = rows.copy()
    j = np.flatnonzero(partner > np.arange(partner.size))
    out[j], out[partner[j]] = rows[partner[j]], rows[j]
    return out


def cycles_1_to_9():
    """Cycles of every length from 1 to 9, one after the other (45 positions)."""
    sigma, a = [], 0
    for m in range(1, 10):
        sigma += [a + (t + 1) % m for t in range(m)]
        a += m
    return np.asarray(sigma, np.int64)


def perms(n):
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    at = np.arange(n, dtype=np.int64)
    out = {"identity": at.copy(), "reversal": at[::-1].copy(), "rot+1": np.roll(at, -1),
           "rot-1": np.roll(at, 1), "rot_half": np.roll(at, n // 2)}
    for i in range(3):
        out[f"random{i}"] = rng.permutation(n).astype(np.int64)
    return out


def plan_gpu(sigma):
    """lmi_perm_involutions over a workspace of junk: (partner1, partner2, status)."""
    lib = _lib.load()
    s = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.int64)).to(DEV)
    n = int(s.numel())
    p1 = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    p2 = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.lmi_perm_involutions_ws_bytes(n)
    ws = torch.full((max(need, 16) // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    _lib.check("lmi_perm_involutions", lib.lmi_perm_involutions(
        _lib.ptr(s), n, _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(status), _lib.ptr(ws), need,
        _lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    return p1.cpu().numpy(), p2.cpu().numpy(), int(status.item())


def check_plan(sigma):
    n = sigma.size
    want1, want2 = plan_np(sigma)
    at = np.arange(n)
    for w in (want1, want2):                              # the restatement itself: two involutions ...
        assert np.array_equal(w[w], at)
    rows = np.random.Generator(np.random.PCG64(n)).integers(0, 1 << 30, n)
    assert np.array_equal(swaps_np(swaps_np(rows, want1), want2), rows[sigma])   # ... that give the gather
    p1, p2, st = plan_gpu(sigma)
    assert st == 0
    assert p1.dtype == want1.dtype and np.array_equal(p1, want1)
    assert p2.dtype == want2.dtype and np.array_equal(p2, want2)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 64, 65, 1000, 65537])
def test_plan_equals_its_numpy_restatement(n):
    for name, sigma in perms(n).items():
        check_plan(sigma)


def test_plan_of_cycles_of_every_length_from_1_to_9():
    """Even lengths have a pass-1 midpoint that stays (t = m / 2), odd lengths
    a pass-2 midpoint (t = (m - 1) / 2); a 2-cycle swaps in pass 2 only."""
    sigma = cycles_1_to_9()
    check_plan(sigma)
    p1, p2, st = plan_gpu(sigma)
    at, a = np.arange(45), 0
    for m in range(1, 10):
        fixed1, fixed2 = np.flatnonzero(p1[a:a + m] == at[a:a + m]), np.flatnonzero(p2[a:a + m] == at[a:a + m])
        assert fixed1.tolist() == ([0, m // 2] if m % 2 == 0 else [0]), m
        assert fixed2.tolist() == ([(m - 1) // 2] if m % 2 else []), m
        a += m
    assert np.array_equal(p1[1:3], [1, 2]) and np.array_equal(p2[1:3], [2, 1])   # the 2-cycle
    # the same cycles under a random renaming of the positions, inside a larger permutation
    rng = np.random.Generator(np.random.PCG64(45))
    big = np.concatenate([sigma, 45 + rng.permutation(300)])
    name = rng.permutation(big.size)
    conj = np.empty_like(big)
    conj[name] = name[big]
    check_plan(conj)


@pytest.mark.parametrize("n", [2, 5, 1000, 65537])
def test_plan_refuses_what_is_no_permutation(n):
    sigma = np.random.Generator(np.random.PCG64(n)).permutation(n).astype(np.int64)
    for at, value in ((n // 2, sigma[(n // 2 + 1) % n]),   # a repeated entry (another one missing)
                      (n - 1, n), (0, -1), (n // 3, 2 ** 40)):   # out of range
        bad = sigma.copy()
        bad[at] = value
        assert plan_gpu(bad)[2] == _lib.LMI_STATUS_BAD_PERM, (at, value)
    assert plan_gpu(np.zeros(n, np.int64))[2] == _lib.LMI_STATUS_BAD_PERM
    assert plan_gpu(sigma)[2] == 0


# ---- the swap kernel ---------------------------------------------------------------
def swap_gpu(corpus, inv, partner, status):
    lib = _lib.load()
    _lib.check("lmi_index_swap_rows", lib.lmi_index_swap_rows(
        _lib.ptr(corpus), _lib.ptr(inv), corpus.shape[0], corpus.shape[1], _lib.ptr(partner),
        _lib.ptr(status), _lib.stream_handle(DEV)))


def raw_rows(n, d_pad, seed):
    """Random 16-bit patterns (NaN and infinity encodings among them) and
    random 32-bit patterns for inv_norm, as integers."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    corpus = torch.randint(0, 1 << 16, (n, d_pad), generator=g, device=DEV, dtype=torch.int32).to(torch.int16)
    inv = torch.randint(0, 1 << 32, (n,), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    return corpus, inv


@pytest.mark.parametrize("n,d", [(1000, 8), (1000, 100), (1000, 768), (1000, 992), (33, 100), (1, 8),
                                 (65537, 8)])
def test_two_swap_passes_equal_index_select(n, d):
    """d = 8, 100, 768, 992: rows of 4, 16, 96 and 124 16-byte pieces.
    n = 65537 at d = 8: more rows than one pass of the capped grid covers."""
    d_pad = (d + 31) // 32 * 32
    assert d_pad // 8 in (4, 16, 96, 124)
    if n == 65537:
        assert n > MAX_GRID * TILE_ROWS
    corpus, inv = raw_rows(n, d_pad, n + d)
    if n >= 1000:                                         # NaN patterns: exponent all ones, mantissa not 0
        assert bool((((corpus & 0x7C00) == 0x7C00) & ((corpus & 0x03FF) != 0)).any())
    for name, sigma in perms(n).items():
        sig = torch.from_numpy(sigma).to(DEV)
        want, want_inv = corpus.index_select(0, sig), inv.index_select(0, sig)
        p1, p2 = (torch.from_numpy(p).to(DEV) for p in plan_np(sigma))
        got, got_inv = corpus.clone(), inv.clone()
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        swap_gpu(got.view(torch.float16), got_inv.view(torch.float32), p1, status)
        swap_gpu(got.view(torch.float16), got_inv.view(torch.float32), p2, status)
        assert int(status.item()) == 0
        assert torch.equal(got, want) and torch.equal(got_inv, want_inv), name


@pytest.mark.parametrize("how", ["not_an_involution", "above_range", "below_range"])
def test_swap_skips_a_pair_that_fails_its_check(how):
    n, d_pad = 1000, 128
    corpus, inv = raw_rows(n, d_pad, 5)
    sigma = perms(n)["random1"]
    partner = plan_np(sigma)[1]
    a = int(np.flatnonzero(partner > np.arange(n))[17])
    b = int(partner[a])
    bad = partner.copy()
    if how == "not_an_involution":
        c = int(np.flatnonzero((partner != np.arange(n)) & (np.arange(n) != a) & (np.arange(n) != b))[5])
        bad[b] = c                                        # a -> b -> c -> partner[c] != b
    else:
        bad[a] = n + 5 if how == "above_range" else -1    # b -> a, a -> nowhere
    want, want_inv = corpus.clone(), inv.clone()
    ok = torch.from_numpy(partner).to(DEV)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[[a, b]] = False
    want[keep], want_inv[keep] = corpus[ok][keep], inv[ok][keep]   # every valid pair; a and b as they were
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got, got_inv = corpus.clone(), inv.clone()
    swap_gpu(got.view(torch.float16), got_inv.view(torch.float32), torch.from_numpy(bad).to(DEV), status)
    assert int(status.item()) == _lib.LMI_STATUS_INTERNAL
    assert torch.equal(got[[a, b]], corpus[[a, b]]) and torch.equal(got_inv[[a, b]], inv[[a, b]])
    assert torch.equal(got, want) and torch.equal(got_inv, want_inv)


def test_swap_byte_offsets_past_4_gib():
    """2 900 000 x 768 fp16 = 4.45 GB in one store: byte offsets pass 2^32 and
    element offsets 2^31.  The permutation is the identity but for 2- and
    3-cycles whose rows lie on both sides of the 4 GiB line (row 2 796 202 is
    the one the line cuts); those rows are compared, the rest by a sample."""
    n, d = 2_900_000, 768
    line = 2 ** 32 // (2 * d)
    assert n * d * 2 > 2 ** 32 and n * d > 2 ** 31 and line == 2_796_202 and line + 5 < n
    g = torch.Generator(device=DEV)
    g.manual_seed(41)
    corpus = torch.empty((n, d), dtype=torch.int16, device=DEV)
    step = 1 << 18
    for a in range(0, n, step):
        corpus[a:a + step] = torch.randint(0, 1 << 16, (min(step, n - a), d), generator=g, device=DEV,
                                           dtype=torch.int32).to(torch.int16)
    inv = torch.randint(0, 1 << 32, (n,), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    orig, orig_inv = corpus.clone(), inv.clone()
    cycles = [(5, line + 100), (line, line + 1), (line - 1, n - 1), (0, line + 2),
              (100, n - 2, line - 3), (line + 3, 7, line + 4), (line - 2, line + 5, 3000)]
    sigma = np.arange(n, dtype=np.int64)
    for cyc in cycles:
        for t, e in enumerate(cyc):
            sigma[e] = cyc[(t + 1) % len(cyc)]
    touched = torch.tensor(sorted(e for cyc in cycles for e in cyc), device=DEV)
    lib = _lib.load()
    sig = torch.from_numpy(sigma).to(DEV)
    p1 = torch.empty(n, dtype=torch.int64, device=DEV)
    p2 = torch.empty(n, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.lmi_perm_involutions_ws_bytes(n)
    ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
    _lib.check("lmi_perm_involutions", lib.lmi_perm_involutions(
        _lib.ptr(sig), n, _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(status), _lib.ptr(ws), need,
        _lib.stream_handle(DEV)))
    assert int(status.item()) == 0
    del ws
    at = torch.arange(n, device=DEV)
    moved1, moved2 = int((p1 != at).sum()), int((p2 != at).sum())
    assert 0 < moved1 <= len(touched) and 0 < moved2 <= len(touched)
    swap_gpu(corpus.view(torch.float16), inv.view(torch.float32), p1, status)
    swap_gpu(corpus.view(torch.float16), inv.view(torch.float32), p2, status)
    assert int(status.item()) == 0
    src = sig[touched]
    assert torch.equal(corpus[touched], orig[src]) and torch.equal(inv[touched], orig_inv[src])
    assert not torch.equal(corpus[touched], orig[touched])
    sample = torch.randint(0, n, (100_000,), generator=g, device=DEV)
    sample = torch.cat([sample, torch.arange(line - 64, line + 64, device=DEV), at[:64], at[-64:]])
    sample = sample[~torch.isin(sample, touched)]
    assert torch.equal(corpus[sample], orig[sample]) and torch.equal(inv[sample], orig_inv[sample])


# ---- relabel(inplace=True) -----------------------------------------------------------
class _SeqInplace:
    """The row sequence of an index beside the index; every relabel runs three
    ways -- copying, in place, and as a construction from scratch."""

    def __init__(self, x, labels, ids, chunk_rows, n_buckets=C, capacity=None):
        self.x, self.labels, self.ids = x, np.asarray(labels, np.int64), ids
        self.chunk_rows, self.C, self.capacity = chunk_rows, n_buckets, capacity
        self.index = _index(x, labels, ids, chunk_rows, n_buckets, capacity=capacity)

    def rebuilt(self):
        return _index(self.x, self.labels, self.ids, self.chunk_rows, self.C, storage="f16")

    def relabel(self, labels, n_buckets=None, on_device=False):
        labels = np.asarray(labels, np.int64)
        given = torch.from_numpy(labels.astype(np.int32)).to(DEV) if on_device else labels
        old = self.index
        ptrs = (old._store.data_ptr(), old._store_inv.data_ptr(), old.capacity)
        copied = old.relabel(given, n_buckets)
        assert not old.consumed
        t = {}
        new = old.relabel(given, n_buckets, inplace=True, timings=t)
        assert new is not old and old.consumed and not new.consumed
        assert old.corpus is None and old.inv_norm is None and old.bucket_off_local is None
        assert (new._store.data_ptr(), new._store_inv.data_ptr(), new.capacity) == ptrs
        assert new.capacity == (self.capacity or new.n_rows)
        if new.n_rows:
            assert (new.corpus.data_ptr(), new.inv_norm.data_ptr()) == ptrs[:2]
            assert {"sort", "tables", "plan", "swap", "host"} <= set(t) and "gather" not in t
        self.index, self.labels = new, labels
        if n_buckets is not None:
            self.C = n_buckets
        assert new.n_buckets == self.C and new.layout.n_buckets == self.C
        _same(new, copied)
        _same(new, self.rebuilt())
        return t


@pytest.mark.parametrize("reserved", [False, True], ids=["tight", "reserved"])
@pytest.mark.parametrize("mode", ["router", "skewed"])
@pytest.mark.parametrize("d", [8, 100, 768])
def test_relabel_inplace_equals_relabel_and_rebuild(d, mode, reserved):
    w = _w(d, mode)
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64) * 3 + 1            # (not the default ids)
    rng = np.random.Generator(np.random.PCG64(200 + d))
    s = _SeqInplace(x[:N], lab[:N], ids[:N], 1024, capacity=N + EXTRA if reserved else None)
    # the same labels: no row moves, yet a new object over the same store
    t = s.relabel(lab[:N])
    assert t["swapped_rows"] == [0, 0]
    # a permutation of the bucket names, then uniformly random labels: every row moves
    s.relabel(rng.permutation(C)[lab[:N]], on_device=True)
    t = s.relabel(rng.integers(0, C, N))
    assert min(t["swapped_rows"]) > N // 2
    # more buckets, fewer, more than rows per bucket can fill (empty buckets)
    s.relabel(rng.integers(0, 122, N), 122, on_device=True)
    s.relabel(rng.integers(0, 7, N), 7)
    s.relabel(rng.integers(0, 122, N), 122)
    s.relabel(rng.integers(0, 300, N), 300, on_device=True)
    # labels that leave the first, a middle and the last bucket empty; one bucket
    live = np.setdiff1d(np.arange(300), [0, 150, 299])
    s.relabel(rng.choice(live, N), 300)
    assert not s.index.bucket_size[[0, 150, 299]].any()
    s.relabel(np.zeros(N, np.int64), 1)
    s.relabel(lab[:N], C)
    if not reserved:
        return
    # a chain inside one store: add in place, relabel in place, remove in place
    store0 = s.index._store.data_ptr()
    s.index = s.index.add(x[N:N + 257], lab[N:N + 257], ids[N:N + 257], inplace=True)
    s.x, s.ids = x[:N + 257], ids[:N + 257]
    s.relabel(rng.integers(0, C, N + 257), on_device=True)
    gone = rng.choice(s.ids, 150, replace=False)
    keep = ~np.isin(s.ids, gone)
    got = s.index.remove(gone, inplace=True)
    assert got.capacity == N + EXTRA and got._store.data_ptr() == store0
    _same(got, _index(s.x[keep], s.labels[keep], s.ids[keep], 1024, C, storage="f16"))


def test_relabel_inplace_of_no_rows_and_of_one_row():
    w = _w(100, "skewed")
    ids = np.arange(1, N + 1, dtype=np.int64)
    z = _SeqInplace(w["x"][:0], w["labels"][:0], ids[:0], 1024)
    z.relabel(w["labels"][:0], 5)
    one = _SeqInplace(w["x"][:1], w["labels"][:1], ids[:1], 1024)
    one.relabel(np.asarray([3]), 5)


def test_relabel_inplace_carries_inv_norm64():
    """A row whose norm lies below 10 eps(float32): the new index recomputes
    inv_norm64 from the rows where they now are, as the copying path does."""
    w = _w(100, "skewed")
    x, lab = w["x"][:N].copy(), w["labels"][:N]
    for r in (7, 1500, N - 1):
        x[r] = 0
        x[r, r % 100] = 2.0 ** -20
    ids = np.arange(1, N + 1, dtype=np.int64)
    base = _index(x, lab, ids, 1024)
    assert base.inv_norm64 is not None
    new_lab = (lab * 5 + np.arange(N)) % (C + 3)
    got = base.relabel(new_lab, C + 3, inplace=True)
    want = _index(x, new_lab, ids, 1024, C + 3)
    _same(got, want)
    assert got.inv_norm64 is not None and torch.equal(got.inv_norm64, want.inv_norm64)
    assert int((got.inv_norm64 != got.inv_norm).sum()) == 3


def test_relabel_inplace_allocates_no_second_corpus():
    """The rise of the allocator's peak over the in-place call stays below half
    the corpus (partners, workspace and tables: about 0.4 MB against 6.3 MB);
    over the copying call it is at least the corpus."""
    import workloads
    n = 4096
    w = workloads.clustered(n=n, d=768, nq=1, C=C, seed=3, label_mode="skewed")
    x, lab = w["x"], w["labels"]
    new_lab = np.random.Generator(np.random.PCG64(9)).integers(0, C, n)
    dev_lab = torch.from_numpy(new_lab).to(DEV)
    index = _index(x, lab, None, 1024)
    corpus_bytes = n * 768 * 2
    torch.cuda.synchronize()

    def rise(fn):
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = fn()
        return out, torch.cuda.max_memory_allocated(DEV) - base

    copied, up_copy = rise(lambda: index.relabel(dev_lab))
    assert up_copy >= corpus_bytes, up_copy
    del copied
    new, up_inplace = rise(lambda: index.relabel(dev_lab, inplace=True))
    assert up_inplace < corpus_bytes // 2, up_inplace
    _same(new, _index(x, new_lab, None, 1024))


def test_objects_consumed_by_a_relabel_refuse_before_any_launch():
    from li.index import DeviceRouter, Searcher
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + EXTRA + 1, dtype=np.int64)
    old = _index(x[:N], lab[:N], ids[:N], 1024, capacity=N + EXTRA)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    new_lab = np.roll(lab[:N], 1)
    new = old.relabel(new_lab, inplace=True)
    assert old.consumed and not new.consumed
    for call in (lambda: s.search(qn, q, 3, k=10, use_threshold=True),
                 lambda: s.lists(qn, q, 3, 10),
                 lambda: old.add(x[N:N + 1], lab[N:N + 1], [N + 1]),
                 lambda: old.add(x[N:N + 1], lab[N:N + 1], [N + 1], inplace=True),
                 lambda: old.remove(ids[:1]),
                 lambda: old.remove(ids[:1], inplace=True),
                 lambda: old.relabel(lab[:N]),
                 lambda: old.relabel(lab[:N], inplace=True),
                 lambda: old.reserve(N + EXTRA),
                 lambda: old.desc,
                 lambda: old.workspace(64, 3, 10, _lib.LMI_Q_F16)):
        with pytest.raises(RuntimeError, match="in place"):
            call()
    got = s.with_index(new).search(qn, q, 3, k=10, use_threshold=True)
    want = Searcher(_index(x[:N], new_lab, ids[:N], 1024), s.router).search(qn, q, 3, k=10,
                                                                           use_threshold=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_relabel_inplace_refusals_leave_the_index_in_use(monkeypatch):
    import workloads
    from li.index import DeviceIndex, DeviceRouter, Searcher
    w = _w(100, "skewed")
    x, lab = w["x"], w["labels"]
    ids = np.arange(1, N + 1, dtype=np.int64)
    old = _index(x[:N], lab[:N], ids, 1024)
    s = Searcher(old, DeviceRouter(w["layers"], device=DEV))
    qn, q = torch.from_numpy(w["qn"]).to(DEV), torch.from_numpy(w["q"]).to(DEV)
    before = s.search(qn, q, 3, k=10, use_threshold=True)
    dev0, host0 = _arrays(old)
    order0 = old.layout.order.copy()
    ptrs = {k: getattr(old, k).data_ptr() for k in ARRAYS}

    def unchanged():
        assert not old.consumed and old.n_rows == N and old.capacity == N
        for k in ARRAYS:
            assert getattr(old, k).data_ptr() == ptrs[k] and torch.equal(getattr(old, k), dev0[k]), k
        for k in HOST:
            assert np.array_equal(getattr(old, k), host0[k]), k
        after = s.search(qn, q, 3, k=10, use_threshold=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

    for wrong in (lab[:N - 1], lab[:N + 1], torch.from_numpy(lab[:N + 1]).to(DEV)):   # a wrong label count
        with pytest.raises(ValueError, match="one entry per row"):
            old.relabel(wrong, inplace=True)
    unchanged()
    for bad in (-1, C):                                                    # a label out of range
        labels = lab[:N].copy()
        labels[1234] = bad
        for given in (labels, torch.from_numpy(labels.astype(np.int32)).to(DEV)):
            with pytest.raises(ValueError, match="labels must lie in"):
                old.relabel(given, inplace=True)
    big = lab[:N].copy()
    big[5] = _lib.LMI_REBUCKET_MAX_BUCKETS + 1
    with pytest.raises(ValueError, match="labels must lie in"):            # the fallback sort's check
        old.relabel(big, _lib.LMI_REBUCKET_MAX_BUCKETS + 1, inplace=True)
    unchanged()
    for nb in (0, -3):
        with pytest.raises(ValueError):
            old.relabel(lab[:N], nb, inplace=True)
    unchanged()
    # a plan whose status is not clean: a new order that names a row twice
    # gives a src_pos that is no permutation
    real = DeviceIndex._sorted_by_bucket

    def twice(labels, n_buckets):
        order, off = real(labels, n_buckets)
        order[10] = order[11]
        return order, off

    monkeypatch.setattr(DeviceIndex, "_sorted_by_bucket", staticmethod(twice))
    with pytest.raises(RuntimeError, match="unchanged"):
        old.relabel(np.roll(lab[:N], 1), inplace=True)
    monkeypatch.undo()
    assert np.array_equal(old.layout.order, order0)
    unchanged()
    for kw, word in ((dict(storage="f32"), "storage"), (dict(rank=0, world=2), "striped"),
                     (dict(subcluster=True), "sub-cluster")):
        other = _index(x[:N], lab[:N], ids, 64, **kw)
        with pytest.raises(ValueError, match=word):
            other.relabel(lab[:other.n_total], inplace=True)
        assert not other.consumed
    x64, _ = workloads.float64_inputs(w, 3)
    other = _index(x64[:N], lab[:N], ids, 64)
    assert other.corpus64 is not None
    with pytest.raises(ValueError, match="corpus64"):
        other.relabel(lab[:N], inplace=True)
    assert not other.consumed
    # ... and the index still takes the relabel
    new_lab = np.roll(lab[:N], 1)
    _same(old.relabel(new_lab, inplace=True), _index(x[:N], new_lab, ids, 1024))
    assert old.consumed


@pytest.mark.parametrize("R,how", [(1, "search"), (3, "search"), (3, "f64"), (3, "streamed")])
def test_searches_over_the_inplace_relabelled_index_equal_the_rebuilt_one(R, how):
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
    ptr0 = s_old.index.corpus.data_ptr()
    relabelled = s_old.index.relabel(lab2, inplace=True)
    s_new = s_old.with_index(relabelled)
    assert s_new.router is router2 and s_new.index is relabelled and s_old.index.consumed
    assert relabelled.corpus.data_ptr() == ptr0
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
        classes = O.rank_classes(O.mlp_forward(w["qn"], layers2))
        ref_d, ref_a = O.search_via_lists(lab2, ids, x, w["q"], classes, C, R, k=10, use_threshold=True)
        assert O.compare_lists(ref_d, ref_a, got[0], got[1]) == 0


def test_learned_index_rebucket_in_place():
    from li.LearnedIndex import LearnedIndex
    w = _w(768, "router")
    x, xn, lab = w["x"], w["xn"], w["labels"]
    model = _nn(w["layers"], "MLP", C)
    model2 = _nn(_router2()[0], "MLP", C)
    out = {}
    for inplace in (False, True):
        li_ = LearnedIndex()
        li_.model = model
        nav, ds = _frames(xn[:N], x[:N], 1)
        labels = lab[:N].copy()
        index0 = li_.attach(nav, ds, labels)
        ptr0 = index0.corpus.data_ptr()
        li_.model = model2                                # the retrained router
        nav2, ds2, labels2 = (li_.rebucket(nav, ds, labels, inplace=True) if inplace
                              else li_.rebucket(nav, ds, labels))        # (the default: a copy)
        assert index0.consumed == inplace and li_._index is not index0
        assert (li_._index.corpus.data_ptr() == ptr0) == inplace
        assert ds2 is ds and not np.array_equal(labels2, labels)
        got = li_.search(nav2, w["qn"], ds2, w["q"], labels2, n_buckets=3, k=10, use_threshold=True)
        out[inplace] = (nav2, labels2, got)
    a, b = out[False], out[True]
    assert a[0].equals(b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])
