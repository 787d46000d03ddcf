"""What DeviceIndex.add / remove (K7, K9: csrc/lmi_update.hip) and relabel (K8, K10: csrc/lmi_rebucket.hip)
run on the device: plain functions over an index; li.index calls in here and is not imported.
Every path ends in index._successor(...), whose rows are in a fresh store or stay in the old one."""
from __future__ import annotations

import contextlib
import os
import time

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .layout import BucketLayout

# In-place updates (K9): rows of a staged slab, the least rows of
# a direct slab, and the cap on the staging buffer (the Infinity Cache's size)
DEFAULT_SLAB_ROWS = 64 << 10
DEFAULT_DIRECT_ROWS = 16 << 10
STAGING_MAX_BYTES = 256 << 20
_UNCHANGED = " (the index is unchanged)"


class _Timings:
    """A call's `timings` dict; None: every method is a no-op (no event, no wait)."""

    def __init__(self, out, dev):
        self.out, self.dev, self.ev, self.t = out, dev, {}, time.perf_counter()

    def lap(self, name):   # out[name] += the wall-clock seconds since the last lap, the device idle
        if self.out is not None:
            torch.cuda.synchronize(self.dev)
            t = time.perf_counter()
            self.out[name], self.t = self.out.get(name, 0.0) + t - self.t, t

    def event(self, name):   # a device event on the current stream; ms(a, b): between two of them
        if self.out is not None:
            self.ev[name] = torch.cuda.Event(enable_timing=True)
            self.ev[name].record()

    def ms(self, a, b) -> float:
        return self.ev[a].elapsed_time(self.ev[b])

    def put(self, fn):   # out.update(fn()): figures that cost something to work out
        if self.out is not None:
            self.out.update(fn())


def _ingest(index, x, dst, out, out_inv, n_out: int, status):
    """Launch lmi_index_ingest_rows: x (fp16 / fp32 rows) into out[dst], out_inv[dst]."""
    check("lmi_index_ingest_rows", _lib.load().lmi_index_ingest_rows(
        ptr(x), _lib.LMI_F16 if x.dtype == torch.float16 else _lib.LMI_F32, int(x.shape[0]), x.stride(0),
        index.d, index.d_pad, ptr(dst), ptr(out), ptr(out_inv), n_out, ptr(status),
        _lib.stream_handle(index.device)))


def _ingest_status(st: int, unchanged: bool = False) -> bool:
    """Judge an update's status word, the index in use; True: a low-norm row came."""
    if st & _lib.LMI_STATUS_ROWS_NOT_F16:
        raise ValueError("index update: float32 rows must be fp16-representable (storage 'f16')")
    if st & ~_lib.LMI_STATUS_ROWS_LOW_NORM:
        raise RuntimeError(f"index update: internal status {st}" + (_UNCHANGED if unchanged else ""))
    return bool(st & _lib.LMI_STATUS_ROWS_LOW_NORM)


@contextlib.contextmanager
def _consuming(index, status, tm, what: str, ok_bits: int = 0):
    """Move rows inside `index`'s own store.  On entry the whole device is waited for (replays on other
    streams read this index); the body calls the yielded launched(fn, rc) with the first mover's code;
    on exit the status word is read once and the device waited for again.  The caller hands the store over."""

    def launched(fn, rc):
        if rc == _lib.LMI_E_INVALID:
            check(fn, rc)  # (refused on the host: nothing was launched)
        index._consume()   # from here on rows may have moved: this object must not launch again
        check(fn, rc)
        tm.event("move1")
    torch.cuda.synchronize(index.device)
    tm.event("move0")
    yield launched
    st = int(status.item())  # (waits for the chain: its buffers stay alive until here)
    torch.cuda.synchronize(index.device)
    if st & ~ok_bits:
        raise RuntimeError(f"{what}: internal status {st}; the index is consumed "
                           "and the content of its store is undefined")


def _batch_rows(index, rows) -> torch.Tensor:
    """The batch on the device as lmi_index_ingest_rows reads it: fp16 or
    fp32 with contiguous rows (a device tensor of that form as it is)."""
    if not isinstance(rows, torch.Tensor):
        a = np.asarray(rows)
        a = a if a.dtype in (np.float16, np.float32, np.float64) else a.astype(np.float32)
        rows = torch.from_numpy(np.ascontiguousarray(a))
    if rows.dtype == torch.float64:
        f = rows.float()
        if not torch.equal(f.double(), rows):
            raise ValueError("index update: float64 rows must be fp16-representable")
        rows = f
    elif rows.dtype not in (torch.float16, torch.float32):
        rows = rows.float()
    rows = rows.to(index.device)
    return rows if rows.stride(1) == 1 and rows.stride(0) >= rows.shape[1] else rows.contiguous()


@torch.no_grad()
def update(index, drop, rows, lab, ids, new_tags, *, inplace, slab_rows, direct_rows, timings):
    """The index after dropping the positions `drop` (ascending) and appending the batch.  What both
    ways share: the host tables by index arithmetic, their successor, the kernels' tables on the device."""
    dev, m, r = index.device, int(lab.size), int(drop.size)
    if inplace and index.n_rows - r + m > index.capacity:
        raise ValueError(f"index update in place: {index.n_rows - r + m} rows exceed the capacity of "
                         f"{index.capacity} rows (build the index with `capacity`, or `reserve`)")
    layout, new_dst, surv_off, drop_before = index.layout.updated(drop, lab)
    p2id = BucketLayout.updated_table(index.pos_to_id, drop, surv_off, layout.bucket_off, new_dst, ids)
    tags = None if index.tags_by_pos is None else BucketLayout.updated_table(
        index.tags_by_pos, drop, surv_off, layout.bucket_off, new_dst, new_tags)
    new = index._successor(layout, p2id, tags)
    d_drop = torch.from_numpy(drop.astype(np.int64)).to(dev) if r else None
    d_before = torch.from_numpy(drop_before).to(dev) if r else None
    d_dst = torch.from_numpy(new_dst).to(dev) if m else None
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    # lmi_index_move_rows[_inplace]'s arguments from the new offsets to the drop table
    tables = (ptr(new.bucket_off_local), index.n_buckets, ptr(d_drop), r, ptr(d_before))
    tm = _Timings(timings, dev)
    if inplace:
        _update_inplace(index, new, rows, drop, tables, d_dst, status, slab_rows, direct_rows, tm)
    else:
        _update_copy(index, new, rows, tables, d_dst, status, tm)
    return new


def _update_copy(index, new, rows, tables, d_dst, status, tm):
    """The rows of `new` by the K7 kernels, in a new store of max(capacity, n_new) rows."""
    survivors = index.n_rows - tables[3]   # (the old rows less the dropped ones)
    new._alloc_store(new.n_rows, capacity=index.capacity)
    tm.event("move0")
    if survivors > 0:
        check("lmi_index_move_rows", _lib.load().lmi_index_move_rows(
            ptr(index.corpus), ptr(index.inv_norm), index.n_rows, index.d_pad, ptr(index.bucket_off_local),
            *tables, ptr(new.corpus), ptr(new.inv_norm), new.n_rows, ptr(status),
            _lib.stream_handle(index.device)))
    tm.event("move1")
    if d_dst is not None:
        x = _batch_rows(index, rows)
        _ingest(index, x, d_dst, new.corpus, new.inv_norm, new.n_rows, status)
    low = _ingest_status(int(status.item()))  # (waits for both kernels: their inputs stay alive until here)
    # an inv_norm64 only when this index has one or the batch brings such a
    # row: an update of an index without them launches and reads nothing more
    if low or index.inv_norm64 is not None:
        new._set_inv_norm64()
    tm.put(lambda: dict(move_ms=tm.ms("move0", "move1"), moved_rows=survivors))


def _update_inplace(index, new, rows, drop, tables, d_dst, status, slab_rows, direct_rows, tm):
    """The rows of `new` by the K9 chain inside the index's own store."""
    dev, d_pad = index.device, index.d_pad
    tmp, inv64 = None, index.inv_norm64 is not None   # (an inv_norm64: as in _update_copy)
    if d_dst is not None:
        # the batch first, into a temporary [m, d_pad] buffer: its status
        # word is read before any row of the store moves
        m = new.n_rows - index.n_rows + tables[3]
        tmp = torch.empty((m, d_pad), dtype=torch.float16, device=dev)
        tmp_inv = torch.empty((m,), dtype=torch.float32, device=dev)
        x, seq = _batch_rows(index, rows), torch.arange(m, dtype=torch.int64, device=dev)
        _ingest(index, x, seq, tmp, tmp_inv, m, status)
        inv64 |= _ingest_status(int(status.item()), unchanged=True)
        del x, tmp_inv, seq
    if slab_rows is None:
        slab_rows = max(1, min(DEFAULT_SLAB_ROWS, STAGING_MAX_BYTES // (2 * d_pad + 4)))
    if direct_rows is None:
        direct_rows = DEFAULT_DIRECT_ROWS
    slabs = np.ascontiguousarray(index.layout.inplace_slabs(new.layout.bucket_off, drop, slab_rows, direct_rows))
    staged = slabs[slabs[:, 2] == 1]
    stage_rows = int((staged[:, 1] - staged[:, 0]).max()) if staged.size else 0
    stage = stage_inv = None
    if stage_rows:
        stage = torch.empty((stage_rows, d_pad), dtype=torch.float16, device=dev)
        stage_inv = torch.empty((stage_rows,), dtype=torch.float32, device=dev)
    store, store_inv, old_off = index._store, index._store_inv, index.bucket_off_local   # (dropped when consumed)
    with _consuming(index, status, tm, "index update in place", _lib.LMI_STATUS_ROWS_LOW_NORM) as launched:
        launched("lmi_index_move_rows_inplace", _lib.load().lmi_index_move_rows_inplace(
            ptr(store), ptr(store_inv), index.n_rows, new.n_rows, index.capacity, d_pad, ptr(old_off), *tables,
            _lib.LMI_INPLACE_REMOVE if drop.size else _lib.LMI_INPLACE_ADD, slabs.ctypes.data,
            int(slabs.shape[0]), ptr(stage), ptr(stage_inv), stage_rows,
            _lib.LMI_INPLACE_MEMCPY if os.environ.get("LMI_INPLACE_MEMCPY") == "1" else 0,
            ptr(status), _lib.stream_handle(dev)))
        if tmp is not None:
            # the batch, from the temporary to its places behind the moved rows
            _ingest(index, tmp, d_dst, store, store_inv, new.n_rows, status)
    new._adopt_store(store, store_inv, new.n_rows, inv64)
    tm.put(lambda: dict(move_ms=tm.ms("move0", "move1"),
                        direct_slabs=int((slabs[:, 2] == 0).sum()), staged_slabs=int((slabs[:, 2] == 1).sum()),
                        moved_rows=int((slabs[:, 1] - slabs[:, 0]).sum()),
                        staged_rows=int((staged[:, 1] - staged[:, 0]).sum()), staging_rows=stage_rows))


class UnknownIds(KeyError, ValueError):
    """edit_tags' report of ids the index does not hold: remove's KeyError, and a ValueError like
    the call's other refusals."""


def _edit_words(words, n: int, name: str) -> np.ndarray:
    """`words` (an int or [n] integers in [0, 2^32)) as uint32 [n]; ValueError otherwise."""
    w = words.cpu().numpy() if isinstance(words, torch.Tensor) else np.asarray(words)
    if w.dtype.kind not in "iu" or isinstance(words, bool) or w.shape not in ((), (n,)):
        raise ValueError(f"{name} must be an integer or [{n}] integers, one per id")
    if w.size and (int(w.min()) < 0 or int(w.max()) >= 1 << 32):
        raise ValueError(f"{name} must lie in [0, 2^32)")
    return np.array(np.broadcast_to(w.astype(np.uint32), (n,)))   # (a copy: broadcast views are read-only)


@torch.no_grad()
def edit_tags(index, ids, set_bits, clear_bits) -> None:
    """DeviceIndex.edit_tags: the host table and the device words of `index` itself, one launch of
    lmi_index_edit_tags in stream order; every refusal before it."""
    index._check_live()
    if index.tags_by_pos is None:
        raise ValueError("edit_tags: this index is untagged (build it with `tags`)")
    if index.world > 1:
        raise ValueError("edit_tags: a striped index (world > 1) takes no tag edits: every rank holds the "
                         "whole host table and its own rows' words")
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if ids.size and ids.dtype.kind not in "iu":
        raise ValueError("edit_tags: ids must be integers")
    ids = ids.astype(np.int64, copy=False).ravel()
    n = int(ids.size)
    st, cl = _edit_words(set_bits, n, "set_bits"), _edit_words(clear_bits, n, "clear_bits")
    uniq = np.unique(ids)
    if uniq.size != n:
        raise ValueError("edit_tags: duplicate ids")
    # positions of the ids (one row each: ids are unique in an index), in the caller's order: a sorted
    # search of pos_to_id, whose order is worked out on the first edit of an index and kept (the table
    # never changes in an index's life; a repeated edit, as deletes by tombstone are, then costs log n an id)
    by_id = index.__dict__.get("_by_id")
    if by_id is None:
        by_id = index._by_id = np.argsort(index.pos_to_id, kind="stable")
    at = np.searchsorted(index.pos_to_id, ids, sorter=by_id)
    pos = by_id[np.minimum(at, by_id.size - 1)] if by_id.size else np.zeros(n, np.int64)
    found = (index.pos_to_id[pos] == ids) if by_id.size else np.zeros(n, bool)
    if not found.all():
        missing = np.unique(ids[~found])
        raise UnknownIds(f"ids not in the index: {missing[:8].tolist()}" + (" ..." if missing.size > 8 else ""))
    if n == 0:
        return
    dev = index.device
    # (world == 1: a row's position is its row of the device arrays, gpos = 0 .. n_rows - 1)
    d_rows = torch.from_numpy(pos.astype(np.int64)).to(dev)
    d_clear, d_set = (torch.from_numpy(w.view(np.int32)).to(dev) for w in (cl, st))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    check("lmi_index_edit_tags", _lib.load().lmi_index_edit_tags(
        ptr(index.tags), index.n_rows, ptr(d_rows), ptr(d_clear), ptr(d_set), n, ptr(status),
        _lib.stream_handle(dev)))
    index.tags_by_pos = index.tags_by_pos.copy()   # (a successor or a caller may share the old table)
    index.tags_by_pos[pos] = (index.tags_by_pos[pos] & ~cl) | st
    index.tags_version += 1
    if int(status.item()):   # (waits for the kernel: its inputs stay alive until here)
        raise RuntimeError(f"edit_tags: internal status {int(status.item())}")


def sorted_by_bucket(lab: torch.Tensor, n_buckets: int):
    """(order, bucket_off) of the device labels `lab` (int32 / int64), both
    int64 on the device: BucketLayout.from_labels' tables.  Up to
    LMI_REBUCKET_MAX_BUCKETS buckets by lmi_bucket_sort_labels; above, by
    torch.sort(stable=True) on the device."""
    dev, n = lab.device, int(lab.numel())
    if n_buckets > _lib.LMI_REBUCKET_MAX_BUCKETS:
        if n and (int(lab.min()) < 0 or int(lab.max()) >= n_buckets):
            raise ValueError(f"labels must lie in [0, {n_buckets})")
        order = torch.sort(lab, stable=True).indices
        off = torch.zeros(n_buckets + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(lab, minlength=n_buckets), 0, out=off[1:])
        return order, off
    lib = _lib.load()
    order = torch.empty(n, dtype=torch.int64, device=dev)
    off = torch.empty(n_buckets + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.lmi_bucket_sort_labels_ws_bytes(n, n_buckets)
    ws = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=dev)
    check("lmi_bucket_sort_labels", lib.lmi_bucket_sort_labels(
        ptr(lab), lab.element_size(), n, n_buckets, ptr(off), ptr(order), ptr(status), ptr(ws),
        ws.numel() * 8, _lib.stream_handle(dev)))
    st = int(status.item())  # (before `order` indexes anything: a bad label leaves holes in it)
    if st & _lib.LMI_STATUS_BAD_LABEL:
        raise ValueError(f"labels must lie in [0, {n_buckets})")
    if st:
        raise RuntimeError(f"index relabel: internal status {st}")
    return order, off


def relabel(index, lab: torch.Tensor, n_buckets: int, inplace: bool, timings):
    """The index over the same row sequence with the device labels `lab` (one
    per row) and `n_buckets` buckets; under torch.no_grad() (DeviceIndex.relabel)."""
    dev, n = index.device, index.n_rows
    tm = _Timings(timings, dev)
    order, off = index._sorted_by_bucket(lab, n_buckets)
    tm.lap("sort")
    # src_pos[p]: where the old index holds the row of new position p (the
    # inverse of the old order, read at the new one); pos_to_id moves as the rows do
    old_order = torch.from_numpy(index.layout.order).to(dev)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    inv[old_order] = torch.arange(n, dtype=torch.int64, device=dev)
    src_pos = inv[order]
    del inv, old_order
    p2id = torch.from_numpy(index.pos_to_id).to(dev)[src_pos]
    tm.lap("tables")
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    inv64 = index.inv_norm64 is not None
    if inplace:
        store, store_inv = _swap_inplace(index, src_pos, status, tm)   # (consumes the index)
    else:   # (into a store of the old capacity: a reserved index stays reserved)
        store = torch.empty((index.capacity, index.d_pad), dtype=torch.float16, device=dev)
        store_inv = torch.empty((index.capacity,), dtype=torch.float32, device=dev)
        check("lmi_index_gather_rows", _lib.load().lmi_index_gather_rows(
            ptr(index.corpus), ptr(index.inv_norm), n, index.d_pad, ptr(src_pos), ptr(store),
            ptr(store_inv), n, ptr(status), _lib.stream_handle(dev)))
        st = int(status.item())  # (waits for the kernel: src_pos stays alive until here)
        if st:
            raise RuntimeError(f"index relabel: internal status {st}")
        tm.lap("gather")
    # the new tables come down; the tags move as pos_to_id does (on the host, then uploaded)
    layout = BucketLayout(n_buckets, order.cpu().numpy(), off.cpu().numpy())
    tags = index.tags_by_pos
    if tags is not None:
        tags = tags[BucketLayout.relabel_source(index.layout.order, layout.order)]
    new = index._successor(layout, p2id.cpu().numpy(), tags)
    new._adopt_store(store, store_inv, n, inv64)
    tm.lap("host")
    return new


def _swap_inplace(index, src_pos, status, tm):
    """relabel(inplace=True)'s row move (K10): plan the gather by `src_pos` as
    two involutions, read the plan's status, then swap the rows in two passes.  Returns the store."""
    lib = _lib.load()
    dev, n, s = index.device, index.n_rows, _lib.stream_handle(index.device)
    p1 = torch.empty(n, dtype=torch.int64, device=dev)
    p2 = torch.empty(n, dtype=torch.int64, device=dev)
    need = lib.lmi_perm_involutions_ws_bytes(n)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    tm.event("plan0")
    check("lmi_perm_involutions", lib.lmi_perm_involutions(
        ptr(src_pos), n, ptr(p1), ptr(p2), ptr(status), ptr(ws), need, s))
    tm.event("plan1")
    st = int(status.item())  # (the plan is judged before any row moves)
    del ws
    if st & _lib.LMI_STATUS_BAD_PERM:
        raise RuntimeError("index relabel in place: the row order of the index and the new one "
                           "do not give a permutation of its rows" + _UNCHANGED)
    if st:
        raise RuntimeError(f"index relabel in place: internal status {st}" + _UNCHANGED)
    tm.put(lambda: dict(swapped_rows=[
        2 * int((p > torch.arange(n, dtype=torch.int64, device=dev)).sum()) for p in (p1, p2)]))
    tm.lap("plan")
    store, store_inv = index._store, index._store_inv

    def swap(partner):   # (an empty index: returns at once, as the plan did; nothing is launched)
        return lib.lmi_index_swap_rows(ptr(store), ptr(store_inv), n, index.d_pad, ptr(partner), ptr(status), s)
    with _consuming(index, status, tm, "index relabel in place") as launched:
        launched("lmi_index_swap_rows", swap(p1))
        check("lmi_index_swap_rows", swap(p2))
        tm.event("move2")
    tm.put(lambda: dict(plan_ms=tm.ms("plan0", "plan1"), plan_rounds=2 * max(0, (n - 1).bit_length()),
                        swap_ms=[tm.ms("move0", "move1"), tm.ms("move1", "move2")]))
    tm.lap("swap")
    return store, store_inv
