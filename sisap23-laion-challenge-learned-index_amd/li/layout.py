"""Bucket layout of the corpus and its per-row tag words: host index arithmetic on numpy alone, shared by
every rank (tags given as a tensor come to the host through its `.cpu()`).  li.index re-exports every name."""
from __future__ import annotations

import bisect
import dataclasses
from typing import Optional

import numpy as np

DEFAULT_CHUNK_ROWS = 8192


def default_chunk_rows(world: int, n_rows: Optional[int] = None) -> int:
    """The scan's chunk (rows) for a shard of a `world`-rank index: 8192 on one
    GPU, 4096 on 2-4, 2048 on more, so a 1/world stripe still cuts into enough
    tiles to fill 256 CUs (DESIGN.md §5 "Chunk size"; tools/gpu_shards.sh);
    given the index's rows, halved (down to 1024) while a rank's shard would
    hold fewer than 64 chunks (configs[1], 300K rows: 4096 -- the scan 0.63
    instead of 0.75 ms, the float64 line +8%, the stream as fast; smaller
    chunks speed the scan further but add plan and merge work to a launch
    the host already bounds, profiles/r05aa_300K_chunk_rows.txt)."""
    c = DEFAULT_CHUNK_ROWS if world <= 1 else 4096 if world <= 4 else 2048
    if n_rows is not None:
        per = n_rows / max(int(world), 1)
        while c > 1024 and per / c < 64:
            c //= 2
    return c


@dataclasses.dataclass
class BucketLayout:
    """Bucket-sorted order of the corpus.  Global position p holds row order[p]."""

    n_buckets: int
    order: np.ndarray        # int64 [n]: row index of each global position
    bucket_off: np.ndarray   # int64 [C+1] global offsets

    @classmethod
    def from_labels(cls, labels, n_buckets: int) -> "BucketLayout":
        lab = np.asarray(labels).astype(np.int64, copy=False).ravel()
        if lab.size and (lab.min() < 0 or lab.max() >= n_buckets):
            raise ValueError(f"labels must lie in [0, {n_buckets})")
        order = np.argsort(lab, kind="stable").astype(np.int64)
        size = np.bincount(lab, minlength=n_buckets).astype(np.int64)
        off = np.zeros(n_buckets + 1, np.int64)
        np.cumsum(size, out=off[1:])
        return cls(n_buckets, order, off)

    @property
    def bucket_size(self) -> np.ndarray:
        return np.diff(self.bucket_off)

    def updated(self, drop_positions, new_labels):
        """The layout after an update of the row sequence: the rows at the
        global positions `drop_positions` are deleted from it and one row per
        entry of `new_labels` is appended, in that order.  Returns

            (layout, new_dst, surv_off, drop_before)

        layout      equals from_labels over the updated label sequence (row
                    indices renumbered: survivors keep their relative order,
                    the new rows follow)
        new_dst     int64 [m]: the global position of every new row -- behind
                    its bucket's survivors, stable in batch order
        surv_off    int64 [C+1]: prefix sums of the survivors per bucket; with
                    the new offsets it places any per-position table of
                    the survivors (place_survivors)
        drop_before int64 [C+1]: how many dropped positions lie before each
                    old bucket offset (lmi_index_move_rows' table)

        Pure numpy, O(n + m) index arithmetic (slice copies per bucket) and
        one stable sort of the m new labels; no sort over n."""
        C_, off = self.n_buckets, self.bucket_off
        n = int(off[-1])
        drop = np.unique(np.asarray(drop_positions, dtype=np.int64).ravel())
        if drop.size != np.asarray(drop_positions).size:
            raise ValueError("drop_positions must be distinct")
        if drop.size and (drop[0] < 0 or drop[-1] >= n):
            raise ValueError(f"drop_positions must lie in [0, {n})")
        lab = np.asarray(new_labels).astype(np.int64, copy=False).ravel()
        if lab.size and (lab.min() < 0 or lab.max() >= C_):
            raise ValueError(f"labels must lie in [0, {C_})")
        m = int(lab.size)
        drop_before = np.searchsorted(drop, off, side="left").astype(np.int64)
        surv = np.diff(off) - np.diff(drop_before)
        added = np.bincount(lab, minlength=C_).astype(np.int64)
        new_off = np.zeros(C_ + 1, np.int64)
        np.cumsum(surv + added, out=new_off[1:])
        # survivors, in ascending old position (bucket by bucket): bucket c's
        # start at new_off[c]
        n_surv = n - int(drop.size)
        surv_off = np.zeros(C_ + 1, np.int64)
        np.cumsum(surv, out=surv_off[1:])
        # new rows: stable rank inside the bucket, after its survivors
        by_label = np.argsort(lab, kind="stable")
        add_off = np.zeros(C_ + 1, np.int64)
        np.cumsum(added, out=add_off[1:])
        new_dst = np.empty(m, np.int64)
        new_dst[by_label] = np.arange(m, dtype=np.int64) + np.repeat(
            new_off[:-1] + surv - add_off[:-1], added)
        # row indices of the updated sequence: the kept rows renumbered in
        # their order, then the batch
        kept = self.order
        if drop.size:
            keep_row = np.ones(n, bool)
            keep_row[self.order[drop]] = False
            renum = np.cumsum(keep_row) - 1
            kept = renum[np.delete(self.order, drop)]
        order = np.empty(n_surv + m, np.int64)
        self.place_survivors(kept, surv_off, new_off, order)
        order[new_dst] = n_surv + np.arange(m, dtype=np.int64)
        return BucketLayout(C_, order, new_off), new_dst, surv_off, drop_before

    def inplace_slabs(self, new_off, drop, slab_rows: int, direct_rows: int) -> np.ndarray:
        """The plan of an update inside one buffer (lmi_index_move_rows_inplace):
        int64 [k, 3] rows (a, b, staged) -- slabs [a, b) of this layout's
        positions, in processing order.  `new_off`: the bucket offsets after
        the update (updated()'s layout.bucket_off); `drop`: the ascending
        dropped positions.  No drops: an add, every row moves right by its
        bucket's new_off - bucket_off, which does not decrease along the
        corpus; drops: a remove (no new rows), every survivor moves left by the
        number of drops before it.

        Rows that do not move are in no slab: an add's prefix up to and
        including the first bucket that receives a row, a remove's prefix
        before the first drop.  An add is cut from the end backwards, a remove
        from the front forwards.  At the cursor the longest DIRECT slab is
        taken -- its destinations lie outside [a, b): a + shift(a) >= b for an
        add, dest(b - 1) < a for a remove -- when it has at least
        `direct_rows` rows; otherwise a STAGED slab of at most `slab_rows`
        rows.  Destinations of a slab then lie in its own range or in rows
        earlier slabs have vacated, never in rows a later slab reads.
        O(slabs * log) host arithmetic, no array over n."""
        slab_rows, direct_rows = int(slab_rows), int(direct_rows)
        if slab_rows < 1 or direct_rows < 1:
            raise ValueError("slab_rows and direct_rows must be positive")
        off = self.bucket_off
        n = int(off[-1])
        new_off = np.asarray(new_off, dtype=np.int64)
        drop = np.asarray(drop, dtype=np.int64).ravel()
        if new_off.shape != off.shape:
            raise ValueError("new_off must have one entry per bucket offset")
        out = []
        if drop.size == 0:
            shift = new_off[:-1] - off[:-1]
            if (shift < 0).any() or (np.diff(shift) < 0).any():
                raise ValueError("inplace_slabs: new_off is not this layout plus added rows")
            moved = np.flatnonzero(shift > 0)
            if n == 0 or moved.size == 0:
                return np.zeros((0, 3), np.int64)
            first = int(off[moved[0]])           # rows before it keep their place
            # hi[c]: where the last row of bucket c lands (non-decreasing in c)
            hi, lo, sh = (off[1:] - 1 + shift).tolist(), off[:-1].tolist(), shift.tolist()
            e = n
            while e > first:
                c = bisect.bisect_left(hi, e)    # the first bucket with a row landing at or past e
                a = max(lo[c], e - sh[c], first)
                staged = e - a < direct_rows
                if staged:
                    a = max(first, e - slab_rows)
                out.append((a, e, int(staged)))
                e = a
            return np.array(out, np.int64).reshape(-1, 3)
        r = int(drop.size)
        if (np.diff(drop) <= 0).any() or drop[0] < 0 or drop[-1] >= n:
            raise ValueError(f"inplace_slabs: drop must be ascending, distinct and inside [0, {n})")
        if int(new_off[-1]) != n - r:
            raise ValueError("inplace_slabs: a remove in place takes no new rows")
        n_surv = n - r
        d = drop.tolist()
        key = (drop - np.arange(r, dtype=np.int64)).tolist()   # survivors before each drop

        def survivor(t):                         # position of the survivor of rank t
            return t + bisect.bisect_right(key, t)

        def next_survivor(s):                    # the first survivor at or after s (n: none)
            t = s - bisect.bisect_left(d, s)
            return survivor(t) if t < n_surv else n

        s = next_survivor(d[0])
        while s < n:
            # (dest(i) = survivors before i: the last row with dest < s is the
            # survivor of rank s - 1, at or after s as a drop lies before s)
            b = survivor(s - 1) + 1 if s - 1 < n_surv else n
            staged = b - s < direct_rows
            if staged:
                b = min(n, s + slab_rows)
            out.append((s, b, int(staged)))
            s = next_survivor(b)
        return np.array(out, np.int64).reshape(-1, 3)

    @staticmethod
    def place_survivors(kept, surv_off, new_off, out) -> None:
        """out[new_off[c] + j] = kept[surv_off[c] + j], j < surv_off[c+1] -
        surv_off[c], for every bucket c: a per-position table of the survivors
        (`kept`, in ascending old position) laid out at the front of every
        bucket's new range.  One slice copy per bucket (memcpy speed; an index
        array over n is several times slower), an index array when there are
        more buckets than that pays for."""
        C_ = int(surv_off.size) - 1
        if C_ <= 1 << 14:
            for c in range(C_):
                a, b = int(surv_off[c]), int(surv_off[c + 1])
                if b > a:
                    t = int(new_off[c])
                    out[t:t + (b - a)] = kept[a:b]
            return
        shift = np.repeat(new_off[:-1] - surv_off[:-1], np.diff(surv_off))
        out[np.arange(kept.size, dtype=np.int64) + shift] = kept

    @staticmethod
    def updated_table(table, drop, surv_off, new_off, new_dst, new_values) -> np.ndarray:
        """A per-position table (pos_to_id, tags_by_pos) after updated(): the
        survivors' entries at the front of every bucket's new range, the new
        rows' `new_values` at `new_dst`.  `drop`: the ascending dropped
        positions; the other arguments as updated() returns them."""
        table = np.asarray(table)
        out = np.empty(int(new_off[-1]), table.dtype)
        BucketLayout.place_survivors(np.delete(table, drop) if len(drop) else table, surv_off, new_off, out)
        out[new_dst] = new_values
        return out

    @staticmethod
    def relabel_source(old_order, new_order) -> np.ndarray:
        """src[p]: the position at which a layout of order `old_order` holds
        the row of position p of a layout of order `new_order` over the same
        row sequence -- a per-position table moves as table[src]."""
        inv = np.empty(old_order.size, np.int64)
        inv[old_order] = np.arange(old_order.size, dtype=np.int64)
        return inv[new_order]

    def shard(self, rank: int, world: int):
        """(global positions of the shard's rows, local bucket offsets [C+1])."""
        if world == 1:
            return np.arange(self.bucket_off[-1], dtype=np.int64), self.bucket_off.copy()
        parts, loc = [], np.zeros(self.n_buckets + 1, np.int64)
        for c in range(self.n_buckets):
            a, b = self.bucket_off[c], self.bucket_off[c + 1]
            n = b - a
            lo = a + (n * rank) // world
            hi = a + (n * (rank + 1)) // world
            parts.append(np.arange(lo, hi, dtype=np.int64))
            loc[c + 1] = loc[c] + (hi - lo)
        return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), loc


# ---- tags (filtered search: lmi_bucket_topk_tagged) ---------------------------
def check_tags(tags, n: int) -> np.ndarray:
    """`tags` (any integer array, one word per row, values in [0, 2^32)) as
    uint32 [n]; ValueError otherwise."""
    t = tags.cpu().numpy() if hasattr(tags, "cpu") else np.asarray(tags)
    if t.dtype.kind not in "iu":
        raise ValueError("tags must be integers")
    t = t.ravel()
    if t.shape != (n,):
        raise ValueError(f"tags must have one word per row ({n})")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= 1 << 32):
        raise ValueError("tags must lie in [0, 2^32)")
    return np.ascontiguousarray(t.astype(np.uint32))


def eligible_counts(tags_by_pos, bucket_off, want: int, avoid: int = 0) -> np.ndarray:
    """int64 [C]: the rows of every bucket with (tag & want) == want and
    (tag & avoid) == 0 -- a segmented count over `bucket_off` ([C+1] positions into `tags_by_pos`),
    done in torch (imported on the call).  The reference replay of a filtered
    search reads these as its bucket sizes (the < k quirk, the empty-bucket skip)."""
    import torch
    w, m = int(want), int(want) | int(avoid)
    t = torch.from_numpy(np.ascontiguousarray(tags_by_pos, dtype=np.uint32).astype(np.int64))
    ok = (t & m) == w
    cs = torch.zeros(t.numel() + 1, dtype=torch.int64)
    torch.cumsum(ok, 0, out=cs[1:])
    off = torch.from_numpy(np.ascontiguousarray(bucket_off, dtype=np.int64))
    return (cs[off[1:]] - cs[off[:-1]]).numpy()
