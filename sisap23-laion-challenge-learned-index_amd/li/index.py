"""Device-resident LMI index and the search pipeline over liblmi_hip.so.

This is the host side of the hot path (SURVEY.md §3 "Build-side equivalent"):

    queries (HBM) --K1 lmi_router--> classes[:, :R]
                  --K2 lmi_bucket_topk--> per-(query, probe) top-k lists
                  [--RCCL all_gather + K3 lmi_merge_topk, G > 1 ranks]
                  --D2H (nq*R*k*8 B)--> lmi_replay (host C++) --> dists, anns

Layout in HBM (one shard): the search corpus sorted by bucket label, stable in
row order — the order in which the reference's ``groupby('category')`` visits
objects (LearnedIndex.py:143-145) — stored fp16 when every value is exactly
fp16-representable (then the fp16 MFMA products are exact) and fp32 otherwise,
rows padded to a multiple of 32 elements; per-row 1/||y|| (sklearn's
``normalize`` zero rule, utils.py:11); the global position of every row (the
tie-break key); bucket offsets and the chunk table of the scan.

A G-rank index stripes every bucket: rank g holds the g-th contiguous slice of
each bucket's rows (np.array_split boundaries), so every rank scans 1/G of
every probed bucket whatever the bucket popularity.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, index_update
from ._lib import check, ptr
from .index_update import DEFAULT_DIRECT_ROWS, DEFAULT_SLAB_ROWS, STAGING_MAX_BYTES  # noqa: F401
from .layout import DEFAULT_CHUNK_ROWS, BucketLayout, check_tags, default_chunk_rows, eligible_counts  # noqa: F401

SPLIT_D_PAD = 768  # the split mode's (storage "f32x") row width: the fp16 scan's
# LMI_Q_SEED_ROUND0 in the thresholded reference replay (LMI_NO_SEED=1: off,
# for A/B measurements; results are the same either way)
_SEED_ROUND0 = os.environ.get("LMI_NO_SEED") != "1"


def _as_torch(x, device=None, dtype=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if device is not None:
        t = t.to(device)
    return t.contiguous()


def _rows_f32(x, device) -> torch.Tensor:
    """x as float32 rows on `device` for a kernel that takes a row stride
    (ldq / ldx): a device float32 tensor whose rows are contiguous is passed
    as it is (e.g. a column slice of a staged query batch), anything else is
    converted to a contiguous tensor."""
    if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 2 and \
            x.device == torch.device(device) and (x.stride(1) == 1 or x.shape[1] == 1):
        return x
    return _as_torch(x, device, torch.float32)


def _inv_norm(rows: torch.Tensor) -> torch.Tensor:
    """1/||y|| per row as the scan uses it: sklearn normalize's rule (norms <
    10 * eps(float32) -> 1, utils.py:11), the norm computed in float64 from the
    stored values and rounded once to float32, so its relative error is at
    most 2^-24 whatever the reduction order (the float64 mode's refine band
    relies on that bound: refine_eps)."""
    f = rows.double()
    norm = torch.sqrt((f * f).sum(dim=1))
    norm = torch.where(norm < 10 * float(np.finfo(np.float32).eps), torch.ones_like(norm), norm)
    return (1.0 / norm).float()


def _low_norm(rows: torch.Tensor):
    """(mask, 1/||y|| float32) of the rows whose float64 norm lies in
    [10 eps(float64), 10 eps(float32)): _inv_norm scores them with norm 1 (the
    float32 rule), the reference's float64 branch with their true norm."""
    f = rows.double()
    norm = torch.sqrt((f * f).sum(dim=1))
    low = (norm < 10 * float(np.finfo(np.float32).eps)) & (norm >= 10 * float(np.finfo(np.float64).eps))
    return low, (1.0 / torch.where(low, norm, torch.ones_like(norm))).float()


def refine_eps(d_pad: int, f16math: bool, rounded_inputs: bool = False) -> float:
    """The float64 mode's band ε (lmi_bucket_topk_f64): a bound on |d32 - d64|
    for every (query, row), d32 the scan's float32 distance and d64 the
    reference's float64 one, rounded up to a power of two (>= 2^-16).  With
    u = 2^-24, gamma(n) = n*u / (1 - n*u), |cos| <= 1, and every float32
    rounding taken as <= 2u (covers round-to-nearest and truncation):
      dot   fp16 x fp16 products are exact in float32; a v_mfma_f32_32x32x16_f16
            chain adds 16 products per instruction into the accumulator, so a
            product passes at most 16 + d_pad/16 roundings: gamma(h) with
            h = 2 (d_pad/16 + 16) relative to sum |q_i y_i| <= ||q|| ||y||
            (the f32 path, v_mfma_f32_32x32x2_f32 = an fmaf chain: h = 2 (d_pad + 1));
      1/||q|| prep_kernel: per lane 4 * ceil(d_pad/256) fmaf terms, then a
            6-level butterfly: gamma(2 h_q)/2 for the sqrt of the sum, + 4u for
            sqrt and division (<= 2 ulp each);
      1/||y|| float64 norm rounded once (_inv_norm): u -- of the row's true
            norm: the float64 mode reads DeviceIndex.inv_norm64 where a stored
            row's norm is under the float32 zero rule and not under the float64
            one (with inv_norm's 1 such a row's d32 would be ~1 whatever its
            direction, off by up to 2).  Nothing else changes for such rows:
            fp16 products are exact in float32 down to subnormal x subnormal
            (2^-48), and 1/norm <= 1 / (10 eps64) = 4.6e14 (1.7e7 for fp16
            rows, whose smallest non-zero norm is 2^-24) is a normal float32;
      scale (1/||q||)(1/||y||) one multiply: 2u; the final fma: 2u absolute.
    rounded_inputs: float64 rows or queries scanned after rounding to float32
    (lmi_index_desc.corpus64, lmi_bucket_topk_f64q): the cosine of the rounded
    vectors differs from the float64 one by <= 4u; 8u are added.
    d_pad = 768: 9.2e-6 (f16 path) -> 2^-16; 9.3e-5 (f32 path) -> 2^-13."""
    u = 2.0 ** -24

    def gamma(n):
        return n * u / (1.0 - n * u)
    h = 2 * (d_pad // 16 + 16) if f16math else 2 * (d_pad + 1)
    hq = 4 * (-(-d_pad // 256)) + 6
    bound = gamma(h) + gamma(2 * hq) / 2 + 4 * u + u + 2 * u + 2 * u + (8 * u if rounded_inputs else 0.0)
    eps = 2.0 ** -16
    while eps < bound:
        eps *= 2.0
    return eps


def _rows_q(x, device) -> torch.Tensor:
    """Query rows for the scan: float32 rows as _rows_f32; float64 queries stay
    float64 (bucket_topk_f64 keeps them for its float64 recomputation;
    bucket_topk rounds them)."""
    if (isinstance(x, torch.Tensor) and x.dtype == torch.float64) or \
            (isinstance(x, np.ndarray) and x.dtype == np.float64):
        return _as_torch(x, device, torch.float64)
    return _rows_f32(x, device)


def fp16_exact(x: torch.Tensor) -> bool:
    """True when every value of the float tensor round-trips through fp16."""
    x = x.float()
    return bool(torch.equal(x.half().float(), x))


def _as_i32_bits(a: np.ndarray) -> torch.Tensor:
    """uint32 words as an int32 tensor of the same bits (torch has no uint32 gather)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


I8_MAX_D_PAD = 992  # the 8-bit scan's widest row (its query tile in LDS)


def _check_i8_build(capacity, subcluster: bool, world: int, d: int) -> None:
    """What an index of storage "i8" refuses at construction, before anything
    is allocated."""
    if capacity is not None:
        raise ValueError("storage 'i8': no reserved capacity (an 8-bit index takes no updates)")
    if subcluster:
        raise ValueError("storage 'i8' takes no sub-cluster layout (subcluster=True)")
    if world > 1:
        raise ValueError("storage 'i8' is offered on one GPU (world == 1), not on a striped index")
    if (int(d) + 31) // 32 * 32 > I8_MAX_D_PAD:
        raise ValueError(f"storage 'i8' takes rows of at most {I8_MAX_D_PAD} values, not {int(d)}")


def check_i8(index, what: str) -> None:
    """ValueError when `index` is of storage "i8" and `what` (the feature's
    name in the message) is not offered on it; before anything is launched."""
    if getattr(index, "storage", None) == "i8":
        raise ValueError(f"{what} is not offered on storage 'i8' (the 8-bit storage answers float32 lists of "
                         f"at most {_lib.LMI_MAX_K} entries on one GPU)")


def quantize_rows(rows: torch.Tensor, d_pad: int, codes: torch.Tensor, inv_norm: torch.Tensor,
                  dst_rows: Optional[torch.Tensor] = None, stream=None) -> None:
    """lmi_quantize_rows_i8: the device rows [m, d] (fp16 or float32, unit
    stride along a row, any row stride) as int8 codes in `codes` [slots, d_pad]
    and the codes' 1/||c|| in `inv_norm` [slots] -- row i in slot dst_rows[i]
    (device int64 [m]) or, without dst_rows, slot i.  Every slot named must
    exist: the kernel does not check."""
    if rows.dtype not in (torch.float16, torch.float32):
        rows = rows.float()
    if rows.dim() != 2 or (rows.shape[1] > 1 and rows.stride(1) != 1):
        rows = rows.contiguous()
    m, d = int(rows.shape[0]), int(rows.shape[1])
    if codes.dtype != torch.int8 or codes.dim() != 2 or codes.shape[1] != d_pad or not codes.is_contiguous() \
            or inv_norm.dtype != torch.float32 or inv_norm.shape != (codes.shape[0],) \
            or not inv_norm.is_contiguous():
        raise ValueError("quantize_rows: codes must be int8 [slots, d_pad] and inv_norm float32 [slots], contiguous")
    if dst_rows is None:
        if codes.shape[0] < m:
            raise ValueError("quantize_rows: fewer slots than rows")
    elif dst_rows.dtype != torch.int64 or dst_rows.shape != (m,) or not dst_rows.is_contiguous():
        raise ValueError("quantize_rows: dst_rows must be a contiguous int64 [m] device tensor")
    if m == 0:
        return
    ld = max(int(rows.stride(0)), d)  # (a single row may report any stride)
    s = stream if stream is not None else _lib.stream_handle(codes.device)
    check("lmi_quantize_rows_i8", _lib.load().lmi_quantize_rows_i8(
        ptr(rows), _lib.LMI_F16 if rows.dtype == torch.float16 else _lib.LMI_F32, m, ld, d, d_pad,
        ptr(dst_rows), ptr(codes), ptr(inv_norm), s))


# ---------------------------------------------------------------------------
# device index
# ---------------------------------------------------------------------------
class RowSource:
    """A corpus too large to materialise twice (BASELINE configs[4], 100M x 768):
    ``fn(a, b)`` returns rows [a, b) as an fp16 device tensor [b - a, d] and is
    called on whole chunks [i·chunk, (i+1)·chunk).  DeviceIndex scatters every
    chunk straight into its bucket-sorted slots, so HBM holds the shard once."""

    def __init__(self, n: int, d: int, fn, chunk: int = 1 << 20):
        self.n, self.d, self.fn, self.chunk = int(n), int(d), fn, int(chunk)
        self.shape = (self.n, self.d)

    def chunks(self):
        for a in range(0, self.n, self.chunk):
            b = min(self.n, a + self.chunk)
            yield a, b, self.fn(a, b)


class DeviceIndex:
    """One shard of the bucket-sorted search corpus, resident in HBM.

    storage: "f16" (every value fp16-exact: the fp16 MFMA scan is exact),
    "f32x" (float32 values that are not: the split mode of ABI 9 -- the fp16
    scan runs on each row L2-normalised and rounded to fp16, `corpus`, and the
    rows within its rounding bound of every pair's k-th distance are re-scored
    exactly from the float32 rows, `corpus32`; d_pad 768), or "f32" (the
    general exact-fp32 MFMA scan).  "auto" picks the first that applies.

    "i8" (opt-in, never picked by "auto"): the lossy 8-bit storage -- every row
    quantised on the device to int8 codes with one scale per row
    (lmi_quantize_rows_i8; the scale is not kept, the cosine does not need
    it), `corpus` [n_rows, d_pad] int8 and `inv_norm` the codes' 1/||c||.  The
    queries are quantised inside the call by the same rule, and every list is
    the exact top-k of the quantised distances.  One byte a component; one GPU,
    d_pad <= 992, lists of at most 16 entries, float32 lists; no capacity, no
    sub-cluster layout, no updates, no range search (each a ValueError).

    keep_rows=True (storage "i8" alone): the index also holds `rows16`, the
    bucket-sorted fp16 rows [n_rows, d_pad] (zero past d; row r of `rows16` is
    row r of `corpus`, so a list's position indexes both).  Searcher.lists /
    search(..., dist="f64", rerank=k2) then scan k2-entry 8-bit lists and
    re-score them from these rows in float64 (rerank_f64): exact distances on
    an approximate candidate set.  Built from host rows, every value must be
    fp16-representable (the rule of storage "f16"); not with a RowSource,
    whose point is that no fp16 copy exists.  quantized(keep_rows=True) of an
    index of storage "f16" shares that index's corpus tensor (no copy): the
    source must then not be updated in place while this index is in use."""

    rows16 = None  # the fp16 rows kept beside the int8 codes (storage "i8", keep_rows=True)
    _rows_desc = None  # the descriptor over rows16 (rows_desc)
    corpus64 = None  # float64 rows (float64 input that float32 rounding changes)
    corpus32 = None  # float32 rows of the split mode (storage "f32x")
    corpus32n = None  # corpus32 normalised as sklearn does in float32 (ABI 11)
    inv_norm32 = None  # 1/||y|| of corpus32 (the general scan's, k > 16 in f32x)
    # inv_norm with the true 1/||y|| of the rows whose norm lies in [10 eps64,
    # 10 eps32), for the float64 calls; None when no stored row does (_low_norm)
    inv_norm64 = None
    _desc = _desc32 = _desc64 = None   # built on first use (desc, desc_for), dropped by _adopt_store
    consumed = False   # True once an in-place update has taken this index's store (K9)
    # filtered search: every row's 32-bit tag word -- tags_by_pos host uint32
    # [n_total], parallel to pos_to_id; tags device [n_rows] (the words as
    # int32 bits) = tags_by_pos[gpos], a striped shard's own rows'.  None: an
    # untagged index
    tags_by_pos = None
    tags = None
    tags_version = 0  # edit_tags / set_tags calls so far (Searcher drops its eligible-count cache on a change)

    def __init__(self, data, labels, n_buckets: int, *, ids=None, device=None,
                 storage: str = "auto", chunk_rows: Optional[int] = None,
                 rank: int = 0, world: int = 1, subcluster: bool = False,
                 capacity: Optional[int] = None, tags=None, keep_rows: bool = False):
        """`keep_rows` (storage "i8" alone, see the class): keep the fp16 rows
        beside the codes, for Searcher's `rerank`.  ValueError, before anything
        is allocated, with another storage, with a RowSource, or for rows that
        are not fp16-representable.

        `tags` (None: an untagged index): one 32-bit tag word per input row,
        any integer array with values in [0, 2^32), for filtered search
        (Searcher.lists / search with `want`: a row is eligible for a query iff
        (tag & want) == want).  Not with subcluster=True (ValueError).

        `capacity` (None: as many rows as the index holds, today's
        allocation): the rows the corpus and 1/||y|| stores are allocated for,
        so that add / remove with inplace=True can grow the index inside them
        (K9).  `corpus` and `inv_norm` are the leading [n_rows] views of the
        stores; rows past n_rows have unspecified content.  Only for the
        kinds an update supports (one GPU, storage 'f16', no float64 rows, no
        sub-cluster layout): ValueError otherwise, or when below the row
        count."""
        _lib.load()
        if keep_rows:
            if storage != "i8":
                raise ValueError(f"keep_rows: the fp16 rows are kept beside storage 'i8' alone, not {storage!r}")
            if isinstance(data, RowSource):
                raise ValueError("keep_rows: a RowSource builds storage 'i8' so that no fp16 copy exists")
        self._keep_rows = bool(keep_rows)
        self.device = torch.device(device if device is not None else "cuda")
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        self.layout = BucketLayout.from_labels(lab, n_buckets)
        self.n_buckets = n_buckets
        n = int(self.layout.bucket_off[-1])
        self.n_total = n
        if ids is None:
            ids = np.arange(1, n + 1, dtype=np.int64)  # DataFrame.index += 1 (search.py:72)
        ids = np.asarray(ids).astype(np.int64, copy=False)
        if ids.shape != (n,):
            raise ValueError("ids must have one entry per corpus row")
        self.pos_to_id = ids[self.layout.order]
        if tags is not None:
            if subcluster:
                raise ValueError("tags: a sub-cluster layout (subcluster=True) takes no tags")
            self.tags_by_pos = check_tags(tags, n)[self.layout.order]
        self.bucket_size = self.layout.bucket_size.copy()
        self.rank, self.world = rank, world

        gpos, loc_off = self.layout.shard(rank, world)
        self._capacity = None
        if storage == "i8":
            _check_i8_build(capacity, subcluster, world, int(np.shape(data)[1]) if not hasattr(data, "shape")
                            else int(data.shape[1]))
        if capacity is not None:
            if world > 1 or subcluster:
                raise ValueError("capacity: only an index that add / remove support can reserve rows "
                                 "(not a striped index, world > 1, nor a sub-cluster layout)")
            if int(capacity) < n:
                raise ValueError(f"capacity {int(capacity)} is below the {n} rows of the index")
            self._capacity = int(capacity)
        if isinstance(data, RowSource):
            self._fill_from_source(data, gpos, storage)
        else:
            self._fill(data, gpos, storage)
        self.gpos = torch.from_numpy(gpos.astype(np.int32)).to(self.device)
        self.n_rows = int(gpos.size)
        if self.tags_by_pos is not None:
            self.tags = _as_i32_bits(self.tags_by_pos[gpos]).to(self.device)
        cf = self._plan_tables(loc_off, chunk_rows)
        self.chunk_centroid = None
        if subcluster and self.n_chunks > 0:
            self._subcluster_layout(loc_off, cf)
        self._ws = {}

    def _plan_tables(self, loc_off, chunk_rows):
        """chunk_rows and the scan's tables of a shard with the local bucket
        offsets `loc_off` (bucket_off_local, bucket_rows, chunk_first and
        their counts); returns the host chunk table."""
        # (default: by the index's size and world, default_chunk_rows);
        # _chunk_rows_given: an update keeps an explicit value and takes the
        # default of its new size otherwise (DeviceIndex.add / remove)
        self._chunk_rows_given = bool(chunk_rows)
        self.chunk_rows = int(chunk_rows) if chunk_rows else default_chunk_rows(self.world, self.n_total)
        cf = np.zeros(self.n_buckets + 1, np.int32)
        lib = _lib.load()
        mx = lib.lmi_plan_chunks(loc_off.ctypes.data, self.n_buckets, self.chunk_rows, cf.ctypes.data)
        if mx < 0:
            check("lmi_plan_chunks", -mx)
        self.max_chunks = int(mx)
        self.n_chunks = int(cf[-1])
        self.bucket_off_local = torch.from_numpy(loc_off).to(self.device)
        # every bucket's rows in the whole index (lmi_index_desc.bucket_rows):
        # the shape of the reference's per-bucket product
        self.bucket_rows = torch.from_numpy(np.ascontiguousarray(self.bucket_size, dtype=np.int64)).to(self.device)
        self.chunk_first = torch.from_numpy(cf).to(self.device)
        return cf

    # ---- updates (K7: csrc/lmi_update.hip) ----------------------
    @classmethod
    def empty(cls, d: int, n_buckets: int, *, device=None, chunk_rows: Optional[int] = None,
              capacity: Optional[int] = None, tags=None) -> "DeviceIndex":
        """A one-GPU fp16 index of `n_buckets` empty buckets for rows of `d`
        values, to be filled by `add`: what a construction over zero rows
        gives.  `capacity`: rows to reserve for add(..., inplace=True).
        `tags`: True or an empty integer array for a tagged index (its rows
        then come with add(..., tags=...)); None for an untagged one."""
        if int(d) < 1:
            raise ValueError("d must be positive")
        if tags is not None:
            tags = np.zeros(0, np.uint32) if tags is True else tags
        return cls(np.zeros((0, int(d)), np.float16), np.zeros((0,), np.int64), n_buckets,
                   device=device, storage="f16", chunk_rows=chunk_rows, capacity=capacity, tags=tags)

    # ---- the row store (K9: reserved capacity) -------------------
    def _alloc_store(self, n_rows: int, dtype=torch.float16, zero: bool = False, capacity=None):
        """Allocate the corpus and 1/||y|| stores for max(capacity, n_rows)
        rows (`capacity` default: the constructor's) and set `corpus` /
        `inv_norm` to their leading [n_rows] views -- the stores themselves
        when nothing is reserved."""
        cap = self._capacity if capacity is None else capacity
        cap = max(int(cap), n_rows) if cap is not None else n_rows
        make = torch.zeros if zero else torch.empty
        self._adopt_store(make((cap, self.d_pad), dtype=dtype, device=self.device),
                          torch.empty((cap,), dtype=torch.float32, device=self.device), n_rows)

    def _adopt_store(self, store, store_inv, n_rows: int, inv64: bool = False):
        """Take `store` / `store_inv` (fresh, or a consumed index's): the capacity is its rows, `corpus` /
        `inv_norm` the leading [n_rows] views, and descriptors over an earlier store are dropped.
        `inv64`: the rows are in it already and call for an inv_norm64 (_set_inv_norm64)."""
        self._store, self._store_inv, self._capacity = store, store_inv, int(store.shape[0])
        self.corpus, self.inv_norm = store[:n_rows], store_inv[:n_rows]
        self._desc = self._desc32 = self._desc64 = None
        if inv64:
            self._set_inv_norm64()

    @property
    def capacity(self) -> int:
        """Rows the corpus store holds (n_rows when nothing is reserved)."""
        return int(self._capacity)

    def _check_live(self):
        """Refuse a consumed index before anything is launched on it: its
        store belongs to the index the in-place update returned, and its
        offset tables are gone (a captured graph would replay over moved rows
        through freed tables)."""
        if self.consumed:
            raise RuntimeError("this index was updated in place (add / remove / relabel with inplace=True) and "
                               "is consumed: use the index that call returned "
                               "(Searcher.with_index(new))")

    def _consume(self):
        """Drop the device arrays and mark the index consumed."""
        self.consumed = True
        for name in ("corpus", "inv_norm", "_store", "_store_inv", "gpos", "tags", "bucket_off_local",
                     "bucket_rows", "chunk_first", "_desc", "_desc32", "inv_norm64", "_desc64"):
            setattr(self, name, None)
        self._ws = {}

    def reserve(self, rows: int) -> "DeviceIndex":
        """A NEW index with the same content on a store of `rows` rows (the
        one copying step for an index built without a capacity; this index is
        not touched).  ValueError when `rows` is below the row count."""
        self._check_live()
        self._check_updatable()
        if int(rows) < self.n_rows:
            raise ValueError(f"reserve: {int(rows)} rows are below the {self.n_rows} rows of the index")
        new = self._successor(self.layout, self.pos_to_id, self.tags_by_pos)
        new._alloc_store(self.n_rows, capacity=int(rows))
        new.corpus.copy_(self.corpus)
        new.inv_norm.copy_(self.inv_norm)
        if self.inv_norm64 is not None:
            new.inv_norm64 = self.inv_norm64.clone()
        torch.cuda.current_stream(self.device).synchronize()
        return new

    def _successor(self, layout, pos_to_id, tags_by_pos) -> "DeviceIndex":
        """A one-GPU fp16 index over `layout` / `pos_to_id` / `tags_by_pos`
        (None: untagged) with this one's shape and chunk rule: the one place
        besides __init__ that makes a DeviceIndex.  Every table and scalar is
        set; the caller gives it a row store (_alloc_store, _adopt_store)."""
        n_new = int(layout.bucket_off[-1])
        new = object.__new__(DeviceIndex)
        new.device, new.layout, new.n_buckets = self.device, layout, layout.n_buckets
        new.n_total = new.n_rows = n_new
        new.rank, new.world = 0, 1
        new.d, new.d_pad, new.storage = self.d, self.d_pad, self.storage
        new.pos_to_id = pos_to_id
        new.bucket_size = layout.bucket_size.copy()
        new._plan_tables(layout.bucket_off.copy(), self.chunk_rows if self._chunk_rows_given else None)
        new.gpos = torch.arange(n_new, dtype=torch.int32, device=self.device)
        new.tags_by_pos = tags_by_pos
        new.tags = None if tags_by_pos is None else _as_i32_bits(tags_by_pos).to(self.device)
        new.chunk_centroid = None
        new._ws = {}
        return new

    def _check_updatable(self):
        """What add / remove support, refused before any device work."""
        if self.world > 1:
            raise ValueError("index update: a striped index (world > 1) cannot be updated in place of "
                             "a rebuild: stripe boundaries move with the bucket sizes and rows would "
                             "migrate between ranks")
        if self.storage != "f16":
            raise ValueError(f"index update: storage {self.storage!r} is not supported (only 'f16')")
        if self.corpus64 is not None:
            raise ValueError("index update: an index with float64 rows (corpus64) is not supported")
        if self.chunk_centroid is not None:
            raise ValueError("index update: an index with a sub-cluster layout (chunk_centroid) is "
                             "not supported")

    def add(self, rows, labels, ids=None, tags=None, *, inplace: bool = False,
            slab_rows: Optional[int] = None, direct_rows: Optional[int] = None,
            timings: Optional[dict] = None) -> "DeviceIndex":
        """A NEW index with the batch appended to the row sequence: every row
        goes to the end of the bucket `labels` names for it (host or device
        integers), in batch order -- bitwise the index a construction from
        scratch over the concatenated rows, labels and ids gives.  This index
        is not touched.  `rows`: host or device, [m, d] fp16, or fp32 whose
        values are fp16-exact (ValueError otherwise).  `ids` default to the
        ids after the largest one present; ids that repeat or are present
        already raise ValueError.  `tags` (a tagged index only, ValueError on
        an untagged one): the new rows' tag words, default 0.

        inplace=True (K9): the rows move inside this index's own store, which
        the returned index takes over (same corpus.data_ptr()); no second
        corpus is allocated.  The result is the same index, bit for bit.  THIS
        index is consumed: `consumed` becomes True, its device arrays are
        dropped and everything that would launch on it raises RuntimeError --
        go on with Searcher.with_index(new).  Needs n_rows + m <= capacity
        (ValueError otherwise: build with `capacity`, or `reserve`).  Every
        refusal comes before the first row moves and leaves this index in
        use, unchanged.  The call waits for the whole device before it moves
        a row (replays queued on other streams have finished) and again
        before it returns.  `slab_rows`, `direct_rows`: the slab plan's tuning
        (BucketLayout.inplace_slabs; defaults DEFAULT_SLAB_ROWS capped to a
        STAGING_MAX_BYTES staging buffer, DEFAULT_DIRECT_ROWS).  `timings`
        (measurement only): a dict that receives 'move_ms' (device events
        around the row moves), 'moved_rows' and, in place, 'direct_slabs',
        'staged_slabs', 'staged_rows' (of moved_rows) and 'staging_rows' (the
        staging buffer's)."""
        self._check_live()
        self._check_updatable()
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = lab.astype(np.int64, copy=False).ravel()
        m = int(lab.size)
        shape = tuple(rows.shape) if hasattr(rows, "shape") else np.asarray(rows).shape
        if len(shape) != 2 or shape[0] != m or (m and shape[1] != self.d):
            raise ValueError(f"rows must be [{m}, {self.d}] with one row per label")
        if ids is None:
            first = int(self.pos_to_id.max()) + 1 if self.pos_to_id.size else 1
            ids = np.arange(first, first + m, dtype=np.int64)
        ids = np.asarray(ids).astype(np.int64, copy=False).ravel()
        if ids.shape != (m,):
            raise ValueError("ids must have one entry per new row")
        if np.unique(ids).size != m:
            raise ValueError("duplicate ids among the new rows")
        if m and np.isin(self.pos_to_id, ids).any():
            raise ValueError("ids of new rows are already in the index")
        if tags is not None and self.tags_by_pos is None:
            raise ValueError("tags: this index is untagged (build it with `tags`)")
        new_tags = None
        if self.tags_by_pos is not None:
            new_tags = np.zeros(m, np.uint32) if tags is None else check_tags(tags, m)
        return index_update.update(self, np.zeros(0, np.int64), rows, lab, ids, new_tags, inplace=inplace,
                                   slab_rows=slab_rows, direct_rows=direct_rows, timings=timings)

    def remove(self, ids, *, inplace: bool = False, slab_rows: Optional[int] = None,
               direct_rows: Optional[int] = None, timings: Optional[dict] = None) -> "DeviceIndex":
        """A NEW index without the rows of `ids` (this index is not touched):
        bitwise the index a construction from scratch over the remaining rows
        gives.  An id that is not in the index raises KeyError.  inplace=True
        and the other keywords: as `add` -- the survivors move left inside
        this index's store and this index is consumed."""
        self._check_live()
        self._check_updatable()
        ids = np.asarray(ids).astype(np.int64, copy=False).ravel()
        uniq = np.unique(ids)
        if uniq.size != ids.size:
            raise ValueError("duplicate ids to remove")
        drop = np.flatnonzero(np.isin(self.pos_to_id, uniq))
        if drop.size != uniq.size:
            missing = np.setdiff1d(uniq, self.pos_to_id[drop])
            raise KeyError(f"ids not in the index: {missing[:8].tolist()}"
                           + (" ..." if missing.size > 8 else ""))
        none = np.zeros(0, np.int64)
        return index_update.update(self, drop, None, none, none, none.astype(np.uint32), inplace=inplace,
                                   slab_rows=slab_rows, direct_rows=direct_rows, timings=timings)

    # ---- tag edits in place (csrc/lmi_tags.hip) -----------------
    def edit_tags(self, ids, set_bits=0, clear_bits=0) -> None:
        """tag = (tag & ~clear_bits) | set_bits on the stored objects `ids`, in
        THIS index: no successor, nothing consumed, no row moves.  `set_bits`,
        `clear_bits`: an int or one word per id, in [0, 2^32).  The host table
        (tags_by_pos) and the device words (tags; one 4-byte scatter per id, in
        stream order on the current stream) change together, and tags_version
        counts the call.  Deletes by tombstone: edit_tags(ids, set_bits=T),
        search(..., avoid=T), and later remove(ids_with(want=T)) in one batch.
        ValueError before anything is launched: an untagged index, a striped
        shard (world > 1), duplicate ids, words outside [0, 2^32); an id the
        index does not hold raises as `remove` reports it (a KeyError that is a
        ValueError too); a consumed index raises as every call on it does."""
        index_update.edit_tags(self, ids, set_bits, clear_bits)

    def set_tags(self, ids, tags) -> None:
        """The tag words of the stored objects `ids` := `tags` (an int or one
        word per id): edit_tags with every bit cleared first."""
        index_update.edit_tags(self, ids, tags, 0xFFFFFFFF)

    def ids_with(self, want: int = 0, avoid: int = 0) -> np.ndarray:
        """int64: the ids of the stored objects with (tag & want) == want and
        (tag & avoid) == 0, in position order; read from the host table."""
        if self.tags_by_pos is None:
            raise ValueError("ids_with: this index is untagged (build it with `tags`)")
        value, mask = value_mask(_tag_word(want, "want"), _tag_word(avoid, "avoid"))
        return self.pos_to_id[(self.tags_by_pos & mask) == value].astype(np.int64)

    # ---- re-bucket (K8: csrc/lmi_rebucket.hip) ------------------
    _sorted_by_bucket = staticmethod(index_update.sorted_by_bucket)

    @torch.no_grad()
    def relabel(self, labels, n_buckets: Optional[int] = None, *, inplace: bool = False,
                timings=None) -> "DeviceIndex":
        """A NEW index over the same row sequence with the bucket labels
        `labels` (labels[s]: the bucket of sequence row s -- the constructor's
        rows with survivors renumbered and batches appended, as layout.order
        numbers them; host or device integers) and `n_buckets` buckets (default:
        as many as now) -- bitwise the index a construction from scratch over
        the rows in sequence order, these labels and the ids in sequence order
        gives.  The rows move inside HBM (a stable bucket sort of the labels
        and a row gather on the device); the host uploads the old order /
        pos_to_id tables and downloads the new ones.  This index is not
        touched.  `timings` (measurement only): a dict that receives the
        seconds spent in 'sort', 'tables', 'gather' and 'host'.

        inplace=True (K10): the rows change places inside this index's own
        store, which the returned index takes over (same corpus.data_ptr(),
        same capacity); no second corpus is allocated, and no reserved
        capacity is needed, as the row count stays.  The gather is run as two
        passes of disjoint row swaps (lmi_perm_involutions plans them,
        lmi_index_swap_rows moves the rows).  The result is the same index,
        bit for bit.  THIS index is consumed, as by add / remove in place: go
        on with Searcher.with_index(new).  Every refusal -- this method's, and
        a plan whose status is not clean -- comes before the first row moves
        and leaves this index in use, unchanged.  The call waits for the whole
        device before it moves a row and again before it returns.  `timings`
        then receives 'plan' and 'swap' in place of 'gather', and 'plan_ms',
        'plan_rounds', 'swap_ms' (both passes, by device events) and
        'swapped_rows' (rows that change places, per pass)."""
        self._check_live()
        self._check_updatable()
        C_ = self.n_buckets if n_buckets is None else int(n_buckets)
        if C_ < 1:
            raise ValueError("n_buckets must be positive")
        dev, n = self.device, self.n_rows
        if isinstance(labels, torch.Tensor):
            lab = labels
        else:
            lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
        if int(lab.numel()) != n:
            raise ValueError(f"labels must have one entry per row of the index ({n})")
        if lab.dtype not in (torch.int32, torch.int64):
            lab = lab.to(torch.int64)
        lab = lab.reshape(-1).to(dev).contiguous()
        return index_update.relabel(self, lab, C_, inplace, timings)

    @torch.no_grad()
    def _fill(self, data, gpos, storage):
        n = self.n_total
        rows = torch.from_numpy(self.layout.order[gpos])
        if isinstance(data, torch.Tensor):
            src = data
        else:
            a = np.asarray(data)
            a = a if a.dtype in (np.float16, np.float32, np.float64) else a.astype(np.float32)
            src = torch.from_numpy(np.ascontiguousarray(a))
        if src.dim() != 2 or src.shape[0] != n:
            raise ValueError("data must be [n, d] with one row per label")
        src64 = None
        if src.dtype == torch.float64 and storage == "i8":
            src = src.float()  # (the codes come from the float32 values; no corpus64)
        elif src.dtype == torch.float64:
            # float64 rows (a float64 data_search): the scan reads them rounded
            # to float32; the float64 mode recomputes from the float64 values
            # when rounding changed any (lmi_index_desc.corpus64)
            src64 = src
            src = src.float()
            step64 = 1 << 20
            if all(torch.equal(src64[a:a + step64].to(self.device),
                               src[a:a + step64].to(self.device).double())
                   for a in range(0, n, step64)):
                src64 = None
        elif src.dtype not in (torch.float16, torch.float32):
            src = src.float()
        self.d = int(src.shape[1])
        self.d_pad = (self.d + 31) // 32 * 32
        step = 1 << 20
        if src64 is not None:
            self.corpus64 = torch.zeros((int(gpos.size), self.d_pad), dtype=torch.float64,
                                        device=self.device)
            for a in range(0, int(gpos.size), step):
                self.corpus64[a:a + step, : self.d] = src64.index_select(
                    0, rows[a:a + step].to(src64.device)).to(self.device)
        if storage == "auto":
            storage = "f16" if src.dtype == torch.float16 or all(
                fp16_exact(src[a:a + step].to(self.device)) for a in range(0, n, step)) else \
                ("f32x" if self.d_pad == SPLIT_D_PAD else "f32")
        if storage not in ("f16", "f32", "f32x", "i8"):
            raise ValueError("storage must be 'auto', 'f16', 'f32', 'f32x' or 'i8'")
        if storage == "f32x" and self.d_pad != SPLIT_D_PAD:
            raise ValueError(f"storage='f32x' needs d_pad {SPLIT_D_PAD}")
        self.storage = storage
        tdt = torch.float32 if storage == "f32" else torch.float16
        n_rows = int(gpos.size)
        if self._capacity is not None and (storage != "f16" or src64 is not None):
            raise ValueError("capacity: only an index that add / remove support can reserve rows "
                             f"(storage 'f16' without float64 rows; this one is {storage!r}"
                             + (" with corpus64)" if src64 is not None else ")"))
        if storage == "i8":
            # every block quantised on the device into its slots of the int8
            # store: the codes plus one uploaded block at the peak
            keep = getattr(self, "_keep_rows", False)
            if keep and src.dtype != torch.float16 and not all(
                    fp16_exact(src[a:a + step]) for a in range(0, n, step)):
                raise ValueError("keep_rows needs fp16-representable data (the rule of storage='f16')")
            self._alloc_store(n_rows, torch.int8)
            if keep:
                self.rows16 = torch.zeros((n_rows, self.d_pad), dtype=torch.float16, device=self.device)
            for a in range(0, n_rows, step):
                blk = src.index_select(0, rows[a:a + step].to(src.device)).to(self.device)
                quantize_rows(blk, self.d_pad, self.corpus[a:a + step], self.inv_norm[a:a + step])
                if keep:
                    self.rows16[a:a + step, : self.d] = blk.half()
                del blk
            torch.cuda.current_stream(self.device).synchronize()
            return
        self._alloc_store(n_rows, tdt, zero=True)
        if storage == "f32x":
            self.corpus32 = torch.zeros((n_rows, self.d_pad), dtype=torch.float32, device=self.device)
            self.inv_norm32 = torch.empty((n_rows,), dtype=torch.float32, device=self.device)
        for a in range(0, n_rows, step):
            blk = src.index_select(0, rows[a:a + step].to(src.device)).to(self.device)
            f = blk.float()
            if storage == "f16" and blk.dtype != torch.float16 and not fp16_exact(f):
                raise ValueError("storage='f16' needs fp16-representable data (exact products)")
            if storage == "f32x":
                # the rows as given, and each row / its float64 norm (sklearn's
                # zero rule) rounded to fp16: the split mode's scan rows
                self.corpus32[a:a + step, : self.d] = f
                self.inv_norm32[a:a + step] = _inv_norm(f)
                nrm = torch.sqrt((f.double() * f.double()).sum(dim=1))
                nrm = torch.where(nrm < 10 * float(np.finfo(np.float32).eps), torch.ones_like(nrm), nrm)
                h = (f.double() / nrm[:, None]).float().half()
                self.corpus[a:a + step, : self.d] = h
                self.inv_norm[a:a + step] = _inv_norm(h)
                del blk, f, h, nrm
                continue
            self.corpus[a:a + step, : self.d] = blk.to(tdt)
            self.inv_norm[a:a + step] = _inv_norm(blk.to(tdt))
            del blk, f
        if storage != "f32x":
            self._set_inv_norm64()
        if storage == "f32x" and self.d % 16 == 0 and os.environ.get("LMI_SPLIT_NORM32", "1") != "0":
            # every row divided by its float32 norm as the reference's
            # normalize(Y) computes it, once (lmi_index_desc.corpus32n): the
            # float32 re-score then runs only the product's chains per row
            # (LMI_SPLIT_NORM32=0: normalised per candidate; the same values)
            self.corpus32n = torch.empty_like(self.corpus32)
            check("lmi_split_normalize", _lib.load().lmi_split_normalize(
                ptr(self.corpus32), n_rows, self.d, self.d_pad, ptr(self.corpus32n),
                _lib.stream_handle(self.device)))

    @torch.no_grad()
    def _fill_from_source(self, src: "RowSource", gpos, storage="auto"):
        """Scatter every generated chunk into this shard's bucket-sorted slots
        (fp16 storage; 1/||y|| as sklearn's normalize, zero norms -> 1).
        storage "i8": every chunk quantised straight into its slots
        (lmi_quantize_rows_i8's dst_rows), so no fp16 copy of the corpus exists."""
        n = self.n_total
        if src.n != n:
            raise ValueError("RowSource must have one row per label")
        if storage not in ("auto", "f16", "i8"):
            raise ValueError("a RowSource builds storage 'f16' ('auto') or 'i8'")
        self.d = src.d
        self.d_pad = (self.d + 31) // 32 * 32
        self.storage = "i8" if storage == "i8" else "f16"
        n_rows = int(gpos.size)
        if self.storage == "i8":
            self._alloc_store(n_rows, torch.int8)
        else:
            self._alloc_store(n_rows, torch.float16, zero=True)
        slot = torch.full((n,), -1, dtype=torch.int64, device=self.device)
        slot[torch.from_numpy(self.layout.order[gpos]).to(self.device)] = torch.arange(
            n_rows, dtype=torch.int64, device=self.device)
        for a, b, blk in src.chunks():
            if blk.dtype != torch.float16 or blk.shape != (b - a, self.d):
                raise ValueError("RowSource chunks must be fp16 [b - a, d]")
            sl = slot[a:b]
            m = sl >= 0
            dst = sl[m]
            x = blk[m]
            if self.storage == "i8":
                quantize_rows(x, self.d_pad, self.corpus, self.inv_norm, dst_rows=dst)
                del blk, x
                continue
            self.corpus[dst, : self.d] = x
            self.inv_norm[dst] = _inv_norm(x)
            del blk, x
        del slot
        if self.storage == "i8":
            torch.cuda.current_stream(self.device).synchronize()
            return
        self._set_inv_norm64()

    @torch.no_grad()
    def _set_inv_norm64(self):
        """inv_norm64 from the stored rows (storage 'f16' / 'f32'): None, or
        a copy of inv_norm in which the rows _low_norm finds hold their true
        1/||y||.  Such a row's inv_norm is exactly 1, so only the rows with
        that value are read again.  A function of the stored values alone: an
        update that calls this gets the table of the index built from
        scratch."""
        self.inv_norm64 = self._desc64 = None
        cand = torch.nonzero(self.inv_norm == 1.0).flatten()
        step = 1 << 16
        for a in range(0, int(cand.numel()), step):
            at = cand[a:a + step]
            low, inv = _low_norm(self.corpus.index_select(0, at))
            if bool(low.any()):
                if self.inv_norm64 is None:
                    self.inv_norm64 = self.inv_norm.clone()
                self.inv_norm64[at[low]] = inv[low]

    @torch.no_grad()
    def _subcluster_layout(self, loc_off, cf, iters: int = 8, seed: int = 1):
        """Lay out every bucket of more than one chunk by sub-cluster and keep
        each chunk's unit centroid (lmi_index_desc.chunk_centroid).

        Spherical k-means with one centroid per chunk groups the bucket's rows;
        the rows are ordered by (sub-cluster, global position), cut into the
        usual chunks, and every chunk is put back in ascending global position
        (the scan's tie order inside a chunk).  Only the order of rows inside a
        bucket changes: results are identical with or without it; the scan
        uses the centroids to visit each (query, probe)'s nearest chunk first,
        which tightens its pruning bound early (index build, not hot path)."""
        d, cr = self.d, self.chunk_rows
        cent = torch.zeros((self.n_chunks, self.d_pad), dtype=torch.float32, device=self.device)
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for c in range(self.n_buckets):
            a, b = int(loc_off[c]), int(loc_off[c + 1])
            nch = int(cf[c + 1] - cf[c])
            if nch == 0:
                continue
            if nch > 1:
                x = self.corpus[a:b, :d].float()
                x = x * self.inv_norm[a:b, None]
                n = b - a
                init = torch.randperm(n, generator=g, device=self.device)[:nch]
                ctr = x[init].clone()
                for _ in range(iters):
                    lab = (x @ ctr.T).argmax(dim=1)
                    s = torch.zeros_like(ctr).index_add_(0, lab, x)
                    nrm = s.norm(dim=1, keepdim=True)
                    ctr = torch.where(nrm > 0, s / nrm.clamp(min=1e-30), ctr)
                lab = (x @ ctr.T).argmax(dim=1)
                del x
                gp = self.gpos[a:b].long()
                # order by (sub-cluster, global position), cut into chunks, and
                # restore ascending global position inside every chunk
                order = torch.argsort(lab * (1 << 32) + gp)
                chunk_of = torch.arange(n, device=self.device) // cr
                order = order[torch.argsort(chunk_of * (1 << 32) + gp[order])]
                self.corpus[a:b] = self.corpus[a:b][order]
                self.inv_norm[a:b] = self.inv_norm[a:b][order]
                self.gpos[a:b] = self.gpos[a:b][order]
                # the row arrays that share corpus's local row index (the
                # split mode's float32 rows, the float64 rows) move with it
                for name in ("corpus32", "corpus32n", "inv_norm32", "corpus64", "inv_norm64"):
                    t = getattr(self, name)
                    if t is not None:
                        t[a:b] = t[a:b][order]
            for j in range(nch):
                ra, rb = a + j * cr, min(b, a + (j + 1) * cr)
                v = (self.corpus[ra:rb, :d].float() * self.inv_norm[ra:rb, None]).sum(dim=0)
                cent[int(cf[c]) + j, :d] = v / v.norm().clamp(min=1e-30)
        self.chunk_centroid = cent

    @torch.no_grad()
    def quantized(self, keep_rows: bool = False) -> "DeviceIndex":
        """A NEW index of storage "i8" with this one's rows quantised on the
        device (lmi_quantize_rows_i8 over the stored rows): the same layout,
        ids, tags and chunk tables, and bitwise the index
        DeviceIndex(rows, ..., storage="i8") builds from the same rows.  This
        index is not touched.  For a live one-GPU index of storage "f16" or
        "f32" without a sub-cluster layout (ValueError otherwise); float64
        rows kept beside a float32 store (corpus64) are not carried over.
        keep_rows=True (storage "f16" alone, else ValueError): the new index's
        `rows16` is this index's corpus tensor itself -- no copy; do not update
        this index in place while the new one is in use."""
        self._check_live()
        if self.storage not in ("f16", "f32"):
            raise ValueError(f"quantized: storage {self.storage!r} is not supported (only 'f16' and 'f32')")
        if keep_rows and self.storage != "f16":
            raise ValueError(f"quantized(keep_rows=True): the kept rows are fp16 (storage 'f16'), not {self.storage!r}")
        if self.world > 1:
            raise ValueError("quantized: storage 'i8' is offered on one GPU (world == 1), not on a stripe")
        if self.chunk_centroid is not None:
            raise ValueError("quantized: storage 'i8' takes no sub-cluster layout (chunk_centroid)")
        _check_i8_build(None, False, 1, self.d)
        new = self._successor(self.layout, self.pos_to_id, self.tags_by_pos)
        new.storage = "i8"
        new._adopt_store(torch.empty((self.n_rows, self.d_pad), dtype=torch.int8, device=self.device),
                         torch.empty((self.n_rows,), dtype=torch.float32, device=self.device), self.n_rows)
        quantize_rows(self.corpus[:, : self.d], self.d_pad, new.corpus, new.inv_norm)
        if keep_rows:
            new.rows16 = self.corpus
        torch.cuda.current_stream(self.device).synchronize()
        return new

    @property
    def rows_desc(self) -> _lib.IndexDesc:
        """The descriptor of the kept fp16 rows (`rows16`) that lmi_rerank_f64
        takes: the rows, their width and count; nothing else is read."""
        self._check_live()
        if self.rows16 is None:
            raise ValueError("this index keeps no fp16 rows (build it with storage='i8', keep_rows=True)")
        if self._rows_desc is None:
            d = _lib.IndexDesc()
            d.corpus = ptr(self.rows16)
            d.dtype = _lib.LMI_F16
            d.d, d.d_pad, d.n_rows = self.d, self.d_pad, self.n_rows
            d.n_buckets = self.n_buckets
            self._rows_desc = d
        return self._rows_desc

    @property
    def desc(self) -> _lib.IndexDesc:
        self._check_live()
        if self._desc is None:
            self._desc = IndexDescHolder(self)
        return self._desc.desc

    def desc_for(self, k: int, f64: bool = False) -> _lib.IndexDesc:
        """The descriptor a call with k entries per list takes: the split mode
        (storage "f32x") holds k <= LMI_MAX_K; wider lists scan the float32
        rows with the general exact-fp32 kernel (a second descriptor over
        corpus32).  `f64` (the lmi_bucket_topk_f64* calls): the descriptor
        over inv_norm64 in place of inv_norm, where the index keeps one."""
        if f64 and self.inv_norm64 is not None:
            self._check_live()
            if self._desc64 is None:
                self._desc64 = IndexDescHolder(self, inv_norm=self.inv_norm64)
            return self._desc64.desc
        if self.storage != "f32x" or k <= _lib.LMI_MAX_K:
            return self.desc
        if self._desc32 is None:
            self._desc32 = IndexDescHolder(self, general32=True)
        return self._desc32.desc

    def workspace(self, nq: int, R: int, k: int, qmode: int) -> torch.Tensor:
        lib = _lib.load()
        need = lib.lmi_scan_workspace_bytes(C.byref(self.desc_for(k)), nq, R, k, qmode)
        ws = self._ws.get("buf")
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._ws["buf"] = ws
        return ws


class IndexDescHolder:
    def __init__(self, ix: DeviceIndex, general32: bool = False, inv_norm=None):
        d = _lib.IndexDesc()
        d.corpus = ptr(ix.corpus32 if general32 else ix.corpus)
        d.dtype = _lib.LMI_F32 if (general32 or ix.storage == "f32") else \
            _lib.LMI_I8 if ix.storage == "i8" else _lib.LMI_F16
        d.d = ix.d
        d.d_pad = ix.d_pad
        d.n_rows = ix.n_rows
        d.inv_norm = ptr(inv_norm if inv_norm is not None else ix.inv_norm32 if general32 else ix.inv_norm)
        d.gpos = ptr(ix.gpos)
        d.n_buckets = ix.n_buckets
        d.bucket_off = ptr(ix.bucket_off_local)
        d.chunk_rows = ix.chunk_rows
        d.chunk_first = ptr(ix.chunk_first)
        d.n_chunks = ix.n_chunks
        d.max_chunks = ix.max_chunks
        d.chunk_centroid = ptr(ix.chunk_centroid) if ix.chunk_centroid is not None else None
        d.corpus64 = ptr(ix.corpus64) if ix.corpus64 is not None else None
        d.corpus32 = ptr(ix.corpus32) if (ix.corpus32 is not None and not general32) else None
        d.bucket_rows = ptr(ix.bucket_rows)
        d.corpus32n = ptr(ix.corpus32n) if (ix.corpus32n is not None and not general32) else None
        self.desc = d


# ---------------------------------------------------------------------------
# router
# ---------------------------------------------------------------------------
def check_stop(stop_mass, min_probes=1) -> None:
    """Arguments of the probability-mass stop rule (None: the rule is off), as
    lmi_router_stop checks them, raised as ValueError before any device call."""
    if stop_mass is None:
        return
    # (the float32 value the kernel compares with; a NaN fails both comparisons)
    if not 0.0 < float(np.float32(stop_mass)) <= 1.0:
        raise ValueError(f"stop_mass must lie in (0, 1], got {stop_mass}")
    if int(min_probes) != min_probes or int(min_probes) < 1:
        raise ValueError(f"min_probes must be an integer >= 1, got {min_probes}")


def probe_stop_mask(probs, stop_mass, min_probes: int = 1) -> np.ndarray:
    """The stop rule of lmi_router_stop, restated in numpy: `probs` [nq, R] are
    the float32 probabilities of the picks in rank order; the result [nq, R]
    (bool) is True where probe r is kept:

        S_0 = 0,  S_{r+1} = fl32(S_r + p_r)   (float32, ascending r)
        keep[r]  <=>  r < min_probes  or  S_r < stop_mass

    The kept probes are a prefix (the S_r do not decrease)."""
    check_stop(stop_mass, min_probes)
    p = np.asarray(probs, dtype=np.float32)
    if p.ndim != 2:
        raise ValueError("probs must be [nq, R]")
    nq, R = p.shape
    keep = np.zeros((nq, R), dtype=bool)
    mass = np.zeros((nq,), dtype=np.float32)
    sm = np.float32(stop_mass)
    for r in range(R):
        keep[:, r] = (mass < sm) if r >= min_probes else True
        mass = (mass + p[:, r]).astype(np.float32)
    return keep


class DeviceRouter:
    """Weights of a Linear/ReLU stack in HBM, evaluated by K1 (lmi_router)."""

    def __init__(self, layers: Sequence, device=None):
        _lib.load()
        self.device = torch.device(device if device is not None else "cuda")
        if not 1 <= len(layers) <= _lib.LMI_MAX_LAYERS:
            raise ValueError("1..8 Linear layers supported")
        self.W, self.b = [], []
        dims = [int(_as_torch(layers[0][0]).shape[1])]
        for (w, b) in layers:
            w = _as_torch(w, self.device, torch.float32)
            b = _as_torch(b, self.device, torch.float32)
            if w.shape[1] != dims[-1] or b.shape != (w.shape[0],):
                raise ValueError("inconsistent layer shapes")
            dims.append(int(w.shape[0]))
            self.W.append(w)
            self.b.append(b)
        self.dims = dims
        self.n_classes = dims[-1]
        m = _lib.MlpDesc()
        m.n_layers = len(self.W)
        for i, v in enumerate(dims):
            m.dims[i] = v
        for i, (w, b) in enumerate(zip(self.W, self.b)):
            m.W[i] = ptr(w)
            m.b[i] = ptr(b)
        self._desc = m

    @classmethod
    def from_module(cls, module: torch.nn.Module, device=None) -> "DeviceRouter":
        """From a reference-shaped ``Model`` (model.py:15-83): ``layers`` is a
        Sequential of Linear with ReLU between consecutive Linears."""
        seq = getattr(module, "layers", module)
        mods = list(seq.children()) if isinstance(seq, torch.nn.Sequential) else [seq]
        layers = []
        for i, m in enumerate(mods):
            if isinstance(m, torch.nn.Linear):
                layers.append((m.weight.detach(), m.bias.detach()))
            elif isinstance(m, torch.nn.ReLU):
                if not layers or i == len(mods) - 1:
                    raise ValueError("ReLU must sit between Linear layers")
            else:
                raise ValueError(f"unsupported router layer {type(m).__name__}")
        for a, b in zip(mods, mods[1:]):
            if isinstance(a, torch.nn.Linear) and not isinstance(b, torch.nn.ReLU):
                raise ValueError("expected ReLU after every hidden Linear")
        return cls(layers, device)

    def topr(self, x: torch.Tensor, R: int, with_probs: bool = False, stream=None, out=None,
             stop_mass=None, min_probes: int = 1, n_probes_out=None):
        """K1 TOPR: classes [nq, R] int32 (into `out` when given, a contiguous
        int32 tensor of nq*R elements) and, with `with_probs`, their softmax
        probabilities.

        `stop_mass` (None: off, lmi_router exactly as without the argument):
        the probability-mass stop rule of lmi_router_stop, in the same launch
        -- probe r is kept iff r < min_probes or the float32 sum of the
        probabilities of the picks before it is below stop_mass
        (probe_stop_mask); a dropped probe's class is LMI_PROBE_NONE (-1), the
        probabilities are those of the plain call for every r.  `n_probes_out`
        (a contiguous int32 tensor of nq elements) receives the probes kept."""
        check_stop(stop_mass, min_probes)
        if stop_mass is None and n_probes_out is not None:
            raise ValueError("n_probes_out needs stop_mass")
        x = _rows_f32(x, self.device)
        nq = x.shape[0]
        if out is not None:
            if out.dtype != torch.int32 or out.numel() != nq * R or not out.is_contiguous():
                raise ValueError("out must be a contiguous int32 tensor of nq*R elements")
            classes = out.view(nq, R)
        else:
            classes = torch.empty((nq, R), dtype=torch.int32, device=self.device)
        probs = torch.empty((nq, R), dtype=torch.float32, device=self.device) if with_probs else None
        s = stream if stream is not None else _lib.stream_handle(self.device)
        if stop_mass is not None:
            if n_probes_out is not None and (n_probes_out.dtype != torch.int32
                                             or n_probes_out.numel() != nq
                                             or not n_probes_out.is_contiguous()):
                raise ValueError("n_probes_out must be a contiguous int32 tensor of nq elements")
            check("lmi_router_stop", _lib.load().lmi_router_stop(
                ptr(x), nq, x.stride(0), C.byref(self._desc), R, float(stop_mass), int(min_probes),
                ptr(classes), ptr(probs), ptr(n_probes_out), s))
            return classes, probs
        check("lmi_router", _lib.load().lmi_router(ptr(x), nq, x.stride(0), C.byref(self._desc), R,
                                                   _lib.LMI_ROUTER_TOPR, ptr(classes), ptr(probs), s))
        return classes, probs

    def argmax(self, x: torch.Tensor, stream=None) -> torch.Tensor:
        x = _rows_f32(x, self.device)
        nq = x.shape[0]
        out = torch.empty((nq,), dtype=torch.int32, device=self.device)
        s = stream if stream is not None else _lib.stream_handle(self.device)
        check("lmi_router", _lib.load().lmi_router(ptr(x), nq, x.stride(0), C.byref(self._desc), 1,
                                                   _lib.LMI_ROUTER_ARGMAX, ptr(out), 0, s))
        return out


# ---------------------------------------------------------------------------
# scan / merge / replay
# ---------------------------------------------------------------------------
def _workspace(ws, need: int, what: str) -> torch.Tensor:
    if ws.dtype != torch.uint8 or ws.numel() < need:
        raise ValueError(f"{what} workspace too small ({ws.numel()} < {need} bytes)")
    return ws


class i8_lists16:
    """Inside this context the calling thread's scans of an index of storage
    "i8" at d_pad 768 run k = 11..16 on the 8-bit ring's 16-entry lists
    (lmi_scan_set_i8_lists16) instead of scan_i8_kernel: the same lists bit for
    bit, about a fifth of the time.  Off by default, so that every call keeps
    the plan (kernel family, workspace size) it had; bucket_topk(...,
    lists16=True) and the re-rank of Searcher turn it on for their own scan."""

    def __enter__(self):
        self.prev = _lib.load().lmi_scan_set_i8_lists16(1)
        return self

    def __exit__(self, *exc):
        _lib.load().lmi_scan_set_i8_lists16(self.prev)


def bucket_topk(index: DeviceIndex, q: torch.Tensor, classes: torch.Tensor, k: int,
                qmode: Optional[int] = None, stream=None, out=None, ws=None,
                seed_round0: bool = False, phases: int = 0, want=None, avoid=None, lists16: bool = False):
    """K2 on one shard.  Returns (d [nq,R,k] f32, pos [nq,R,k] int32, status int32 tensor);
    `out` = such a triple to write into (the status word zeroed by the caller);
    `ws` = a caller-owned uint8 workspace (default: the index's cached one,
    which a later call with a larger batch may replace — a captured graph
    passes its own).  `seed_round0` (LMI_Q_SEED_ROUND0, the thresholded
    replay only): probes r >= 1 keep only objects under the round-0 bound.
    `phases` (LMI_Q_PHASE_* bits, 0 = all): run only those phases of the call
    (StreamedSearch overlaps one batch's plan with another's scan).
    `want` (a tagged index; device int32 [nq], the want words' bits, see
    want_words): the tagged scan, lmi_bucket_topk_masked -- only rows with
    (tag & want) == want are listed; never seeded, no phases.  `avoid` (the
    same form; alone it means want = 0): and only rows with (tag & avoid) == 0.
    At this level the words are on the device: that no query wants and avoids
    one bit is the caller's check (mask_words makes it on the host).
    `lists16`: the call runs inside i8_lists16() (storage "i8" at d_pad 768:
    k = 11..16 on the ring's 16-entry lists; the workspace is sized there too)."""
    if lists16:
        with i8_lists16():
            return bucket_topk(index, q, classes, k, qmode=qmode, stream=stream, out=out, ws=ws,
                               seed_round0=seed_round0, phases=phases, want=want, avoid=avoid)
    lib = _lib.load()
    q = _rows_f32(q, index.device)
    classes = _as_torch(classes, index.device, torch.int32)
    nq, R = classes.shape
    if q.shape[0] != nq or q.shape[1] != index.d:
        raise ValueError("query shape does not match the index")
    if index.storage == "i8":
        if k > _lib.LMI_MAX_K:
            raise ValueError(f"storage 'i8' takes lists of at most {_lib.LMI_MAX_K} entries, not {k}")
        # (the one query class of the 8-bit storage; its scan is never seeded)
        qmode, seed_round0 = _lib.LMI_Q_I8, False
    if qmode is None:
        qmode = _lib.LMI_Q_F16 if index.storage == "f16" else _lib.LMI_Q_F32
    if want is not None or avoid is not None:
        return _bucket_topk_tagged(index, q, classes, k, qmode, want, avoid, stream, out, ws, phases)
    desc = index.desc_for(k)
    if out is None:
        out_d = torch.empty((nq, R, k), dtype=torch.float32, device=index.device)
        out_pos = torch.empty((nq, R, k), dtype=torch.int32, device=index.device)
        status = torch.zeros((1,), dtype=torch.int32, device=index.device)
    else:
        out_d, out_pos, status = out
    if ws is None:
        ws = index.workspace(nq, R, k, qmode)
    else:
        _workspace(ws, lib.lmi_scan_workspace_bytes(C.byref(desc), nq, R, k, qmode), "scan")
    s = stream if stream is not None else _lib.stream_handle(index.device)
    if index.storage == "f32x":
        seed_round0 = False  # (the split mode scans every pair whole)
    flags = (_lib.LMI_Q_SEED_ROUND0 if seed_round0 else 0) | phases
    check("lmi_bucket_topk", lib.lmi_bucket_topk(C.byref(desc), ptr(q), nq, q.stride(0),
                                                 ptr(classes), R, k, qmode | flags, ptr(out_d),
                                                 ptr(out_pos), ptr(status), ptr(ws), ws.numel(), s))
    return out_d, out_pos, status


SCAN_FAMILIES = ("general", "ring4", "ring8", "ring8-i8")


def scan_family(index: DeviceIndex, k: int, tagged: bool = False, qmode: Optional[int] = None,
                lists16: bool = False) -> str:
    """The kernel family bucket_topk (tagged: with want / avoid) of this index
    and k scans with -- "general" | "ring4" | "ring8" | "ring8-i8" -- as
    lmi_scan_family reads it from the plan the launch uses (the diagnostic
    switches LMI_SCAN_V1 / LMI_SCAN_V2 included).  `qmode` as in bucket_topk;
    `lists16`: the family of bucket_topk(..., lists16=True), the re-rank's scan."""
    if lists16:
        with i8_lists16():
            return scan_family(index, k, tagged, qmode)
    if index.storage == "i8":
        qmode = _lib.LMI_Q_I8
    elif qmode is None:
        qmode = _lib.LMI_Q_F16 if index.storage == "f16" else _lib.LMI_Q_F32
    fam = _lib.load().lmi_scan_family(C.byref(index.desc_for(k)), k, qmode, 1 if tagged else 0)
    if fam < 0:
        check("lmi_scan_family", -fam)
    return SCAN_FAMILIES[fam]


def want_words(index: DeviceIndex, want, nq: int, k_list: int, dist: str = "f32",
               per_query: bool = True) -> torch.Tensor:
    """The want words of a filtered scan as a device int32 [nq] tensor (the
    uint32 words' bits), after every check a filtered call makes before it
    launches or allocates anything: ValueError on an untagged index, on
    dist="f64", on storage "f32x", on k_list > LMI_MAX_K, and for a `want` that
    is neither an integer in [0, 2^32) nor (per_query) an integer array [nq]
    of such."""
    return _as_i32_bits(_host_words(index, want, nq, k_list, dist, per_query, "want")).to(index.device)


def _host_words(index, word, nq, k_list, dist, per_query, name) -> np.ndarray:
    """want_words' checks on the words `word` of the keyword `name`; host uint32 [nq]."""
    if index.tags is None:
        raise ValueError(f"{name}: this index is untagged (build it with `tags`)")
    if dist != "f32":
        raise ValueError(f"{name}: filtered search is not offered with dist='f64'")
    if index.storage == "f32x":
        raise ValueError(f"{name}: filtered search is not offered on storage 'f32x' (the split mode)")
    if k_list > _lib.LMI_MAX_K:
        raise ValueError(f"{name}: filtered search takes lists of at most {_lib.LMI_MAX_K} entries, not {k_list}")
    if isinstance(word, (int, np.integer)) and not isinstance(word, bool):
        if not 0 <= int(word) < 1 << 32:
            raise ValueError(f"{name} must lie in [0, 2^32)")
        return np.full(nq, int(word), np.uint32)
    if not per_query:
        raise ValueError(f"{name}: semantics='reference' takes one {name} word for the whole batch (an int): "
                         "its round merge couples the queries of a batch")
    w = word.cpu().numpy() if isinstance(word, torch.Tensor) else np.asarray(word)
    if w.dtype.kind not in "iu" or w.shape != (nq,):
        raise ValueError(f"{name} must be an integer or an integer array of shape [{nq}]")
    if w.size and (int(w.min()) < 0 or int(w.max()) >= 1 << 32):
        raise ValueError(f"{name} must lie in [0, 2^32)")
    return w.astype(np.uint32)


def _tag_word(word, name: str) -> int:
    if not isinstance(word, (int, np.integer)) or isinstance(word, bool) or not 0 <= int(word) < 1 << 32:
        raise ValueError(f"{name} must be an integer in [0, 2^32)")
    return int(word)


def value_mask(want, avoid):
    """(value, mask) of the scan's one test (tag & mask) == value from the
    all-of word(s) `want` and the none-of word(s) `avoid` (ints or uint32
    arrays of one shape): value = want, mask = want | avoid.  ValueError where
    a word wants and avoids the same bit: the test would read it as wanted."""
    w, a = np.asarray(want, dtype=np.uint32), np.asarray(avoid, dtype=np.uint32)
    both = w & a
    if both.any():
        i = int(np.flatnonzero(both.ravel())[0])
        raise ValueError(f"want and avoid share bits (0x{int(both.ravel()[i]):x}"
                         + (f" at query {i}" if both.ndim else "") + "): a bit cannot be both wanted and avoided")
    return w, w | a


def mask_words(index: DeviceIndex, want, avoid, nq: int, k_list: int, dist: str = "f32",
               per_query: bool = True) -> torch.Tensor:
    """The words of a filtered scan with `want` and / or `avoid` (each None, an
    int or, per_query, an integer array [nq]; None: 0) as one device int32
    [2, nq] tensor -- row 0 the value words (want), row 1 the mask words
    (want | avoid) -- after every check of want_words on each of the two and
    value_mask's: all on the host, before anything is launched or allocated.
    bucket_topk / bucket_range take it as their `want`."""
    value, mask = value_mask(*(_host_words(index, 0 if word is None else word, nq, k_list, dist, per_query, name)
                               for name, word in (("want", want), ("avoid", avoid))))
    return _as_i32_bits(np.stack([value, mask])).to(index.device)


def filter_words(index: DeviceIndex, want, avoid, nq: int, k_list: int, dist: str = "f32",
                 per_query: bool = True):
    """What Searcher's calls hand their scans as `want` for the keywords `want`
    and `avoid`: None (neither given), want_words (want alone: the call as it
    was before `avoid`) or mask_words."""
    if avoid is None:
        return None if want is None else want_words(index, want, nq, k_list, dist, per_query)
    return mask_words(index, want, avoid, nq, k_list, dist, per_query)


def _tag_words(want, avoid, nq, device):
    """bucket_topk's / bucket_range's (value, mask) device tensors from their
    `want` ([nq], or mask_words' [2, nq]) and `avoid` ([nq] or None)."""
    def ok(t, shape):
        return (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == shape
                and t.device == device and t.is_contiguous())
    if want is not None and ok(want, (2, nq)):
        if avoid is not None:
            raise ValueError("avoid: the [2, nq] words of mask_words hold the avoided bits already")
        return want[0], want[1]
    if want is not None and not ok(want, (nq,)):
        raise ValueError("want must be a device int32 tensor [nq] (want_words) or [2, nq] (mask_words)")
    if avoid is None:
        return want, want
    if not ok(avoid, (nq,)):
        raise ValueError("avoid must be a device int32 tensor [nq] (want_words)")
    if want is None:
        return torch.zeros_like(avoid), avoid
    return want, torch.bitwise_or(want, avoid)


def _bucket_topk_tagged(index, q, classes, k, qmode, want, avoid, stream, out, ws, phases):
    """bucket_topk's tagged call (q, classes already on the device)."""
    lib = _lib.load()
    nq, R = classes.shape
    if index.tags is None:
        raise ValueError("want / avoid: this index is untagged (build it with `tags`)")
    if phases:
        raise ValueError("want / avoid: the tagged scan runs whole (no phases)")
    value, mask = _tag_words(want, avoid, nq, q.device)
    desc = index.desc_for(k)
    need = lib.lmi_scan_tagged_workspace_bytes(C.byref(desc), nq, R, k, qmode)
    if need == 0 and nq:
        raise ValueError("want: this index or call takes no tagged scan "
                         "(k > 16, the split mode or a sub-cluster layout)")
    if out is None:
        out_d = torch.empty((nq, R, k), dtype=torch.float32, device=index.device)
        out_pos = torch.empty((nq, R, k), dtype=torch.int32, device=index.device)
        status = torch.zeros((1,), dtype=torch.int32, device=index.device)
    else:
        out_d, out_pos, status = out
    if ws is None:
        ws = index._ws.get("buf")
        if ws is None or ws.numel() < need:
            ws = index._ws["buf"] = torch.empty(max(need, 256), dtype=torch.uint8, device=index.device)
    else:
        _workspace(ws, need, "tagged scan")
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_bucket_topk_masked", lib.lmi_bucket_topk_masked(
        C.byref(desc), ptr(index.tags), ptr(value), ptr(mask), None, None, ptr(q), nq, q.stride(0), ptr(classes),
        R, k, qmode, ptr(out_d), ptr(out_pos), ptr(status), ptr(ws), ws.numel(), s))
    return out_d, out_pos, status


def check_range_index(index: DeviceIndex, dist: str = "f32") -> None:
    """What a range search refuses about the index, as a ValueError before
    anything is launched or allocated: the split mode (storage "f32x"), float64
    rows (corpus64), a sub-cluster layout, a stripe of a sharded index, and in
    float64 a width the float64 search does not take, and in either
    arithmetic a width whose query tile the collect scan cannot stage
    (lmi_range_workspace_bytes answers 0: d_pad > 1248)."""
    if index.storage == "f32x":
        raise ValueError("range search is not offered on storage 'f32x' (the split mode)")
    check_i8(index, "range search")
    if index.corpus64 is not None:
        raise ValueError("range search is not offered on an index that keeps float64 rows (corpus64)")
    if index.chunk_centroid is not None:
        raise ValueError("range search is not offered on a sub-cluster layout")
    if index.world > 1:
        raise ValueError("range search is not offered on a stripe of a sharded index (world > 1)")
    if dist == "f64" and index.d > 1024:
        raise ValueError(f"range search in float64 takes d <= 1024, not {index.d}")
    # either arithmetic the storage can run in (a stale fp16 check falls back to fp32 math)
    lib = _lib.load()
    for qmode in ((_lib.LMI_Q_F16, _lib.LMI_Q_F32) if index.storage == "f16" else (_lib.LMI_Q_F32,)):
        if lib.lmi_range_workspace_bytes(C.byref(index.desc), 1, 1, qmode, 0, 1) == 0:
            raise ValueError(f"range search takes no d_pad = {index.d_pad}: the collect scan's query tile "
                             "exceeds the LDS of a workgroup (d_pad <= 1248)")


def bucket_range(index: DeviceIndex, q: torch.Tensor, classes: torch.Tensor, radius, *,
                 qmode: Optional[int] = None, pair_cap: int = 256, want=None, avoid=None, stream=None,
                 ws=None, f64: bool = False):
    """K11's collect scan on one shard (lmi_bucket_range): per (query, probe)
    pair every row of the probed bucket with d <= radius[q], d the float32
    distance of the top-k lists of the same kernel family (inclusive).  Returns
    (count int32 [nq, R], cand int64 [nq, R, pair_cap], status int32 tensor) on
    the device: count is exact whatever pair_cap; cand holds the first
    min(count, pair_cap) hits to arrive, unsorted, as the bits of
    (distance ordinal << 32 | shard-local row).  `radius`: a number or float32
    values [nq] (the scan's bound as it stands).  `want` (a tagged index; a
    device int32 [nq] tensor of want words, see want_words): only rows with
    (tag & want) == want; `avoid` (the same form): and (tag & avoid) == 0, as
    bucket_topk takes the two.  `f64`: scan with the float64 mode's descriptor
    (desc_for(k, f64=True): low-norm rows with their true norm).  A bucket that
    a query's classes row names twice is collected twice.  `ws` as bucket_topk."""
    lib = _lib.load()
    check_range_index(index)
    if not 1 <= int(pair_cap) <= 1 << 24:
        raise ValueError("pair_cap must lie in [1, 2^24]")
    tagged = want is not None or avoid is not None
    if tagged and index.tags is None:
        raise ValueError("want / avoid: this index is untagged (build it with `tags`)")
    q = _rows_f32(q, index.device)
    classes = _as_torch(classes, index.device, torch.int32)
    nq, R = classes.shape
    if q.shape[0] != nq or q.shape[1] != index.d:
        raise ValueError("query shape does not match the index")
    value, mask = _tag_words(want, avoid, nq, q.device) if tagged else (None, None)
    if isinstance(radius, torch.Tensor):
        bound = radius.to(device=index.device, dtype=torch.float32).contiguous()
    else:
        bound = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(
            np.asarray(radius, dtype=np.float32), (nq,)))).to(index.device)
    if bound.shape != (nq,) or bool(torch.isnan(bound).any()):
        raise ValueError(f"radius must be a number or [{nq}] values, none NaN")
    if qmode is None:
        qmode = _lib.LMI_Q_F16 if index.storage == "f16" else _lib.LMI_Q_F32
    desc = index.desc_for(1, f64=f64)
    need = lib.lmi_range_workspace_bytes(C.byref(desc), nq, R, qmode, int(tagged), int(pair_cap))
    if need == 0:
        raise ValueError("range search: this index or call takes no range scan")
    if ws is None:
        ws = index._ws.get("range")
        if ws is None or ws.numel() < need:
            ws = index._ws["range"] = torch.empty(max(need, 256), dtype=torch.uint8, device=index.device)
    else:
        _workspace(ws, need, "range scan")
    count = torch.empty((nq, R), dtype=torch.int32, device=index.device)
    cand = torch.empty((nq, R, int(pair_cap)), dtype=torch.int64, device=index.device)
    status = torch.zeros((1,), dtype=torch.int32, device=index.device)
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_bucket_range_masked", lib.lmi_bucket_range_masked(
        C.byref(desc), ptr(index.tags) if tagged else None, ptr(value), ptr(mask), None, None, ptr(q), nq,
        q.stride(0), ptr(classes), R, qmode, ptr(bound), int(pair_cap), ptr(cand), ptr(count), ptr(status),
        ptr(ws), ws.numel(), s))
    return count, cand, status


def range_rescore_f64(index: DeviceIndex, q: torch.Tensor, radius64: torch.Tensor, count: torch.Tensor,
                      cand: torch.Tensor, stream=None):
    """Float64 distances of bucket_range's stored candidates
    (lmi_range_rescore_f64: the bits lmi_bucket_topk_f64 gives each (query,
    row)).  Returns (d64 float64 [nq, R, pair_cap], kept int32 [nq, R]), kept =
    the candidates with d64 <= radius64[q]; pairs with count > pair_cap are left
    out (kept 0).  q: the float32 queries; radius64: device float64 [nq]."""
    lib = _lib.load()
    nq, R, cap = cand.shape
    d64 = torch.empty((nq, R, cap), dtype=torch.float64, device=index.device)
    kept = torch.empty((nq, R), dtype=torch.int32, device=index.device)
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_range_rescore_f64", lib.lmi_range_rescore_f64(
        C.byref(index.desc_for(1, f64=True)), ptr(q), nq, q.stride(0), R, ptr(radius64), cap, ptr(cand),
        ptr(count), ptr(d64), ptr(kept), s))
    return d64, kept


RERANK_MAX = _lib.LMI_MAX_K  # the longest list a re-rank takes (the 8-bit scan's longest)


def check_rerank(index: DeviceIndex, rerank, k_list: int, dist: str) -> None:
    """What Searcher.lists / search(..., rerank=k2) refuse, as a ValueError
    before anything is launched: an index that is not of storage "i8" or keeps
    no fp16 rows, dist="f32" (the re-ranked distances are float64), and k2
    outside (k_list, 16]."""
    if isinstance(rerank, bool) or not isinstance(rerank, (int, np.integer)):
        raise ValueError("rerank must be an integer (the entries of the 8-bit lists to re-rank)")
    if getattr(index, "storage", None) != "i8":
        raise ValueError(f"rerank: re-ranking is for storage 'i8', not {getattr(index, 'storage', None)!r}")
    if getattr(index, "rows16", None) is None:
        raise ValueError("rerank: this index keeps no fp16 rows (build it with keep_rows=True)")
    if dist != "f64":
        raise ValueError("rerank: the re-ranked distances are float64 (dist='f64'), not dist='f32'")
    if not k_list < int(rerank) <= RERANK_MAX:
        raise ValueError(f"rerank = {int(rerank)} must lie in (k_list, {RERANK_MAX}] = ({k_list}, {RERANK_MAX}]")


def rerank_f64(index: DeviceIndex, q: torch.Tensor, pos: torch.Tensor, k: int, stream=None, out=None):
    """Exact float64 distances for short candidate lists (lmi_rerank_f64): for
    every (query, probe) the k smallest of pos's live candidates by (d64,
    position), padded (+inf, -1); d64 from the index's kept fp16 rows (`rows16`;
    an index of storage "f16" serves from its corpus), with the bits
    lmi_bucket_topk_f64 gives that (query, row).  q: the float32 queries [nq, d];
    pos: device int32 [nq, R, k_in] positions (bucket_topk's), -1 = empty
    anywhere, 1 <= k <= k_in <= 16.  Returns (d float64 [nq, R, k], pos int32
    [nq, R, k], status int32 tensor); `out`: such a triple to write into (the
    status word is OR-ed into).  A position past the index's rows is skipped
    and raises LMI_STATUS_INTERNAL in the status."""
    lib = _lib.load()
    if index.storage == "f16" and index.world == 1 and index.chunk_centroid is None:
        desc = index.desc
    else:
        desc = index.rows_desc
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32 or pos.dim() != 3:
        raise ValueError("rerank_f64: pos must be an int32 tensor [nq, R, k_in]")
    nq, R, k_in = (int(v) for v in pos.shape)
    if not 1 <= int(k) <= k_in <= RERANK_MAX:
        raise ValueError(f"rerank_f64: need 1 <= k <= k_in <= {RERANK_MAX}, not k={k}, k_in={k_in}")
    q = _rows_f32(q, index.device)  # (float64 queries are rounded, as the 8-bit scan rounds them)
    if q.shape[0] != nq or q.shape[1] != index.d:
        raise ValueError("rerank_f64: query shape does not match the lists or the index")
    pos = pos.to(index.device).contiguous()
    if out is None:
        out = (torch.empty((nq, R, int(k)), dtype=torch.float64, device=index.device),
               torch.empty((nq, R, int(k)), dtype=torch.int32, device=index.device),
               torch.zeros((1,), dtype=torch.int32, device=index.device))
    out_d, out_pos, status = out
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_rerank_f64", lib.lmi_rerank_f64(C.byref(desc), ptr(q), nq, q.stride(0), R, ptr(pos), k_in, int(k),
                                               ptr(out_d), ptr(out_pos), ptr(status), s))
    return out_d, out_pos, status


def range_pack(index: DeviceIndex, count: torch.Tensor, cand: torch.Tensor, off: torch.Tensor, out,
               d64=None, radius64=None, stream=None) -> None:
    """lmi_range_pack: every pair with count <= pair_cap writes its candidates
    (with d64 / radius64: those with d64 <= radius64[q]) to entries off[pair] ..
    of out = (d float64, pos int32, query int32), unsorted."""
    lib = _lib.load()
    nq, R, cap = cand.shape
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_range_pack", lib.lmi_range_pack(
        C.byref(index.desc), nq, R, cap, ptr(cand), ptr(count), ptr(off), ptr(d64), ptr(radius64),
        ptr(out[0]), ptr(out[1]), ptr(out[2]), s))


def bucket_topk_f64(index: DeviceIndex, q: torch.Tensor, classes: torch.Tensor, k: int,
                    qmode: Optional[int] = None, eps: Optional[float] = None, stream=None,
                    fallback_count: bool = False, out=None, ws=None, seed_round0: bool = False,
                    phases: int = 0, band_x=None):
    """K2 with float64 distances (lmi_bucket_topk_f64): the reference's
    arithmetic when either operand is not float32 (utils.py:11, :19).  Returns
    (d f64 [nq,R,k], pos [nq,R,k] int32, status int32 tensor[, n_fallback]);
    `out` and `ws` as bucket_topk.  Float64 queries whose float32 rounding
    changes them are kept for the float64 recomputation (lmi_bucket_topk_f64q;
    the scan reads them rounded).  `band_x` = (kth_send, kth_all, G): the
    band decided over G ranks (lmi_bucket_topk_f64g, ABI 10; kth_send f32
    [nq*R*k] written by the MERGE phase, kth_all f32 [G, nq*R*k] read by the
    REFINE phase, LMI_Q_PHASE_REFINE in `phases`)."""
    check_i8(index, "bucket_topk_f64 (float64 lists)")
    lib = _lib.load()
    q64 = None
    if isinstance(q, torch.Tensor) and q.dtype == torch.float64 or \
            isinstance(q, np.ndarray) and q.dtype == np.float64:
        q64 = _as_torch(q, index.device, torch.float64)
        q = q64.float()
        if torch.equal(q.double(), q64):
            q64 = None
    q = _rows_f32(q, index.device)
    classes = _as_torch(classes, index.device, torch.int32)
    nq, R = classes.shape
    if q.shape[0] != nq or q.shape[1] != index.d:
        raise ValueError("query shape does not match the index")
    if qmode is None:
        qmode = _lib.LMI_Q_F16 if index.storage == "f16" else _lib.LMI_Q_F32
    if eps is None:
        eps = refine_eps(index.d_pad, index.storage == "f16" and qmode == _lib.LMI_Q_F16,
                         rounded_inputs=q64 is not None or index.corpus64 is not None)
    if out is None:
        out_d = torch.empty((nq, R, k), dtype=torch.float64, device=index.device)
        out_pos = torch.empty((nq, R, k), dtype=torch.int32, device=index.device)
        status = torch.zeros((1,), dtype=torch.int32, device=index.device)
    else:
        out_d, out_pos, status = out
    desc = index.desc_for(k, f64=True)
    need = lib.lmi_scan_f64_workspace_bytes(C.byref(desc), nq, R, k, qmode)
    if ws is None:
        ws = index._ws.get("f64")
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=index.device)
            index._ws["f64"] = ws
    else:
        _workspace(ws, need, "float64 scan")
    s = stream if stream is not None else _lib.stream_handle(index.device)
    if index.storage == "f32x":
        seed_round0 = False  # (the split mode scans every pair whole)
    flags = (_lib.LMI_Q_SEED_ROUND0 if seed_round0 else 0) | phases
    if band_x is not None:
        kth_send, kth_all, G = band_x
        check("lmi_bucket_topk_f64g", lib.lmi_bucket_topk_f64g(
            C.byref(desc), ptr(q), nq, q.stride(0), ptr(q64), 0 if q64 is None else q64.stride(0),
            ptr(classes), R, k, qmode | flags, float(eps), ptr(kth_send), ptr(kth_all), int(G),
            nq * R * k, ptr(out_d), ptr(out_pos), ptr(status), ptr(ws), ws.numel(), s))
    else:
        check("lmi_bucket_topk_f64q", lib.lmi_bucket_topk_f64q(
            C.byref(desc), ptr(q), nq, q.stride(0), ptr(q64), 0 if q64 is None else q64.stride(0),
            ptr(classes), R, k, qmode | flags, float(eps), ptr(out_d), ptr(out_pos), ptr(status),
            ptr(ws), ws.numel(), s))
    if not fallback_count:
        return out_d, out_pos, status
    n = C.c_int32(0)
    check("lmi_refine_fallback_count", lib.lmi_refine_fallback_count(
        ptr(ws), C.byref(desc), nq, R, k, qmode, C.byref(n), s))
    return out_d, out_pos, status, int(n.value)


def split_sample_fallback_count(index: DeviceIndex, nq: int, R: int, k: int, ws=None,
                                f64: bool = False, stream=None) -> int:
    """The split mode (k <= 10, ABI 13): how many pairs of the last call on
    this workspace (`ws`, else the index's own: bucket_topk's, or
    bucket_topk_f64's with f64=True) had a band reaching their skipped
    sample's k-th and were scored over the sample rows and candidates
    (lmi_split_sample_fallback_count)."""
    lib = _lib.load()
    if ws is None:
        ws = index._ws.get("f64" if f64 else "buf")
    n = C.c_int32(0)
    s = stream if stream is not None else _lib.stream_handle(index.device)
    check("lmi_split_sample_fallback_count", lib.lmi_split_sample_fallback_count(
        ptr(ws), C.byref(index.desc_for(k)), nq, R, k, C.byref(n), s))
    return int(n.value)


def global_band(index: DeviceIndex, nq: int, R: int, k: int, qmode: int) -> bool:
    """True when the float64 search of a striped index can decide its band
    over every rank's lists (lmi_f64_global_band: the band lists, k <= 10 on
    the fp16 scan, no split mode); LMI_F64_LOCAL_BAND=1 turns it off (every
    rank refines the band of its own list, the round-5 form)."""
    if os.environ.get("LMI_F64_LOCAL_BAND") == "1":
        return False
    return bool(_lib.load().lmi_f64_global_band(C.byref(index.desc_for(k)), nq, R, k, qmode))


def merge_topk(d_in: torch.Tensor, pos_in: torch.Tensor, k: int, stream=None):
    """K3: merge [G, rows, k] lists -> [rows, k] by (distance, global position);
    float32 (lmi_merge_topk) or float64 (lmi_merge_topk_f64) distances."""
    G = d_in.shape[0]
    rows = d_in[0].numel() // k
    f64 = d_in.dtype == torch.float64
    out_d = torch.empty(d_in.shape[1:], dtype=d_in.dtype, device=d_in.device)
    out_pos = torch.empty(d_in.shape[1:], dtype=torch.int32, device=d_in.device)
    s = stream if stream is not None else _lib.stream_handle(d_in.device)
    fn = "lmi_merge_topk_f64" if f64 else "lmi_merge_topk"
    check(fn, getattr(_lib.load(), fn)(ptr(d_in.contiguous()), ptr(pos_in.contiguous()), G, rows, k,
                                       ptr(out_d), ptr(out_pos), s))
    return out_d, out_pos


def replay(classes: np.ndarray, lists_d: np.ndarray, lists_pos: np.ndarray, *, k_round: int,
           k_final: int, bucket_size: np.ndarray, pos_to_id: np.ndarray, use_threshold: bool,
           thr_round0: Optional[np.ndarray] = None):
    """A5 on the host (lmi_replay, or lmi_replay_f64 for float64 lists):
    per-(query, probe) lists -> reference output."""
    classes = np.ascontiguousarray(classes, dtype=np.int32)
    if classes.ndim == 1:
        classes = classes[:, None]
    nq, R = classes.shape
    f64 = np.asarray(lists_d).dtype == np.float64
    lists_d = np.ascontiguousarray(lists_d, dtype=np.float64 if f64 else np.float32).reshape(nq, R, -1)
    lists_pos = np.ascontiguousarray(lists_pos, dtype=np.int32).reshape(nq, R, -1)
    k_list = lists_d.shape[2]
    bucket_size = np.ascontiguousarray(bucket_size, dtype=np.int64)
    pos_to_id = np.ascontiguousarray(pos_to_id, dtype=np.int64)
    w = k_round if R == 1 else k_final
    dists = np.empty((nq, w), np.float64)
    anns = np.empty((nq, w), np.uint32)
    thr = None
    if thr_round0 is not None:
        thr = np.ascontiguousarray(np.asarray(thr_round0, dtype=np.float64).ravel())
        if thr.shape != (nq,):
            raise ValueError("threshold_dist must have one value per query")
    w_out = C.c_int32(0)
    fn = "lmi_replay_f64" if f64 else "lmi_replay"
    check(fn, getattr(_lib.load(), fn)(
        classes.ctypes.data, nq, R, k_list, lists_d.ctypes.data, lists_pos.ctypes.data,
        k_round, k_final, bucket_size.ctypes.data, bucket_size.size, pos_to_id.ctypes.data,
        pos_to_id.size, int(bool(use_threshold)), ptr(thr), dists.ctypes.data, anns.ctypes.data,
        C.byref(w_out)))
    return dists, anns


def replay_device(classes: torch.Tensor, lists_d: torch.Tensor, lists_pos: torch.Tensor, *,
                  k_round: int, k_final: int, bucket_size: torch.Tensor, pos_to_id: torch.Tensor,
                  use_threshold: bool, thr_round0: Optional[torch.Tensor] = None, stream=None,
                  out=None, phases: int = 3, ws: Optional[torch.Tensor] = None,
                  k_list: Optional[int] = None):
    """A5 on the device (lmi_replay_device_phase; float32 or float64 lists):
    same results as `replay`, device tensors in and out: (dists f64 [nq, w],
    anns uint32-as-int32 [nq, w], status); `out` = such a triple to write into
    (the status word zeroed by the caller, or by a GROUPS phase).  `phases`:
    LMI_REPLAY_PHASE_GROUPS (classes only: lists_d / lists_pos may be None,
    then give `k_list`, the lists' width, and float32 is assumed for sizing),
    LMI_REPLAY_PHASE_ROUNDS, or both (3); the calls of one replay share `ws`
    (a caller-owned uint8 workspace; default: a new one per call)."""
    lib = _lib.load()
    dev = classes.device if lists_d is None else lists_d.device
    classes = _as_torch(classes, dev, torch.int32)
    if classes.dim() == 1:
        classes = classes[:, None].contiguous()
    nq, R = classes.shape
    f64 = lists_d is not None and lists_d.dtype == torch.float64
    if lists_d is not None:
        lists_d = _as_torch(lists_d, dev, torch.float64 if f64 else torch.float32).reshape(nq, R, -1).contiguous()
        lists_pos = _as_torch(lists_pos, dev, torch.int32).reshape(nq, R, -1).contiguous()
        k_list = lists_d.shape[2]
    w = k_round if R == 1 else k_final
    if out is None:
        dists = torch.empty((nq, w), dtype=torch.float64, device=dev)
        anns = torch.empty((nq, w), dtype=torch.int32, device=dev)  # uint32 bits
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    else:
        dists, anns, status = out
    n_b = int(bucket_size.numel())
    need = lib.lmi_replay_device_workspace_bytes(nq, R, k_list, k_round, k_final, n_b)
    if ws is None:
        ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    else:
        _workspace(ws, need, "replay")
    thr = None
    if thr_round0 is not None:
        thr = _as_torch(thr_round0, dev, torch.float64).reshape(-1)
        if thr.numel() != nq:
            raise ValueError("threshold_dist must have one value per query")
    s = stream if stream is not None else _lib.stream_handle(dev)
    check("lmi_replay_device_phase", lib.lmi_replay_device_phase(
        int(phases), int(f64), ptr(classes), nq, R, k_list, ptr(lists_d), ptr(lists_pos), k_round,
        k_final, ptr(bucket_size), n_b, ptr(pos_to_id), int(pos_to_id.numel()),
        int(bool(use_threshold)), ptr(thr), ptr(dists), ptr(anns), ptr(status), ptr(ws), ws.numel(), s))
    return dists, anns, status


def answer_buffer(nq: int, w: int, device):
    """The step's answer in ONE device buffer, so it crosses PCIe in one copy:
    int32 words [dists f64 nq*w (2 words each)][anns uint32 nq*w][scan status,
    replay status] -> (buf, dists [nq, w], anns [nq, w], status words [2],
    zeroed)."""
    n = nq * w
    buf = torch.empty((3 * n + 2,), dtype=torch.int32, device=device)
    st = buf[3 * n:]
    st.zero_()
    return buf, buf[:2 * n].view(torch.float64).view(nq, w), buf[2 * n:3 * n].view(nq, w), st


def answer_views(h: torch.Tensor, nq: int, w: int):
    """numpy views of an answer buffer copied to the host:
    (dists f64 [nq, w], anns uint32 [nq, w], scan status, replay status)."""
    a = h.numpy()
    n = nq * w
    return (a[:2 * n].view(np.float64).reshape(nq, w), a[2 * n:3 * n].view(np.uint32).reshape(nq, w),
            int(a[3 * n]), int(a[3 * n + 1]))


class Searcher:
    """Runs the whole hot path for one shard set (one process per GPU).

    ``search`` times like search.py:116-141 (router + scan + merge + replay)."""

    def __init__(self, index: DeviceIndex, router: DeviceRouter, group=None,
                 exchange: Optional[bool] = None):
        """`exchange`: run the list exchange (route_sharded, K2 into the packed
        send buffer, the all-gather, lmi_merge_topk_packed) over the process
        group.  None (default): when a group is initialised and the index is
        a stripe of a G > 1 index, or LMI_FORCE_EXCHANGE=1
        (li.dist.force_exchange: a one-rank RCCL group then takes the G > 1
        branch of every step form, so the exchange runs on one GPU exactly as
        on eight).  A whole index (index.world == 1) under a group of several
        ranks answers on its own: every rank holds every row, K3 does not
        deduplicate, and gathering G copies of the same lists would repeat
        each object G times -- asking for that exchange is a ValueError."""
        import torch.distributed as tdist
        from .dist import force_exchange
        self.index = index
        self.router = router
        self.group = group
        grouped = tdist.is_available() and tdist.is_initialized()
        if exchange is None:
            exchange = grouped and (index.world > 1 or force_exchange())
        if exchange:
            check_i8(index, "the list exchange over a process group")
        if exchange and not grouped:
            raise ValueError("the list exchange needs an initialised process group")
        if exchange and index.world == 1 and tdist.get_world_size(group) > 1:
            raise ValueError("the list exchange over a group of several ranks needs a striped "
                             "index (world > 1): every rank of a whole index returns the same "
                             "lists, and the merge would repeat each object once per rank")
        self.exchange = bool(exchange)
        self._pinned = {}
        self._qcheck = None

    def with_index(self, index: DeviceIndex) -> "Searcher":
        """A Searcher over `index` (e.g. the result of DeviceIndex.add /
        remove) with this one's router and group; its device tables are its
        own, so this Searcher keeps answering from its own index -- unless the
        update was made in place: this Searcher's index is then consumed and
        every search on it raises RuntimeError."""
        return Searcher(index, self.router, self.group, exchange=self.exchange)

    def _host(self, name, shape, dtype):
        buf = self._pinned.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            buf = torch.empty(shape, dtype=dtype, pin_memory=torch.cuda.is_available())
            self._pinned[name] = buf
        return buf

    def qmode(self, q_search: torch.Tensor) -> int:
        """The scan's query path, decided before the scan: LMI_Q_F16 (exact
        fp16 MFMA products) when the corpus is stored fp16 and every query
        value is fp16-representable, else LMI_Q_F32 (exact fp32 MFMA).  The
        check is one device reduction, run once per query batch (cached by the
        tensor's storage, shape and version counter); every rank holds the same
        batch, so every rank decides the same."""
        if self.index.storage == "i8":
            return _lib.LMI_Q_I8  # (the queries are quantised inside the call)
        if self.index.storage != "f16":
            return _lib.LMI_Q_F32
        import weakref
        q = q_search
        # keyed by the live tensor object (a weak reference) and its version
        # counter: a new tensor that reuses a freed one's memory, or the same
        # tensor written in place, is checked again
        key = (q.data_ptr(), q._version, tuple(q.shape), q.stride(), q.dtype, q.device)
        if self._qcheck is not None and self._qcheck[0] == key and self._qcheck[2]() is q:
            return self._qcheck[1]
        mode = _lib.LMI_Q_F16 if fp16_exact(q) else _lib.LMI_Q_F32
        self._qcheck = (key, mode, weakref.ref(q))
        return mode

    def _scan(self, q_search, classes, k_list: int, qmode: int, f64: bool, lap=None,
              status_out=None, ws=None, seed_round0: bool = False, want=None, rerank=None):
        """K2 on this shard (+ all-gather and K3 for G > 1 ranks, the status
        words riding along so every rank sees every rank's bits).  `lap`
        (measurement only) is called after the scan and after the exchange.
        `status_out` (a zeroed device int32 word): the status lands there.
        `ws`: a caller-owned scan workspace (GraphedSearch's).  `want`: the
        want words of a filtered scan (want_words; float32 lists only).
        `rerank` (checked by check_rerank; f64, one GPU): the 8-bit scan keeps
        `rerank` entries a pair and rerank_f64 cuts them to k_list float64 ones."""
        if rerank is not None:
            st = status_out if status_out is not None else torch.zeros((1,), dtype=torch.int32,
                                                                       device=self.index.device)
            nq, R = classes.shape
            scan_out = (torch.empty((nq, R, rerank), dtype=torch.float32, device=self.index.device),
                        torch.empty((nq, R, rerank), dtype=torch.int32, device=self.index.device), st)
            # (the over-fetch runs on the ring's 16-entry lists where the plan has them)
            _, pos2, _ = bucket_topk(self.index, q_search, classes, rerank, qmode=qmode, out=scan_out, ws=ws,
                                     want=want, lists16=True)
            if lap:
                lap("scan")
            d, pos, status = rerank_f64(self.index, q_search, pos2, k_list, out=(
                torch.empty((nq, R, k_list), dtype=torch.float64, device=self.index.device),
                torch.empty((nq, R, k_list), dtype=torch.int32, device=self.index.device), st))
            if lap:
                lap("rerank")
            return d, pos, status
        out = None
        if not self.exchange and status_out is not None:
            nq, R = classes.shape
            dev = self.index.device
            out = (torch.empty((nq, R, k_list), dtype=torch.float64 if f64 else torch.float32,
                               device=dev),
                   torch.empty((nq, R, k_list), dtype=torch.int32, device=dev), status_out)
        if self.exchange:
            # the lists and the status word land in this rank's slice of the
            # all-gather's packed send buffer (li.dist.packed_lists)
            from .dist import packed_lists
            nq, R = classes.shape
            buf, dv, pv, sv = packed_lists(nq * R, k_list, f64, self.index.device)
            out = (dv.view(nq, R, k_list), pv.view(nq, R, k_list), sv)
        if f64 and self.exchange and global_band(self.index, nq, R, k_list, qmode):
            # the band decided over every rank's lists (ABI 10): the ranks'
            # k smallest d32 per pair are all-gathered between the chunk merge
            # and the float64 refinement, so each rank refines only its own
            # rows of the merged band
            from .dist import _all_gather
            G = torch.distributed.get_world_size(self.group)
            kth = torch.empty((nq * R * k_list,), dtype=torch.float32, device=q_search.device)
            kall = torch.empty((G, nq * R * k_list), dtype=torch.float32, device=q_search.device)
            ph = _lib.LMI_Q_PHASE_PLAN | _lib.LMI_Q_PHASE_SCAN | _lib.LMI_Q_PHASE_MERGE
            bucket_topk_f64(self.index, q_search, classes, k_list, qmode=qmode, out=out, ws=ws,
                            seed_round0=seed_round0, phases=ph, band_x=(kth, None, G))
            _all_gather(kall.view(-1), kth, self.group)
            d, pos, status = bucket_topk_f64(self.index, q_search, classes, k_list, qmode=qmode,
                                             out=out, ws=ws, seed_round0=seed_round0,
                                             phases=_lib.LMI_Q_PHASE_REFINE, band_x=(None, kall, G))
        elif f64:
            d, pos, status = bucket_topk_f64(self.index, q_search, classes, k_list, qmode=qmode,
                                             out=out, ws=ws, seed_round0=seed_round0)
        else:
            d, pos, status = bucket_topk(self.index, q_search, classes, k_list, qmode=qmode, out=out,
                                         ws=ws, seed_round0=seed_round0, want=want)
        if lap:
            lap("scan")
        if self.exchange:
            from .dist import gather_merge_packed
            d, pos, status = gather_merge_packed(buf, nq * R, k_list, f64, self.group,
                                                 status_out=status_out)
            d, pos = d.view(nq, R, k_list), pos.view(nq, R, k_list)
            if lap:
                lap("allgather")
        return d, pos, status

    def lists(self, q_nav: torch.Tensor, q_search: torch.Tensor, R: int, k_list: int,
              classes: Optional[torch.Tensor] = None, dist: str = "f32", stop_mass=None,
              min_probes: int = 1, want=None, avoid=None, rerank: Optional[int] = None):
        """Device part: router + scan (+ RCCL merge).  Returns device tensors.
        `rerank` = k2 (an index of storage "i8" with keep_rows, dist="f64",
        k_list < k2 <= 16): the 8-bit scan keeps k2 entries a pair and their
        float64 distances from the kept fp16 rows decide the k_list returned
        (rerank_f64) -- exact distances on an approximate candidate set; with
        `want` / `avoid` the k2 candidates are eligible rows.  ValueError
        (check_rerank) before anything is launched otherwise.
        `stop_mass`, `min_probes`: the router's stop rule (DeviceRouter.topr);
        a dropped probe's list is (+inf, -1).  `want` (a tagged index; an int
        or an integer array [nq], words in [0, 2^32)): filtered lists -- each
        the exact top-k_list of the bucket's rows with (tag & want) == want,
        padded (+inf, -1); the lists of an index built from those rows alone.
        `avoid` (the same forms; alone it means want = 0): and only rows with
        (tag & avoid) == 0.  A query that wants and avoids one bit is a
        ValueError, like every refusal of `want`, before anything is launched."""
        check_stop(stop_mass, min_probes)
        self.index._check_live()
        self._check_i8_lists(k_list, dist, rerank)
        if want is not None or avoid is not None:
            nq = int(q_search.shape[0]) if classes is None else int(classes.shape[0])
            # (re-ranked: the filtered scan is the float32 one of `rerank` entries)
            want = filter_words(self.index, want, avoid, nq, *((k_list, dist) if rerank is None else
                                                               (int(rerank), "f32")))
        if classes is None:
            classes = self.route(q_nav, R, stop_mass=stop_mass, min_probes=min_probes)
        q_search = _rows_q(q_search, self.index.device)
        d, pos, status = self._scan(q_search, classes, k_list, self.qmode(q_search), dist == "f64",
                                    want=want, rerank=None if rerank is None else int(rerank))
        return classes, d, pos, status

    def _check_i8_lists(self, k_list: int, dist: str, rerank=None) -> None:
        """The lists an index of storage "i8" answers: float32, at most
        LMI_MAX_K entries -- or, with `rerank`, float64 ones re-ranked from its
        kept fp16 rows (check_rerank, on any index); ValueError otherwise,
        before anything is launched."""
        if rerank is not None:
            check_rerank(self.index, rerank, k_list, dist)
            return
        if self.index.storage == "i8":
            if dist != "f32":
                check_i8(self.index, "dist='f64' (float64 lists)")
            if k_list > _lib.LMI_MAX_K:
                check_i8(self.index, f"k_list = {k_list} > {_lib.LMI_MAX_K}")

    def route(self, q_nav, R: int, stop_mass=None, min_probes: int = 1) -> torch.Tensor:
        """K1 classes [nq, R]; with G > 1 ranks each routes nq/G queries and
        the classes are all-gathered (li.dist.route_sharded).  `stop_mass`,
        `min_probes`: the stop rule of DeviceRouter.topr (dropped probes are
        -1; the rule is per query, so sharding the queries does not change it)."""
        check_stop(stop_mass, min_probes)
        if self.exchange:
            from .dist import route_sharded
            return route_sharded(self.router, _rows_f32(q_nav, self.index.device), R, self.group,
                                 stop_mass=stop_mass, min_probes=min_probes)
        if stop_mass is None:
            return self.router.topr(q_nav, R)[0]
        return self.router.topr(q_nav, R, stop_mass=stop_mass, min_probes=min_probes)[0]

    def eligible_bucket_size(self, want: int, avoid: int = 0) -> np.ndarray:
        """The eligible rows of every bucket of the whole index under the words
        `want` and `avoid` (eligible_counts, cached per pair until the index's
        tags are edited: DeviceIndex.tags_version): the reference replay's
        bucket_size of a filtered search."""
        version = self.index.tags_version
        if self.__dict__.get("_eligible_version") != version:
            self._eligible, self._eligible_version = {}, version
        key = (int(want), int(avoid))
        if key not in self._eligible:
            self._eligible[key] = eligible_counts(self.index.tags_by_pos, self.index.layout.bucket_off,
                                                  key[0], key[1])
        return self._eligible[key]

    def _device_tables(self):
        """bucket sizes and position -> id map in HBM for the device replay."""
        t = getattr(self, "_dev_tables", None)
        if t is None:
            dev = self.index.device
            t = (torch.from_numpy(np.ascontiguousarray(self.index.bucket_size, dtype=np.int64)).to(dev),
                 torch.from_numpy(np.ascontiguousarray(self.index.pos_to_id, dtype=np.int64)).to(dev))
            self._dev_tables = t
        return t

    def range_search(self, q_nav, q_search, R: int, radius, *, classes: Optional[torch.Tensor] = None,
                     dist: str = "f32", stop_mass=None, min_probes: int = 1, want=None, avoid=None,
                     pair_cap: int = 256, timings: Optional[dict] = None):
        """Every object of each query's probed buckets within `radius` of it
        (K11) -> host arrays (lims int64 [nq + 1], dists float64 [total], anns
        uint32 [total]): query i owns entries lims[i]:lims[i + 1], ordered by
        (distance, global position); the comparison d <= radius is inclusive.

        `radius`: a number or one value per query.  The probed buckets are the
        router's top-R, cut short by `stop_mass` / `min_probes` as in search, or
        the caller's `classes` [nq, R] (-1: no probe).  A classes row that
        names a bucket twice returns that bucket's objects twice (nothing is
        de-duplicated).  dist="f32": d is the scan's float32 distance -- the
        value a top-k list of the same kernel family holds for that (query,
        object) -- and the radius is rounded once to float32.  dist="f64": d is
        the float64 distance of search(dist="f64") (lmi_bucket_topk_f64), the
        radius float64; the scan collects under float32(radius + 2 eps), eps =
        refine_eps, and the candidates are re-scored in float64.  `want` (a
        tagged index; an int or one word per query): only objects with
        (tag & want) == want answer; `avoid` (the same forms; alone it means
        want = 0): and only objects with (tag & avoid) == 0.

        `pair_cap`: candidate slots per (query, probe) of the first scan.  The
        counts are exact whatever it is; if a pair's count exceeds it, one more
        scan runs over those pairs alone with the largest count as its cap, so
        the result does not depend on pair_cap.  Memory: the first scan holds
        nq * R * pair_cap keys of 8 bytes.  The second scan's buffer is dense
        too, nq * R * cmax keys with cmax the largest count of any pair
        (twice that in float64, for the re-scored distances, and once more in
        the workspace at d = 768), although only the overflowed pairs use it:
        nothing compacts them, so one large bucket under a wide radius sets the
        footprint of the whole batch (40 000 pairs with cmax = 80 000: 25.6 GB
        of keys).  Split such a batch, or the radius, on the caller's side.
        `timings` (measurement only;
        the stages are then separated by stream synchronisations) receives
        per-stage times in ms, `scans` (1 or 2), `results`, and `fp32_redo`
        = 1 when the scan found the cached fp16 check stale and the call was
        redone with exact fp32 MFMA.

        ValueError before anything is launched on: a radius that is NaN or
        not [nq]; storage "f32x"; an index with float64 rows; float64 queries
        that float32 rounding changes; a sub-cluster layout; a striped index
        or a Searcher with an exchange group; `want` or `avoid` on an untagged
        index, or sharing a bit; in
        float64 d > 1024; in either arithmetic d_pad > 1248 (the collect
        scan's query tile would not fit a workgroup's LDS)."""
        import time
        check_stop(stop_mass, min_probes)
        ix = self.index
        ix._check_live()
        if dist not in ("f32", "f64"):
            raise ValueError("dist must be 'f32' or 'f64'")
        f64 = dist == "f64"
        check_range_index(ix, dist)
        if self.exchange:
            raise ValueError("range search is not offered on a Searcher with an exchange group")
        if not 1 <= int(pair_cap) <= 1 << 24:
            raise ValueError("pair_cap must lie in [1, 2^24]")
        nq = int(q_search.shape[0]) if classes is None else int(classes.shape[0])
        r64 = np.asarray(radius.cpu() if isinstance(radius, torch.Tensor) else radius, dtype=np.float64)
        if r64.ndim == 0:
            r64 = np.full(nq, float(r64))
        if r64.shape != (nq,) or np.isnan(r64).any():
            raise ValueError(f"radius must be a number or [{nq}] values, none NaN")
        want_w = filter_words(ix, want, avoid, nq, 1, "f32")
        dev = ix.device
        q64 = (isinstance(q_search, torch.Tensor) and q_search.dtype == torch.float64) or \
            (isinstance(q_search, np.ndarray) and q_search.dtype == np.float64)
        q_search = _rows_q(q_search, dev)
        if q64:
            if not torch.equal(q_search.float().double(), q_search):
                raise ValueError("range search takes float64 queries only where float32 holds their values")
            q_search = q_search.float()
        sync = (lambda: torch.cuda.current_stream(dev).synchronize()) if timings is not None else None
        tl = [time.perf_counter()]

        def lap(name):
            if sync:
                sync()
                t1 = time.perf_counter()
                timings[name] = timings.get(name, 0.0) + (t1 - tl[0]) * 1e3
                tl[0] = t1

        if nq == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.float64), np.zeros(0, np.uint32)
        qmode = self.qmode(q_search)
        if classes is None:
            classes = self.route(q_nav, R, stop_mass=stop_mass, min_probes=min_probes)
        classes = _as_torch(classes, dev, torch.int32)
        lap("router")
        r_dev = torch.from_numpy(r64).to(dev) if f64 else None

        def scan_bound(mode):
            """The scan's float32 bound under `mode`'s arithmetic: the radius
            rounded once, in float64 float32(r + 2 eps) rounded up."""
            if not f64:
                b32 = r64.astype(np.float32)
            else:
                eps = refine_eps(ix.d_pad, ix.storage == "f16" and mode == _lib.LMI_Q_F16)
                wide = r64 + 2.0 * eps
                b32 = wide.astype(np.float32)
                b32 = np.where(b32.astype(np.float64) < wide, np.nextafter(b32, np.float32(np.inf)), b32)
            return torch.from_numpy(np.ascontiguousarray(b32, dtype=np.float32)).to(dev)

        def first_scan(mode):
            bound = scan_bound(mode)
            count, cand, status = bucket_range(ix, q_search, classes, bound, qmode=mode, pair_cap=pair_cap,
                                               want=want_w, f64=f64)
            # the one host read of the scan: the largest count, the total, the status
            head = torch.stack([count.max().long(), count.sum(), status[0].long()]).cpu()
            return bound, count, cand, int(head[0]), int(head[1]), int(head[2])

        bound, count, cand, cmax, total, st = first_scan(qmode)
        if st & _lib.LMI_STATUS_QUERY_NOT_F16:
            # the cached fp16 check was stale: redo with exact fp32 MFMA, under
            # the bound of that arithmetic (its eps is the wider one)
            qmode = _lib.LMI_Q_F32
            bound, count, cand, cmax, total, st = first_scan(qmode)
            if timings is not None:
                timings["fp32_redo"] = 1
        if st:
            raise RuntimeError(f"range_search: scan status {st}")
        scans = [(count, cand)]
        status2 = None
        if cmax > pair_cap:
            # the overflowed pairs alone, with room for the largest of them
            over = count > pair_cap
            classes2 = torch.where(over, classes, torch.full_like(classes, -1))
            count2, cand2, status2 = bucket_range(ix, q_search, classes2, bound, qmode=qmode, pair_cap=cmax,
                                                  want=want_w, f64=f64)
            scans.append((count2, cand2))
        lap("scan")

        def second_read(kept):
            """The second scan's host read: the total again and that scan's status."""
            head = torch.stack([kept.sum(), status2[0].long()]).cpu()
            if int(head[1]):
                raise RuntimeError(f"range_search: second scan status {int(head[1])}")
            return int(head[0])

        if f64:
            scored = [range_rescore_f64(ix, q_search, r_dev, c, x) for c, x in scans]
            kept = scored[0][1] if len(scored) == 1 else scored[0][1] + scored[1][1]
            total = int(kept.sum().item()) if len(scans) == 1 else second_read(kept)
            lap("rescore")
        else:
            scored = [(None, None)] * len(scans)
            # (the counts are exact whatever the cap; the entries a pack writes are
            # its own scan's)
            kept = count if len(scans) == 1 else torch.where(count > pair_cap, scans[1][0], count)
            if len(scans) == 2:
                total = second_read(kept)
        per_q = kept.sum(dim=1, dtype=torch.int64)
        lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        torch.cumsum(per_q, 0, out=lims[1:])
        flat = kept.reshape(-1).long()
        off = (torch.cumsum(flat, 0) - flat).contiguous()
        out = (torch.empty(total, dtype=torch.float64, device=dev),
               torch.empty(total, dtype=torch.int32, device=dev),
               torch.empty(total, dtype=torch.int32, device=dev))
        if total:
            for (c, x), (d64, _) in zip(scans, scored):
                range_pack(ix, c, x, off, out, d64=d64, radius64=r_dev if f64 else None)
        lap("pack")
        # (query, distance, global position): three stable sorts, last key first
        d, pos, qi = out
        if total:
            pos, o = torch.sort(pos, stable=True)
            d, qi = d[o], qi[o]
            d, o = torch.sort(d, stable=True)
            pos, qi = pos[o], qi[o]
            qi, o = torch.sort(qi, stable=True)
            d, pos = d[o], pos[o]
        _, p2id = self._device_tables()
        ids = p2id[pos.long()].to(torch.int32)
        lap("sort")
        h_lims, h_d, h_a = lims.cpu(), d.cpu(), ids.cpu()
        lap("d2h")
        if timings is not None:
            timings["scans"] = len(scans)
            timings["results"] = total
            if stop_mass is not None:
                timings["mean_probes"] = float((classes >= 0).sum().item()) / max(1, nq)
        return h_lims.numpy(), h_d.numpy(), h_a.numpy().view(np.uint32)

    def streamed(self, q_nav, q_search, R: int, k: int = 10, **kw) -> "StreamedSearch":
        """The step as a four-stage pipeline of captured graphs over a stream
        of batches (StreamedSearch); answers equal search(...) per batch."""
        check_i8(self.index, "streamed() (the batch stream)")
        from .stream import StreamedSearch
        return StreamedSearch(self, q_nav, q_search, R, k, **kw)

    def graph(self, q_nav, q_search, R: int, k: int = 10, **kw) -> "GraphedSearch":
        """The step captured as a HIP graph (GraphedSearch), from the batch in
        host memory to the answer in host memory: same results as
        search(..., semantics="reference", replay_on="device")."""
        check_i8(self.index, "graph() (the captured step)")
        from .graphed import GraphedSearch
        return GraphedSearch(self, q_nav, q_search, R, k, **kw)

    def search(self, q_nav, q_search, R: int, k: int = 10, *, k_round: int = 10,
               use_threshold: bool = True, classes: Optional[torch.Tensor] = None,
               timings: Optional[dict] = None, replay_on: str = "device",
               semantics: str = "reference", dist: str = "f32", stop_mass=None,
               min_probes: int = 1, want=None, avoid=None, rerank: Optional[int] = None):
        """Whole hot path for one batch -> (dists f64 [nq, w], anns u32 [nq, w]).

        `rerank` = k2 (an index of storage "i8" with keep_rows, dist="f64"; as
        in lists): the lists the merge or the replay reads are the k2-entry
        8-bit lists re-ranked to float64 from the kept fp16 rows; everything
        downstream runs as on float64 lists.  The scan is never seeded.

        `want` (a tagged index): filtered search -- only rows with
        (tag & want) == want answer.  semantics="exact" takes an int or an
        integer array [nq] (a word per query); semantics="reference" takes one
        int for the whole batch (its round merge couples the batch's queries)
        and answers as search() on the index built from the eligible rows
        alone: the replay reads every bucket's eligible row count as its size.
        The filtered scan is never seeded.  `avoid` (the same forms as `want`;
        alone it means want = 0): and only rows with (tag & avoid) == 0 answer
        -- "not deleted", "not flagged" (DeviceIndex.edit_tags sets such bits
        in place).  ValueError before anything is launched on an untagged
        index, with dist="f64", storage "f32x", lists of more than 16 entries,
        a malformed `want` or `avoid`, or a query that wants and avoids one bit.

        `stop_mass` (None: off): adaptive probing -- R is the cap, and each
        query stops at the first probe before which the router's probability
        mass reached stop_mass, but not before `min_probes` probes
        (DeviceRouter.topr, probe_stop_mask).  A dropped probe is a round in
        which the query matches no bucket: under the reference semantics it
        keeps the fillers for that round and the merge keeps what it had.
        Everything after the router is unchanged; the answer is that of
        search(classes=<the masked classes>).  `timings` then also receives
        `mean_probes` (read back after the answer).

        semantics="reference" (default) reproduces LearnedIndex.search's round
        merge (thresholds, fillers, the <k quirk).
        semantics="exact" returns instead the exact top-k, by (distance, id
        position), of the union of each query's R probed buckets (K3 merge of
        its R lists on the device; fewer than k objects pad with (10000, 0)),
        the option SURVEY.md §8(a) asks for beside the reference semantics.

        dist="f32": distances in float32, the reference's arithmetic when the
        corpus and the queries are both float32; dist="f64": float64 distances
        (lmi_bucket_topk_f64), its arithmetic otherwise — e.g. the real clip768
        'emb', which is float16 (utils.py:11, :19).

        replay_on="device" (default) runs the reference's round merge on the GPU
        (lmi_replay_device) and copies back only the result; "host" copies the
        lists back and runs lmi_replay (same results, the checker of the device
        replay).  `timings` (measurement only) receives per-stage wall times in
        ms; the stages are then separated by stream synchronisations."""
        import time
        check_stop(stop_mass, min_probes)
        self.index._check_live()
        if replay_on not in ("device", "host"):
            raise ValueError("replay_on must be 'device' or 'host'")
        if semantics not in ("reference", "exact"):
            raise ValueError("semantics must be 'reference' or 'exact'")
        if dist not in ("f32", "f64"):
            raise ValueError("dist must be 'f32' or 'f64'")
        k_list = k_round if semantics == "reference" else max(k_round, k)
        self._check_i8_lists(k_list, dist, rerank)
        rerank = None if rerank is None else int(rerank)
        f64 = dist == "f64"
        kmax = _lib.LMI_MAX_K_F64 if f64 else _lib.LMI_MAX_K_PASSES
        if k_list > kmax:
            raise ValueError(f"k={k_list} > {kmax}")
        if k_round > _lib.LMI_REPLAY_DEVICE_MAX_KR or k > _lib.LMI_REPLAY_DEVICE_MAX_K:
            replay_on = "host"  # the device replay holds rows of <= 32 / 64 entries
        dev = self.index.device
        want_w = None
        if want is not None or avoid is not None:
            nq_w = int(q_search.shape[0]) if classes is None else int(classes.shape[0])
            want_w = filter_words(self.index, want, avoid, nq_w, *((k_list, dist) if rerank is None else
                                                                   (rerank, "f32")),
                                  per_query=semantics == "exact")
        sync = (lambda: torch.cuda.current_stream(dev).synchronize()) if timings is not None else None

        def lap(name, t0):
            if sync:
                sync()
                t1 = time.perf_counter()
                timings[name] = timings.get(name, 0.0) + (t1 - t0) * 1e3
                return t1
            return t0

        t0 = time.perf_counter()
        q_search = _rows_q(q_search, dev)
        qmode = self.qmode(q_search)
        if classes is None:
            classes = self.route(q_nav, R, stop_mass=stop_mass, min_probes=min_probes)
        t0 = lap("router", t0)

        def done(out):
            if timings is not None and stop_mass is not None:
                timings["mean_probes"] = float((classes >= 0).sum().item()) / max(1, classes.shape[0])
            return out
        tl = [t0]

        def lap_at(name):
            tl[0] = lap(name, tl[0])

        nq = classes.shape[0]
        ans = None
        if semantics == "reference" and replay_on == "device":
            # the answer and both status words in one buffer: one D2H copy
            w_ans = k_round if classes.shape[1] == 1 else k
            ans = answer_buffer(nq, w_ans, dev)
        # (valid while the merged width k is at most the round lists' k_round:
        # the running threshold then never exceeds round 0's k-th distance;
        # with k > k_round the first merge pads with 10000s)
        seed = (semantics == "reference" and use_threshold and k <= k_round and _SEED_ROUND0
                and want_w is None)
        d, pos, status = self._scan(q_search, classes, k_list, qmode, f64, lap_at if sync else None,
                                    status_out=None if ans is None else ans[3][0:1],
                                    seed_round0=seed, want=want_w, rerank=rerank)
        # (filtered: the replay's bucket sizes are the eligible row counts)
        bsize = self.index.bucket_size
        if want_w is not None and semantics == "reference":
            bsize = self.eligible_bucket_size(int(want or 0), int(avoid or 0))
        t0 = tl[0]
        h_st = self._host("st", (2,), torch.int32)

        def check_status(st, rst=0):
            # every rank holds the OR of all ranks' scan bits (they rode the
            # all-gather) and runs the same replay: all ranks raise together
            if st & _lib.LMI_STATUS_INTERNAL or rst:
                raise RuntimeError(f"search: internal status {st}/{rst}")
            return bool(st & _lib.LMI_STATUS_QUERY_NOT_F16)

        if semantics == "exact":
            _, p2id = self._device_tables()

            def exact(d, pos):
                Rr = classes.shape[1]
                md, mp = merge_topk(d.view(nq, Rr, k_list).transpose(0, 1).contiguous(),
                                    pos.view(nq, Rr, k_list).transpose(0, 1).contiguous(), k_list)
                md, mp = md[:, :k], mp[:, :k]
                none = mp < 0
                ids = p2id[mp.clamp(min=0).long()]
                return (torch.where(none, torch.full_like(md, 10000.0), md).double(),
                        torch.where(none, torch.zeros_like(ids), ids).to(torch.int32))

            rd, ra = exact(d, pos)
            t0 = lap("replay", t0)
            h_d = self._host("xd", tuple(rd.shape), torch.float64)
            h_a = self._host("xa", tuple(ra.shape), torch.int32)
            h_d.copy_(rd, non_blocking=True)
            h_a.copy_(ra, non_blocking=True)
            h_st[0:1].copy_(status, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            t0 = lap("d2h", t0)
            if check_status(int(h_st[0])):
                # the cached fp16 check was stale: redo with exact fp32 MFMA
                d, pos, status = self._scan(q_search, classes, k_list, _lib.LMI_Q_F32, f64, want=want_w,
                                            rerank=rerank)
                rd, ra = exact(d, pos)
                h_d.copy_(rd)
                h_a.copy_(ra)
                h_st[0:1].copy_(status)
                check_status(int(h_st[0]) & ~_lib.LMI_STATUS_QUERY_NOT_F16)
            return done((h_d.numpy().copy(), h_a.numpy().view(np.uint32).copy()))
        if replay_on == "device":
            bsz, p2id = self._device_tables()
            if want_w is not None:  # (here semantics == "reference")
                bsz = torch.from_numpy(np.ascontiguousarray(bsize, dtype=np.int64)).to(dev)

            def run_replay(d, pos, ans):
                replay_device(classes, d, pos, k_round=k_round, k_final=k, bucket_size=bsz,
                              pos_to_id=p2id, use_threshold=use_threshold,
                              out=(ans[1], ans[2], ans[3][1:2]))
                # a fresh pinned buffer from torch's caching host allocator,
                # handed to the caller as numpy views (no host copy; it returns
                # to the cache when the caller drops the arrays)
                h = torch.empty(tuple(ans[0].shape), dtype=torch.int32, pin_memory=True)
                h.copy_(ans[0], non_blocking=True)
                return h

            h = run_replay(d, pos, ans)
            t0 = lap("replay", t0)
            torch.cuda.current_stream(dev).synchronize()
            t0 = lap("d2h", t0)
            hd, ha, st0, st1 = answer_views(h, nq, w_ans)
            if check_status(st0, st1):
                ans = answer_buffer(nq, w_ans, dev)
                d, pos, status = self._scan(q_search, classes, k_list, _lib.LMI_Q_F32, f64,
                                            status_out=ans[3][0:1], seed_round0=seed, want=want_w,
                                            rerank=rerank)
                h = run_replay(d, pos, ans)
                torch.cuda.current_stream(dev).synchronize()
                hd, ha, st0, st1 = answer_views(h, nq, w_ans)
                check_status(st0 & ~_lib.LMI_STATUS_QUERY_NOT_F16, st1)
            return done((hd, ha))
        h_cls = self._host("cls", (nq, R), torch.int32)
        h_d = self._host("d", tuple(d.shape), d.dtype)
        h_pos = self._host("pos", tuple(pos.shape), torch.int32)
        h_cls.copy_(classes, non_blocking=True)
        h_d.copy_(d, non_blocking=True)
        h_pos.copy_(pos, non_blocking=True)
        h_st[0:1].copy_(status, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        t0 = lap("d2h", t0)
        if check_status(int(h_st[0])):
            d, pos, status = self._scan(q_search, classes, k_list, _lib.LMI_Q_F32, f64,
                                        seed_round0=seed, want=want_w, rerank=rerank)
            h_d.copy_(d)
            h_pos.copy_(pos)
            h_st[0:1].copy_(status)
            check_status(int(h_st[0]) & ~_lib.LMI_STATUS_QUERY_NOT_F16)
        out = replay(h_cls.numpy(), h_d.numpy(), h_pos.numpy(), k_round=k_round, k_final=k,
                     bucket_size=bsize, pos_to_id=self.index.pos_to_id,
                     use_threshold=use_threshold)
        lap("replay", t0) if sync else None
        return done(out)
