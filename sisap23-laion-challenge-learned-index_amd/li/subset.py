"""Search inside an id allow-list (`subset=` of bucket_topk, Searcher.lists / search, LearnedIndex.search): what
the call refuses, and the two small tables scan_subset_kernel (csrc/lmi_scan_subset.hip) reads -- the subset's
rows sorted ascending, and every bucket's range of them."""
from typing import Optional

import numpy as np
import torch

from . import _lib, index_update

MAX_D_PAD = 992  # the kernel's query image in LDS, as the few-query scan's


class Subset:
    """A prepared allow-list of one index: `pos` device int32 [n] the rows, ascending (so sorted by bucket);
    `off` device int64 [C + 1], bucket c's rows are pos[off[c]:off[c + 1]]; `max_range` the longest such range;
    `bucket_size` host int64 [C] their lengths -- the bucket sizes of the index built from the subset alone.
    Valid while the index it was made for lives; pass it as `subset=` to spare a call the preparation."""

    def __init__(self, index, pos: torch.Tensor, off: torch.Tensor):
        self.index, self.pos, self.off, self.n = index, pos, off, int(pos.numel())
        self.bucket_size = (off[1:] - off[:-1]).cpu().numpy()
        self.max_range = int(self.bucket_size.max()) if self.n else 0


def prepare(index, ids) -> Subset:
    """The Subset of the stored ids `ids` (a host or device integer array, any order, or a Subset of this index):
    ids -> positions through the index's sorted id table on the host (index_update.positions_of: KeyError for
    an id the index does not hold), ValueError for duplicates; the positions uploaded and sorted on the
    device, one searchsorted of bucket_off against them for the ranges.  Nothing is allocated per corpus row."""
    if isinstance(ids, Subset):
        if ids.index is not index:
            raise ValueError("subset: this Subset was prepared for another index")
        return ids
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if ids.size and ids.dtype.kind not in "iu":
        raise ValueError("subset: ids must be integers")
    ids = ids.astype(np.int64, copy=False).ravel()
    if np.unique(ids).size != ids.size:
        raise ValueError("subset: duplicate ids")
    pos = index_update.positions_of(index, ids)
    # (world == 1: a row's position is its row of the device arrays)
    d_pos = torch.sort(torch.from_numpy(pos.astype(np.int32)).to(index.device)).values
    off = torch.searchsorted(d_pos, index.bucket_off_local.to(torch.int32)).to(torch.int64)
    return Subset(index, d_pos, off)


# REFUSALS["subset"] of li.index: what a call with `subset=` does not take (a property of the call)
ROWS = {key: "subset= (search inside an id allow-list) takes " + text for key, text in {
    "k": "k in [1, {K}], not {k}",
    "storage": "storage 'f16' alone, not {s!r}",
    "corpus64": "no float64 rows (an index built from float64 data that float32 rounding changes)",
    "metric": "metric 'cosine' alone, not {m!r}",
    "d_pad": f"d_pad <= {MAX_D_PAD}, not {{d_pad}}",
    "bucket": "buckets below 2 GiB of rows (max_chunks * chunk_rows * 2 d_pad)",
    "subcluster": "no sub-cluster layout (subcluster=True)",
    "world": "one GPU (not a striped index)",
    "tags": "no tags (want / avoid)",
    "few": "no few=True (it is a scan of its own)",
    "flags": "no seed, phase or lists16 flag",
    "qmode": "fp16-exact queries (LMI_Q_F16) alone",
    "sub_rows": "sub_rows a positive multiple of 32, not {sub_rows}",
    "dist": "dist='f32' alone",
    "rerank": "no rerank",
    "exchange": "one GPU (no list exchange over a process group)",
    "streamed": "no streamed() and no graph() (the eager step alone)",
    "range": "no range search",
    # (the default path would scan such queries in exact fp32; this kernel rounds them to fp16)
    "batch": "fp16-exact queries (LMI_Q_F16) alone: a value of this batch is not fp16-representable",
}.items()}


def refusal(index, k: int, sub_rows=None, **flags) -> Optional[str]:
    """The first row of ROWS that applies to a call with `subset=`, or None."""
    f = flags.get
    return "k" if not 1 <= k <= _lib.LMI_MAX_K else \
        "storage" if index.storage != "f16" else \
        "corpus64" if index.corpus64 is not None else \
        "metric" if index.metric != "cosine" else \
        "d_pad" if index.d_pad > MAX_D_PAD else \
        "bucket" if max(index.max_chunks, 1) * index.chunk_rows * index.d_pad * 2 >= 1 << 31 else \
        "subcluster" if index.chunk_centroid is not None else \
        "world" if getattr(index, "world", 1) > 1 else \
        "tags" if f("want") is not None or f("avoid") is not None else \
        "few" if f("few") else \
        "flags" if f("seed_round0") or f("phases") or f("lists16") else \
        "qmode" if f("qmode") not in (None, _lib.LMI_Q_F16) else \
        "sub_rows" if sub_rows is not None and (sub_rows <= 0 or sub_rows % 32) else \
        "dist" if f("dist", "f32") != "f32" else \
        "rerank" if f("rerank") is not None else \
        "exchange" if f("exchange") else None
