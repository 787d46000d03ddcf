"""The 8-bit storage on the GPU (storage "i8": lmi_quantize_rows_i8,
prep_i8_kernel, scan_i8_kernel), bit for bit against the numpy restatement of
tests/i8_cases.py -- int8 x int8 products summed in int32 are exact and
order-independent, so no check here has a tolerance.

One seeded fixture per row width: five buckets of 2 100 / 37 / 700 / 7 / 0 rows
with chunk_rows = 1024 (bucket 0: three chunks with a 52-row tail; bucket 3
shorter than k; bucket 4 empty), 300 queries x 2 probes with `classes` given.
Planted in bucket 0: five exact duplicates across its chunks (ties break by
position), one all-zero row, and one row [127, 0.5, 1.5, 2.5, -0.5, 0, ...]
(s = 1: the half-way values round to even, 0, 2, 2, -0).  Widths: 768, 96, 200
(d_pad 224: one 128-wide block and three 32-wide ones), 32 (a single 32-wide
block) and 992 (the widest, the largest |acc|)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import i8_cases as I8
import workloads
from li import _lib
from li.index import DeviceIndex, DeviceRouter, RowSource, Searcher, bucket_range, bucket_topk, bucket_topk_f64, \
    quantize_rows, replay

pytestmark = pytest.mark.gpu

SIZES = (2100, 37, 700, 7, 0)
N, C, CHUNK, NQ, R = sum(SIZES), 5, 1024, 300, 2
WIDTHS = (768, 96, 200, 32, 992)
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 2), (0, 7), (1 << 31, 1), (0, 1 << 30), (4, 3))
TOMB = 1 << 29
SEED = 5302
DEV = "cuda"


def _ok(tags, w, a):
    tags = np.asarray(tags, np.uint32)
    return ((tags & np.uint32(w)) == np.uint32(w)) & ((tags & np.uint32(a)) == 0)


@functools.lru_cache(maxsize=None)
def _fixture(d):
    rng = np.random.default_rng(SEED + d)
    x = rng.standard_normal((N, d)).astype(np.float16).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float16).astype(np.float32)
    labels = rng.permutation(np.repeat(np.arange(C), SIZES)).astype(np.int64)
    ids = (rng.permutation(N) + 1001).astype(np.int64)
    b0 = np.flatnonzero(labels == 0)
    dup = b0[[10, 11, 900, 2060, 2090]]                     # five copies of one row, across the chunks
    x[dup] = x[dup[0]]
    q[5] = x[dup[0]]                                        # a query that lists all five
    zero, half = b0[20], b0[1100]
    x[zero] = 0.0
    x[half] = 0.0
    x[half, :5] = [127.0, 0.5, 1.5, 2.5, -0.5]
    # tags as the tag-mask fixture draws them
    tags = rng.integers(0, 8, N).astype(np.uint32)
    tags[labels == 1] |= np.uint32(1 << 30)
    tags[b0[[3, 700, 1400, 2099]]] |= np.uint32(1 << 31)
    tags[dup] = (tags[dup] & ~np.uint32(7)) | np.arange(5, dtype=np.uint32)
    classes = np.empty((NQ, R), np.int32)
    i = np.arange(NQ)
    classes[:270, 0], classes[:270, 1] = 0, 1 + i[:270] % 4
    classes[270:, 0], classes[270:, 1] = 1 + i[270:] % 4, 0
    pair = rng.integers(0, len(PAIRS), NQ)
    pair[:len(PAIRS)] = np.arange(len(PAIRS))
    pw = np.array(PAIRS, np.int64)[pair]
    return dict(x=x, q=q, labels=labels, ids=ids, tags=tags, classes=classes, pair=pair, want=pw[:, 0].copy(),
                avoid=pw[:, 1].copy(), dup=dup, zero=zero, half=half)


def _build(f, rows=slice(None), storage="i8", tags="own", **kw):
    t = f["tags"][rows] if isinstance(tags, str) else tags
    return DeviceIndex(f["x"][rows], f["labels"][rows], C, ids=f["ids"][rows], chunk_rows=CHUNK, device=DEV,
                       storage=storage, tags=t, **kw)


@functools.lru_cache(maxsize=None)
def _searcher(d):
    return Searcher(_build(_fixture(d)), None)


@functools.lru_cache(maxsize=None)
def _restated(d):
    """The restatement of width d, computed once and left unchanged: the codes
    in position order, the queries' codes, every distance."""
    f, ix = _fixture(d), _searcher(d).index
    cx, invx = I8.quantize(f["x"][ix.layout.order])
    cq, invq = I8.quantize(f["q"])
    dist = I8.distances(cq, invq, cx, invx)
    for a in (cx, invx, dist):
        a.setflags(write=False)
    return cx, invx, dist


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _lists(s, f, k, rows=slice(None), **kw):
    _, d, pos, st = s.lists(None, _T(f["q"][rows]), R, k, classes=_T(f["classes"][rows]), **kw)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    d, pos = d.cpu().numpy(), pos.cpu().numpy()
    ids = np.where(pos >= 0, s.index.pos_to_id[np.maximum(pos, 0)], -1)
    return d, pos, ids


# ---- 1. the quantiser ----------------------------------------------------------------------
@pytest.mark.parametrize("d", [200, 768, 32])
def test_quantiser_is_the_restatement_bit_for_bit(d):
    f = _fixture(d)
    rng = np.random.default_rng(SEED + 7 * d)
    d_pad = I8.d_pad_of(d)
    exact = f["x"][:600].copy()                                   # (holds the planted rows' neighbours: any rows do)
    exact[0], exact[1] = f["x"][f["zero"]], f["x"][f["half"]]
    exact[2] = 0.0
    exact[2, d - 1] = 2.0 ** -14                                   # fp16-exact and tiny beside nothing: m = 2^-14
    rough = rng.standard_normal((600, d)).astype(np.float32)      # not fp16-exact
    rough[3] = 0.0
    rough[3, 0] = 2.0 ** -101                                      # under the 2^-100 rule: zero codes
    rough[4, 1] = np.nan
    assert not np.array_equal(rough.astype(np.float16).astype(np.float32), rough)
    cases = (("fp16", exact.astype(np.float16)), ("f32 of fp16 values", exact), ("f32", rough))
    for name, rows in cases:
        ref_c, ref_inv = I8.quantize(rows)
        m = rows.shape[0]
        # contiguous, slot i
        codes = torch.full((m, d_pad), 0x55, dtype=torch.int8, device=DEV)
        inv = torch.full((m,), -1.0, dtype=torch.float32, device=DEV)
        quantize_rows(_T(rows), d_pad, codes, inv)
        torch.cuda.synchronize()
        assert np.array_equal(codes.cpu().numpy(), ref_c), name
        assert np.array_equal(_bits(inv.cpu().numpy()), _bits(ref_inv)), name
        assert not ref_c[:, d:].any()
        # ld > d (a column slice of a wider block, rows not 16-byte aligned), scattered by dst_rows
        wide = torch.zeros((m, d + 5), dtype=_T(rows[:1]).dtype, device=DEV)
        wide[:, 3:3 + d] = _T(rows)
        dst = rng.permutation(m + 50)[:m].astype(np.int64)
        codes = torch.full((m + 50, d_pad), 0x55, dtype=torch.int8, device=DEV)
        inv = torch.full((m + 50,), -1.0, dtype=torch.float32, device=DEV)
        quantize_rows(wide[:, 3:3 + d], d_pad, codes, inv, dst_rows=_T(dst))
        torch.cuda.synchronize()
        got_c, got_inv = codes.cpu().numpy(), inv.cpu().numpy()
        assert np.array_equal(got_c[dst], ref_c) and np.array_equal(_bits(got_inv[dst]), _bits(ref_inv)), name
        rest = np.setdiff1d(np.arange(m + 50), dst)
        assert (got_c[rest] == 0x55).all() and (got_inv[rest] == -1.0).all(), name   # untouched slots
    c, inv = I8.quantize(exact[:3])
    assert not c[0].any() and inv[0] == 1.0
    assert c[1, :5].tolist() == [127, 0, 2, 2, 0]


# ---- 2. lists --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("d", WIDTHS)
def test_lists_are_the_restatement_bit_for_bit(d, k):
    f, s = _fixture(d), _searcher(d)
    ix = s.index
    cx, invx, dist = _restated(d)
    assert ix.storage == "i8" and ix.corpus.dtype == torch.int8 and ix.corpus64 is None
    assert np.array_equal(ix.corpus.cpu().numpy(), cx) and np.array_equal(_bits(ix.inv_norm.cpu().numpy()), _bits(invx))
    ref_d, ref_p = I8.bucket_lists(dist, ix.layout.bucket_off, f["classes"], k)
    got_d, got_p, _ = _lists(s, f, k)                               # (asserts the status word is 0)
    assert np.array_equal(_bits(got_d), _bits(ref_d)) and np.array_equal(got_p, ref_p)
    # the short and the empty bucket are padded
    short, empty = f["classes"] == 3, f["classes"] == 4
    assert short.any() and empty.any()
    assert np.isinf(got_d[empty]).all() and (got_p[empty] == -1).all()
    assert np.isfinite(got_d[short][:, :min(k, 7)]).all() and np.isinf(got_d[short][:, 7:]).all()
    if k > 1:
        # the duplicates: equal distances, ascending positions, wherever they are listed
        dup_pos = np.sort(np.flatnonzero(np.isin(ix.pos_to_id, f["ids"][f["dup"]])))
        seen = 0
        for i in range(NQ):
            for r in range(R):
                at = np.flatnonzero(np.isin(got_p[i, r], dup_pos))
                if at.size > 1:
                    seen += 1
                    assert np.unique(_bits(got_d[i, r, at])).size == 1
                    assert np.array_equal(got_p[i, r, at], dup_pos[:at.size])
        assert seen, "no list holds two of the duplicates"


# ---- 3. filtered -----------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(768, 10), (96, 16), (200, 10), (992, 16)])
def test_filtered_lists_equal_the_eligible_rows_index(d, k):
    f, s = _fixture(d), _searcher(d)
    got_d, got_p, got_ids = _lists(s, f, k, want=f["want"], avoid=f["avoid"])
    # the restatement over the eligible rows
    t = f["tags"][s.index.layout.order]
    elig = np.stack([_ok(t, f["want"][i], f["avoid"][i]) for i in range(NQ)])
    ref_d, ref_p = I8.bucket_lists(_restated(d)[2], s.index.layout.bucket_off, f["classes"], k, eligible=elig)
    assert np.array_equal(_bits(got_d), _bits(ref_d)) and np.array_equal(got_p, ref_p)
    # and the i8 index built from the eligible rows alone (per-row quantisation makes this exact)
    for p, (w, a) in enumerate(PAIRS[:5] if d != 768 else PAIRS):
        rows = np.flatnonzero(f["pair"] == p)
        ref = Searcher(_build(f, _ok(f["tags"], w, a), tags=None), None)
        e_d, _, e_ids = _lists(ref, f, k, rows=rows)
        assert np.array_equal(_bits(got_d[rows]), _bits(e_d)) and np.array_equal(got_ids[rows], e_ids), (w, a)


# ---- 4. phases -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(768, 10), (200, 16)])
def test_plan_scan_merge_as_three_calls(d, k):
    f, ix = _fixture(d), _searcher(d).index
    q, cls = _T(f["q"]), _T(f["classes"])
    one_d, one_p, st = bucket_topk(ix, q, cls, k)
    need = _lib.load().lmi_scan_workspace_bytes(ctypes.byref(ix.desc), NQ, R, k, _lib.LMI_Q_I8)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = (torch.full((NQ, R, k), 7.0, device=DEV), torch.full((NQ, R, k), 7, dtype=torch.int32, device=DEV),
           torch.zeros(1, dtype=torch.int32, device=DEV))
    for ph in (_lib.LMI_Q_PHASE_PLAN, _lib.LMI_Q_PHASE_SCAN, _lib.LMI_Q_PHASE_MERGE):
        bucket_topk(ix, q, cls, k, out=out, ws=ws, phases=ph)
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(out[2].item()) == 0
    assert torch.equal(out[0].view(torch.int32), one_d.view(torch.int32)) and torch.equal(out[1], one_p)


# ---- 5. builds -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 200])
def test_three_builds_give_one_index(d):
    f = _fixture(d)
    direct = _searcher(d).index
    f16 = _build(f, storage="f16")
    quant = f16.quantized()
    x16 = _T(f["x"].astype(np.float16))
    source = DeviceIndex(RowSource(N, d, lambda a, b: x16[a:b], chunk=1000), f["labels"], C, ids=f["ids"],
                         chunk_rows=CHUNK, device=DEV, storage="i8", tags=f["tags"])
    for other in (quant, source):
        assert other.storage == "i8" and other.corpus.dtype == torch.int8 and other.d_pad == direct.d_pad
        assert torch.equal(other.corpus, direct.corpus)
        assert torch.equal(other.inv_norm.view(torch.int32), direct.inv_norm.view(torch.int32))
        assert torch.equal(other.gpos, direct.gpos) and torch.equal(other.tags, direct.tags)
        assert torch.equal(other.bucket_off_local, direct.bucket_off_local)
        assert torch.equal(other.chunk_first, direct.chunk_first)
        assert np.array_equal(other.pos_to_id, direct.pos_to_id) and other.chunk_rows == direct.chunk_rows
    # the old index stays valid, and the new one answers as the direct build
    assert f16.storage == "f16" and not f16.consumed
    a = _lists(Searcher(f16, None), f, 10)
    assert np.isfinite(a[0]).any()
    b, c = _lists(Searcher(quant, None), f, 10), _lists(_searcher(d), f, 10)
    assert np.array_equal(_bits(b[0]), _bits(c[0])) and np.array_equal(b[1], c[1])


def test_float32_and_float64_rows_quantise_from_their_float32_values():
    d = 96
    f = _fixture(d)
    rng = np.random.default_rng(SEED + 11)
    x32 = rng.standard_normal((N, d)).astype(np.float32)              # not fp16-exact
    x64 = x32.astype(np.float64) * (1.0 + 1e-10 * rng.uniform(-1.0, 1.0, (N, d)))   # far inside half an ulp
    assert np.array_equal(x64.astype(np.float32), x32) and not np.array_equal(x64, x32.astype(np.float64))
    kw = dict(ids=f["ids"], chunk_rows=CHUNK, device=DEV)
    a = DeviceIndex(x32, f["labels"], C, storage="i8", **kw)
    b = DeviceIndex(x64, f["labels"], C, storage="i8", **kw)
    c = DeviceIndex(x32, f["labels"], C, storage="f32", **kw).quantized()
    ref_c, ref_inv = I8.quantize(x32[a.layout.order])
    for ix in (a, b, c):
        assert ix.corpus64 is None
        assert np.array_equal(ix.corpus.cpu().numpy(), ref_c)
        assert np.array_equal(_bits(ix.inv_norm.cpu().numpy()), _bits(ref_inv))
    assert DeviceIndex(f["x"], f["labels"], C, **kw).storage == "f16"   # "auto" never chooses it


# ---- 6. Searcher.search ----------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 96])
def test_search_equals_the_replay_of_the_restated_lists(d):
    f, s = _fixture(d), _searcher(d)
    ix = s.index
    ref_d, ref_p = I8.bucket_lists(_restated(d)[2], ix.layout.bucket_off, f["classes"], 10)
    q, cls = _T(f["q"]), _T(f["classes"])
    for thr in (True, False):
        want = replay(f["classes"], ref_d, ref_p, k_round=10, k_final=10, bucket_size=ix.bucket_size,
                      pos_to_id=ix.pos_to_id, use_threshold=thr)
        for on in ("device", "host"):
            got = s.search(None, q, R, k=10, classes=cls, use_threshold=thr, replay_on=on)
            assert np.array_equal(got[1], want[1]), (thr, on)
            assert np.array_equal(_bits(got[0]), _bits(want[0])), (thr, on)
    for k in (10, 16):
        lists = I8.bucket_lists(_restated(d)[2], ix.layout.bucket_off, f["classes"], k)
        want = I8.merged_topk(*lists, k, ix.pos_to_id)
        got = s.search(None, q, R, k=k, classes=cls, semantics="exact")
        assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0])), k
    # float64 queries are rounded to float32 inside the call
    got = s.search(None, _T(f["q"].astype(np.float64)), R, k=10, classes=cls, semantics="exact")
    assert np.array_equal(got[1], want[1][:, :10])


def test_learned_index_attach_storage_i8():
    import pandas as pd
    from li.LearnedIndex import LearnedIndex
    from li.model import NeuralNetwork
    Cw = 8
    w = workloads.clustered(n=2000, nq=64, C=Cw, seed=11, label_mode="router")
    nn = NeuralNetwork(input_dim=w["xn"].shape[1], output_dim=Cw, lr=0.009, model_type="MLP")
    lin = [m for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (wt, b) in zip(lin, w["layers"]):
            m.weight.copy_(torch.from_numpy(wt))
            m.bias.copy_(torch.from_numpy(b))
    nav, ds = pd.DataFrame(w["xn"]), pd.DataFrame(w["x"].astype(np.float16))   # (fp16 'emb': dist_dtype says f64)
    nav.index += 1
    ds.index += 1
    li_ = LearnedIndex()
    li_.model = nn
    index = li_.attach(nav, ds, w["labels"], storage="i8")
    assert index.storage == "i8"
    got = li_.search(nav, w["qn"], ds, w["q"], w["labels"], n_buckets=3, k=10, use_threshold=True)
    assert li_._index is index
    ref = Searcher(DeviceIndex(w["x"].astype(np.float16), w["labels"], index.n_buckets,
                               ids=np.arange(1, 2001, dtype=np.int64), device=DEV, storage="i8"),
                   DeviceRouter(w["layers"], device=DEV)).search(_T(w["qn"]), _T(w["q"]), 3, k=10, use_threshold=True)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    # an attach without `storage` keeps the cached index; one that names another storage rebuilds
    assert li_.attach(nav, ds, w["labels"]) is index
    assert li_.attach(nav, ds, w["labels"], storage="f16").storage == "f16"


# ---- 7. tag edits ----------------------------------------------------------------------------
def test_edit_tags_then_avoid_hides_the_rows():
    d = 96
    f = _fixture(d)
    s = Searcher(_build(f), None)                                     # (its own index: the edit is in place)
    q, cls = _T(f["q"]), _T(f["classes"])
    before = s.search(None, q, R, k=10, classes=cls, semantics="exact")
    hide = np.unique(before[1][:, :3].ravel())                        # every query's three best
    hide = hide[hide > 0].astype(np.int64)
    s.index.edit_tags(hide, set_bits=TOMB)
    s.index.set_tags(hide[:2], TOMB | 5)
    assert np.array_equal(np.sort(s.index.ids_with(want=TOMB)), np.sort(hide))
    got = s.search(None, q, R, k=10, classes=cls, semantics="exact", avoid=TOMB)
    assert not np.isin(got[1], hide).any()
    elig = np.broadcast_to(~np.isin(s.index.pos_to_id, hide), (NQ, N))
    lists = I8.bucket_lists(_restated(d)[2], s.index.layout.bucket_off, f["classes"], 10, eligible=elig)
    want = I8.merged_topk(*lists, 10, s.index.pos_to_id)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
    # the reference semantics: the answer of the index built from the rows that are left
    keep = ~np.isin(f["ids"], hide)
    ref = Searcher(_build(f, keep, tags=None), None).search(None, q, R, k=10, classes=cls)
    got = s.search(None, q, R, k=10, classes=cls, avoid=TOMB)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])


# ---- 8. refusals -----------------------------------------------------------------------------
def test_refusals_name_the_storage_and_the_index_still_answers():
    d = 96
    f, s = _fixture(d), _searcher(d)
    ix = s.index
    q, cls = _T(f["q"]), _T(f["classes"])
    free0 = torch.cuda.memory_allocated()
    calls = {
        "capacity": lambda: _build(f, capacity=N + 10),
        "subcluster": lambda: _build(f, tags=None, subcluster=True),
        "world > 1": lambda: _build(f, rank=0, world=2),
        "d > 992": lambda: DeviceIndex(np.zeros((4, 1000), np.float16), np.zeros(4, np.int64), 1, device=DEV,
                                       storage="i8"),
        "search f64": lambda: s.search(None, q, R, k=10, classes=cls, dist="f64"),
        "lists f64": lambda: s.lists(None, q, R, 10, classes=cls, dist="f64"),
        "lists k 17": lambda: s.lists(None, q, R, 17, classes=cls),
        "search k 20 exact": lambda: s.search(None, q, R, k=20, classes=cls, semantics="exact"),
        "search k_round 17": lambda: s.search(None, q, R, k=10, k_round=17, classes=cls),
        "bucket_topk k 17": lambda: bucket_topk(ix, q, cls, 17),
        "bucket_topk_f64": lambda: bucket_topk_f64(ix, q, cls, 10),
        "range_search": lambda: s.range_search(None, q, R, 0.5, classes=cls),
        "bucket_range": lambda: bucket_range(ix, q, cls, 0.5),
        "streamed": lambda: s.streamed(None, q, R, 10),
        "graph": lambda: s.graph(None, q, R, 10),
        "process group": lambda: Searcher(ix, None, exchange=True),
        "add": lambda: ix.add(f["x"][:2], f["labels"][:2]),
        "remove": lambda: ix.remove(f["ids"][:2]),
        "relabel": lambda: ix.relabel(f["labels"]),
        "reserve": lambda: ix.reserve(N + 10),
        "quantized": lambda: ix.quantized(),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError) as e:
            call()
        assert "'i8'" in str(e.value), (name, str(e.value))
    assert torch.cuda.memory_allocated() == free0                      # nothing was allocated on the way
    with pytest.raises(ValueError):
        _build(f, storage="i4")
    ref_d, ref_p = I8.bucket_lists(_restated(d)[2], ix.layout.bucket_off, f["classes"], 10)
    got_d, got_p, _ = _lists(s, f, 10)
    assert np.array_equal(_bits(got_d), _bits(ref_d)) and np.array_equal(got_p, ref_p)
