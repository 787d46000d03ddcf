// K2 at k > 16 (gfx950): lists longer than one scan's register lists, by
// lower-bound passes (bucket_topk_passes) or, on the 8-wave ring, by a sampled
// bound and a collect scan (bucket_topk_wide).  Every scan is a call of
// bucket_topk_impl (lmi_scan.hip); the kernels here prepare and consume them.
#include "lmi_scan_internal.hpp"

#include <algorithm>

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// k > 16: lower-bound passes
// ---------------------------------------------------------------------------
// After pass j (entries [j*kp, (j+1)*kp) of every pair's list): the next
// pass's lower bound is the (distance, global position) key of the pass's last
// entry; a pair whose pass came back short is exhausted (a key above every
// real key: nothing passes).
__global__ __launch_bounds__(256) void next_lo_kernel(const float* __restrict__ d,
                                                      const int32_t* __restrict__ pos, int32_t P,
                                                      int32_t ldo, int32_t last,
                                                      unsigned long long* __restrict__ lo) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const size_t o = (size_t)p * ldo + last;
    const int32_t g = pos[o];
    lo[p] = g < 0 ? ~0ull : (((unsigned long long)f2ord(d[o]) << 32) | (uint32_t)g);
}

// ---------------------------------------------------------------------------
// k > 16: bound + collect (bucket_topk_wide)
// ---------------------------------------------------------------------------
// slot of the j-th list of a pair in the partial lists: chunks first, then
// parts 1..S-1 of every split chunk (bit of sm) in ascending order (the order
// chunk_merge_kernel reads them in; X = max_chunks / S)
__device__ inline int wide_slot(int j, int nch_c, uint32_t sm, int S, int X) {
    if (j < nch_c) return j;
    const int jj = j - nch_c;
    int nth = jj / (S - 1);
    const int part = 1 + jj % (S - 1);
    for (; nth > 0; --nth) sm &= sm - 1u;
    return part * X + __builtin_ctz(sm);
}

// The bound pass's lists (one workgroup): bucket c of n_c rows gets L =
// min(lists, n_c / 32) lists of r_c = n_c / L rows (up to a multiple of 32),
// each scanning its first take_c = max(128, r_c / 4) rows (a sample); chunk_first
// is the prefix of the list counts (a thread per contiguous run of buckets, then
// a prefix over the threads).
__global__ __launch_bounds__(256) void bound_lists_kernel(const int64_t* __restrict__ bucket_off, int32_t C,
                                                          int32_t lists, int32_t* __restrict__ chunk_first,
                                                          int32_t* __restrict__ sub_rows,
                                                          int32_t* __restrict__ sub_take) {
    __shared__ int32_t part[256];
    const int t = threadIdx.x;
    const int per = (C + 255) / 256;
    const int c0 = min(C, t * per), c1 = min(C, c0 + per);
    auto count = [&](int c) {
        const int64_t n = bucket_off[c + 1] - bucket_off[c];
        if (n <= 0) return 0;
        const int64_t L = std::max<int64_t>(1, std::min<int64_t>(lists, n / 32));
        const int64_t r = (n + L - 1) / L;
        const int32_t rr = (int32_t)((r + 31) / 32 * 32);
        sub_rows[c] = rr;
        sub_take[c] = std::min(rr, std::max(128, (rr / 4 + 31) / 32 * 32));
        return (int)((n + rr - 1) / rr);
    };
    int32_t acc = 0;
    for (int c = c0; c < c1; ++c) acc += count(c);
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int32_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    acc = part[t];
    for (int c = c0; c < c1; ++c) {
        chunk_first[c] = acc;
        const int64_t n = bucket_off[c + 1] - bucket_off[c];
        acc += n <= 0 ? 0 : (int32_t)((n + sub_rows[c] - 1) / sub_rows[c]);
    }
    if (c0 < C && c1 == C) chunk_first[C] = acc;
}

// outputs padded (+inf, -1), bounds and the fix-up flags cleared
__global__ __launch_bounds__(256) void wide_init_kernel(int64_t P, int32_t ldo, float* __restrict__ d,
                                                        int32_t* __restrict__ pos, int32_t* __restrict__ row,
                                                        uint32_t* __restrict__ bound_ord,
                                                        int32_t* __restrict__ fix) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < P * ldo) {
        d[t] = __builtin_inff();
        pos[t] = -1;
        if (row) row[t] = -1;
    }
    if (t < P) {
        bound_ord[t] = 0u;
        fix[t] = 0;
    }
}

// Per grouped pair of the chunk-list scan (one 64-lane workgroup): the kw-th
// smallest distance ordinal over its chunk lists (each the part's own top-15,
// so at least kw rows lie within it) by a 4-digit radix select; fewer than
// kw entries: no bound, the pair goes to the fix-up passes.
__global__ __launch_bounds__(64) void kth_bound_kernel(
    const uint64_t* __restrict__ partial, int32_t max_chunks, int32_t S,
    const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_bucket,
    const int32_t* __restrict__ chunk_first, const uint32_t* __restrict__ split_mask, int32_t P,
    int32_t kw, const int64_t* __restrict__ bucket_off, int32_t cap, uint32_t* __restrict__ bound_ord,
    int32_t* __restrict__ fix) {
    constexpr int KL = 15;
    const int pp = blockIdx.x;
    const int c = pair_bucket[pp];
    if (c < 0) return;
    const int p = pair_q[pp];
    if (p < 0 || p >= P) return;
    const uint32_t sm = split_mask != nullptr ? split_mask[pp] : 0u;
    const int nch_c = chunk_first[c + 1] - chunk_first[c];
    const int nl = nch_c + (S - 1) * __popc(sm);
    const int X = max_chunks / S;
    const uint64_t* base = partial + (size_t)pp * max_chunks * KL;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_mask, s_rem, s_n;
    const int tid = threadIdx.x;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    uint32_t n = 0;
    for (int e = tid; e < nl * KL; e += 64) {
        const uint64_t key = base[(size_t)wide_slot(e / KL, nch_c, sm, S, X) * KL + e % KL];
        n += key != kEmptyKey ? 1u : 0u;
    }
    atomicAdd(&s_n, n);
    if (tid == 0) {
        s_prefix = 0u;
        s_mask = 0u;
        s_rem = (uint32_t)kw;
    }
    __syncthreads();
    if (s_n < (uint32_t)kw) {
        // too few list entries: a bucket of no more rows than the slots is
        // collected whole (no bound), else the pair takes the fix-up passes
        // (bound_ord stays 0: the collect takes nothing)
        if (tid == 0) {
            if (bucket_off[c + 1] - bucket_off[c] <= cap) bound_ord[p] = 0xffffffffu;
            else fix[p] = 1;
        }
        return;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += 64) hist[i] = 0u;
        __syncthreads();
        const uint32_t prefix = s_prefix, mask = s_mask;
        for (int e = tid; e < nl * KL; e += 64) {
            const uint64_t key = base[(size_t)wide_slot(e / KL, nch_c, sm, S, X) * KL + e % KL];
            const uint32_t h = (uint32_t)(key >> 32);
            if (key != kEmptyKey && (h & mask) == prefix) atomicAdd(&hist[(h >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rem = s_rem, dg = 0;
            for (; dg < 255u && hist[dg] < rem; ++dg) rem -= hist[dg];
            s_rem = rem;
            s_prefix = prefix | (dg << shift);
            s_mask = mask | (255u << shift);
        }
        __syncthreads();
    }
    if (tid == 0) bound_ord[p] = s_prefix;
}
// Per grouped pair of the collect scan (one 256-lane workgroup): its
// candidates sorted by (distance, row) -- rows ascend with global position
// inside a bucket, so this is the reference's (distance, g.index) order --
// and the first kw written as (d, global position, row).  A pair whose
// candidates overflowed (or, never for a sound scan, came back short) goes to
// the fix-up passes.
__global__ __launch_bounds__(256) void collect_select_kernel(
    const uint64_t* __restrict__ cand, const uint32_t* __restrict__ ccount, int32_t cap,
    const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_bucket,
    const int32_t* __restrict__ gpos, int32_t P, int32_t kw, int32_t ldo,
    const uint32_t* __restrict__ bound_ord, int32_t* __restrict__ fix, float* __restrict__ out_d,
    int32_t* __restrict__ out_pos, int32_t* __restrict__ out_row) {
    extern __shared__ uint64_t keys[];
    const int pp = blockIdx.x;
    if (pair_bucket[pp] < 0) return;
    const int p = pair_q[pp];
    if (p < 0 || p >= P || fix[p]) return;
    const uint32_t n = ccount[pp];
    const int tid = threadIdx.x;
    // (fewer than kw: only a bucket collected whole, every row under the
    // all-ones bound; never for a sound scan otherwise)
    if (n > (uint32_t)cap || (n < (uint32_t)kw && bound_ord[p] != 0xffffffffu)) {
        if (tid == 0) fix[p] = 1;
        return;
    }
    uint32_t m = 1;
    while (m < n) m <<= 1;
    const uint64_t* src = cand + (size_t)pp * cap;
    for (uint32_t i = tid; i < m; i += 256) keys[i] = i < n ? src[i] : kEmptyKey;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= m; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < m; i += 256) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t x = keys[i], y = keys[l];
                    const bool up = (i & k2) == 0;
                    if ((x > y) == up) {
                        keys[i] = y;
                        keys[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    const size_t o = (size_t)p * ldo;
    for (int i = tid; i < kw && i < (int)n; i += 256) {
        const uint64_t key = keys[i];
        const uint32_t r = (uint32_t)key;
        out_d[o + i] = ord2f((uint32_t)(key >> 32));
        out_pos[o + i] = gpos[r];
        if (out_row) out_row[o + i] = (int32_t)r;
    }
}

// the fix-up passes' classes: the pair's class where it needs them, else -1
// (out of range: the plan skips the pair)
__global__ __launch_bounds__(256) void fix_classes_kernel(const int32_t* __restrict__ classes,
                                                          const int32_t* __restrict__ fix, int32_t P,
                                                          int32_t* __restrict__ cls_fix) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < P) cls_fix[p] = fix[p] ? classes[p] : -1;
}

// the fix-up passes' lists over the outputs of the pairs that took them
__global__ __launch_bounds__(256) void fix_combine_kernel(const int32_t* __restrict__ fix, int64_t P,
                                                          int32_t ldo, const float* __restrict__ fd,
                                                          const int32_t* __restrict__ fpos,
                                                          const int32_t* __restrict__ frow,
                                                          float* __restrict__ d, int32_t* __restrict__ pos,
                                                          int32_t* __restrict__ row) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P * ldo) return;
    if (!fix[t / ldo]) return;
    d[t] = fd[t];
    pos[t] = fpos[t];
    if (row) row[t] = frow[t];
}

// first k of every pair's pass list -> the caller's [P][k] outputs
__global__ __launch_bounds__(256) void take_k_kernel(const float* __restrict__ d,
                                                     const int32_t* __restrict__ pos, int64_t P,
                                                     int32_t ldo, int32_t k, float* __restrict__ out_d,
                                                     int32_t* __restrict__ out_pos) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= P * k) return;
    const int64_t p = t / k;
    const int j = (int)(t - p * k);
    out_d[t] = d[(size_t)p * ldo + j];
    out_pos[t] = pos[(size_t)p * ldo + j];
}

}  // namespace

// k > 16: ceil(k / kp) scan passes of kp-entry lists (kp = 15 on the 8-wave
// ring, else 16), each keeping the next kp entries of the (distance, position)
// order after the previous pass's last key.  Lists of ldo = passes * kp entries.
int passes_of(const lmi_index_desc* idx, int qmode, int k, int* kp_out) {
    const int kp = band_capable(idx, qmode) ? 15 : 16;
    if (kp_out) *kp_out = kp;
    return (k + kp - 1) / kp;
}

size_t passes_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k, int qmode) {
    int kp;
    passes_of(idx, qmode, k, &kp);
    const size_t P = (size_t)nq * R;
    return align_up(P * 8, 256) + scan_workspace_bytes(idx, nq, R, kp, qmode, true);
}

// (c: the lists [nq*R][c.ldo] and no option but ldo)
int bucket_topk_passes(const ScanCall& c) {
    int kp;
    const int np = passes_of(c.idx, c.qmode, c.k, &kp);
    if (c.ldo < np * kp) {
        set_error("pass lists of %d entries < %d passes x %d", c.ldo, np, kp);
        return LMI_E_INVALID;
    }
    const size_t P = (size_t)c.nq * c.R;
    auto* ws = reinterpret_cast<unsigned char*>(c.workspace);
    auto* lo = reinterpret_cast<unsigned long long*>(ws);
    const size_t lo_bytes = align_up(P * 8, 256);
    if (c.ws_bytes < lo_bytes) {
        set_error("workspace %zu B too small", c.ws_bytes);
        return LMI_E_WORKSPACE;
    }
    LMI_TRY(fill_u32(lo, 0u, P * 2, c.stream));
    ScanCall pass = c;
    pass.k = kp;
    pass.workspace = ws + lo_bytes;
    pass.ws_bytes = c.ws_bytes - lo_bytes;
    pass.lo_g = lo;
    for (int j = 0; j < np; ++j) {
        pass.out_d = c.out_d + (size_t)j * kp;
        pass.out_pos = c.out_pos + (size_t)j * kp;
        pass.out_row = c.out_row ? c.out_row + (size_t)j * kp : nullptr;
        pass.prefill = j == 0;
        LMI_TRY(bucket_topk_impl(pass));
        if (j + 1 < np) {
            hipLaunchKernelGGL(next_lo_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c.stream, c.out_d,
                               c.out_pos, (int32_t)P, c.ldo, (j + 1) * kp - 1, lo);
            LMI_LAUNCH_CHECK("next_lo_kernel");
        }
    }
    return LMI_OK;
}

// The bound scan's index: the same rows and buckets, each bucket cut into at
// most `lists` lists (bound_lists_kernel; their rows per bucket in sub_rows),
// no chunk centroids (the nearest-chunk-first plan's units are the index's
// chunks).  Host-side values only: the workspace size must not read the device.
lmi_index_desc bound_desc(const lmi_index_desc* idx, int lists, const int32_t* sub_first) {
    lmi_index_desc b = *idx;
    b.max_chunks = lists;
    b.n_chunks = idx->n_buckets * lists;
    b.chunk_first = sub_first;
    b.chunk_centroid = nullptr;
    return b;
}

int sampled_bound(const ScanCall& scan, const BoundScan& b) {
    const lmi_index_desc* idx = scan.idx;
    hipStream_t s = scan.stream;
    const int P = scan.nq * scan.R;
    const int64_t n_init = std::max<int64_t>((int64_t)P * b.pad_ldo, P);
    hipLaunchKernelGGL(wide_init_kernel, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, s, (int64_t)P,
                       b.pad_ldo, b.pad_d, b.pad_pos, b.pad_row, b.bound, b.fix);
    LMI_LAUNCH_CHECK("wide_init_kernel");
    hipLaunchKernelGGL(bound_lists_kernel, dim3(1), dim3(256), 0, s, idx->bucket_off, idx->n_buckets, b.lists,
                       b.sub_first, b.sub_rows, b.sub_take);
    LMI_LAUNCH_CHECK("bound_lists_kernel");
    const lmi_index_desc bd = bound_desc(idx, b.lists, b.sub_first);
    LMI_TRY(fill_u32(b.bins, 0xffffffffu, (size_t)P * b.nbins, s));
    // every (pair, list)'s own top-15 of the list's first part
    const WideScan m1{1, nullptr, nullptr, nullptr, 0, b.bins, b.nbins, b.sub_rows, b.sub_take};
    const ScanPlan pl = scan_plan(&bd, scan.nq, scan.R, 15, scan.qmode);
    ScanCall c = scan;
    c.idx = &bd;
    c.k = 15;
    c.prefill = false;
    c.phases = kPhasePlan | kPhaseScan;
    c.wide = &m1;
    c.plan = &pl;
    LMI_TRY(bucket_topk_impl(c));
    const auto* region = reinterpret_cast<const unsigned char*>(scan.workspace);
    hipLaunchKernelGGL(kth_bound_kernel, dim3((unsigned)P), dim3(64), 0, s, (const uint64_t*)(region + pl.partial),
                       pl.list_stride, pl.split_s, (const int32_t*)(region + pl.pair_q),
                       (const int32_t*)(region + pl.pair_bucket), b.sub_first,
                       (const uint32_t*)(region + pl.split_mask), P, b.kw, idx->bucket_off, b.cap, b.bound, b.fix);
    LMI_LAUNCH_CHECK("kth_bound_kernel");
    return LMI_OK;
}

namespace {
struct WideWs {
    bool on;       // the bound + collect path (else bucket_topk_passes alone)
    int kw, cap;   // list entries produced (passes * kp); candidate slots per pair
    int lists;     // bound-scan lists per bucket (at most; bound_lists_kernel)
    int nbins;     // the bound scan's pruning bins per pair (Scan2Args::bins)
    size_t bound, fix, cls, ccount, cand, fd, fpos, frow, sub_first, sub_rows, sub_take, bins, region,
        region_bytes, total;
};

WideWs wide_ws(const lmi_index_desc* idx, int nq, int R, int k, int qmode, int ldo) {
    WideWs w{};
    int kp;
    const int np = passes_of(idx, qmode, k, &kp);
    w.kw = np * kp;
    w.on = kp == 15 && !env_config().wide_passes;  // (kp 15: the 8-wave ring)
    const size_t P = (size_t)nq * R;
    // Bound scan: 2 kw / 15 lists per bucket, so a pair's lists hold 2 kw
    // entries, each the top-15 of the first quarter of its list's rows: their
    // kw-th smallest is about the pair's 4 kw-th distance, and the collect scan
    // finds about 4 kw rows within it; 8 kw (+ 64) slots before the fix-up
    // passes take over.  Buckets of fewer lists' entries than kw but no more
    // rows than the slots are collected whole.
    w.lists = 2 * np;
    w.nbins = np;  // (np * 15 = kw)
    int cap = 256;
    while (cap < 8 * w.kw + 64) cap <<= 1;
    w.cap = std::min(cap, 8192);
    // (candidate slots past 8 GiB -- huge batches at large k -- : the passes,
    // whose lists are 8x smaller)
    w.on = w.on && P * (size_t)w.cap * 8 <= (size_t(8) << 30);
    if (!w.on) {
        w.region_bytes = w.total = passes_ws_bytes(idx, nq, R, k, qmode);
        return w;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    w.bound = take(P * 4);
    w.fix = take(P * 4);
    w.cls = take(P * 4);
    w.ccount = take(P * 4);
    w.cand = take(P * (size_t)w.cap * 8);
    w.fd = take(P * (size_t)ldo * 4);
    w.fpos = take(P * (size_t)ldo * 4);
    w.frow = take(P * (size_t)ldo * 4);
    w.sub_first = take(((size_t)idx->n_buckets + 1) * 4);
    w.sub_rows = take((size_t)idx->n_buckets * 4);
    w.sub_take = take((size_t)idx->n_buckets * 4);
    w.bins = take(P * (size_t)w.nbins * 4);
    const lmi_index_desc bd = bound_desc(idx, w.lists, nullptr);
    w.region_bytes = std::max({scan_workspace_bytes(&bd, nq, R, 15, qmode),
                               scan_workspace_bytes(idx, nq, R, 10, qmode),
                               passes_ws_bytes(idx, nq, R, k, qmode)});
    w.region = take(w.region_bytes);
    w.total = off;
    return w;
}
}  // namespace

size_t wide_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k, int qmode, int ldo) {
    return wide_ws(idx, nq, R, k, qmode, ldo).total;
}

// (c: the lists [nq*R][c.ldo] and no option but ldo)
int bucket_topk_wide(const ScanCall& c) {
    const lmi_index_desc* idx = c.idx;
    const int ldo = c.ldo;
    hipStream_t s = c.stream;
    const WideWs w = wide_ws(idx, c.nq, c.R, c.k, c.qmode, ldo);
    if (!w.on || idx->n_rows == 0) return bucket_topk_passes(c);
    if (ldo < w.kw) {
        set_error("lists of %d entries < %d", ldo, w.kw);
        return LMI_E_INVALID;
    }
    if (c.ws_bytes < w.total) {
        set_error("workspace %zu B < required %zu B", c.ws_bytes, w.total);
        return LMI_E_WORKSPACE;
    }
    if (c.nq == 0) return LMI_OK;
    const int P = c.nq * c.R;
    auto* ws = reinterpret_cast<unsigned char*>(c.workspace);
    auto* bound = (uint32_t*)(ws + w.bound);
    auto* fix = (int32_t*)(ws + w.fix);
    auto* ccount = (uint32_t*)(ws + w.ccount);
    auto* cand = (uint64_t*)(ws + w.cand);
    // the scans of all three steps: lists into scratch, the region as workspace
    // (c.ldo stays: it plays no part in a scan without prefill or merge)
    ScanCall scan = c;
    scan.out_d = (float*)(ws + w.fd);
    scan.out_pos = (int32_t*)(ws + w.fpos);
    scan.out_row = nullptr;
    scan.workspace = ws + w.region;
    scan.ws_bytes = w.region_bytes;
    // 1. every (pair, bound-pass chunk part)'s own top-15 -> each pair's bound
    LMI_TRY(sampled_bound(scan, {.lists = w.lists, .nbins = w.nbins, .kw = w.kw, .cap = w.cap,
                                 .sub_first = (int32_t*)(ws + w.sub_first), .sub_rows = (int32_t*)(ws + w.sub_rows),
                                 .sub_take = (int32_t*)(ws + w.sub_take), .bins = (uint32_t*)(ws + w.bins),
                                 .bound = bound, .fix = fix, .pad_d = c.out_d, .pad_pos = c.out_pos,
                                 .pad_row = c.out_row, .pad_ldo = ldo}));
    // 2. every row within the bound -> sorted, the first kw
    const WideScan m2{2, bound, cand, ccount, w.cap, nullptr, 0, nullptr, nullptr};
    const ScanPlan pl = scan_plan(idx, c.nq, c.R, 10, c.qmode);
    ScanCall collect = scan;
    collect.k = 10;
    collect.prefill = false;
    collect.phases = kPhasePlan | kPhaseScan;
    collect.wide = &m2;
    collect.plan = &pl;
    LMI_TRY(bucket_topk_impl(collect));
    {
        const unsigned char* region = ws + w.region;
        static std::once_flag once;
        static hipError_t attr_err = hipSuccess;
        std::call_once(once, [] {
            attr_err = hipFuncSetAttribute((const void*)collect_select_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8);
        });
        LMI_HIP_TRY(attr_err);
        hipLaunchKernelGGL(collect_select_kernel, dim3((unsigned)P), dim3(256), (size_t)w.cap * 8, s, cand,
                           ccount, w.cap, (const int32_t*)(region + pl.pair_q),
                           (const int32_t*)(region + pl.pair_bucket), idx->gpos, P, w.kw, ldo, bound, fix,
                           c.out_d, c.out_pos, c.out_row);
        LMI_LAUNCH_CHECK("collect_select_kernel");
    }
    // 3. the pairs without a bound or with too many candidates: the passes,
    //    over their buckets only (every other pair's class is -1)
    if (env_config().wide_no_fixup) return LMI_OK;
    int32_t* cls = (int32_t*)(ws + w.cls);
    hipLaunchKernelGGL(fix_classes_kernel, dim3((P + 255) / 256), dim3(256), 0, s, c.classes, fix, P, cls);
    LMI_LAUNCH_CHECK("fix_classes_kernel");
    scan.classes = cls;
    scan.out_row = c.out_row ? (int32_t*)(ws + w.frow) : nullptr;
    LMI_TRY(bucket_topk_passes(scan));
    const int64_t PL = (int64_t)P * ldo;
    hipLaunchKernelGGL(fix_combine_kernel, dim3((unsigned)((PL + 255) / 256)), dim3(256), 0, s, fix,
                       (int64_t)P, ldo, scan.out_d, scan.out_pos, scan.out_row, c.out_d, c.out_pos, c.out_row);
    LMI_LAUNCH_CHECK("fix_combine_kernel");
    return LMI_OK;
}

int bucket_topk_wide_k(const ScanCall& c) {
    if (c.phases != kPhaseAll) {
        set_error("phase flags need k <= %d (one scan pass)", LMI_MAX_K);
        return LMI_E_UNSUPPORTED;
    }
    LMI_CHECK_ARG(c.idx != nullptr, "null index");
    LMI_CHECK_ARG(c.k <= LMI_MAX_K_PASSES, "k=%d outside [1, %d]", c.k, LMI_MAX_K_PASSES);
    LMI_CHECK_ARG(c.nq >= 0 && c.R >= 1 && (int64_t)c.nq * c.R < INT32_MAX, "bad nq/R");
    if (c.nq == 0) return LMI_OK;
    LMI_CHECK_ARG(c.out_d && c.out_pos && c.workspace, "null pointer");
    int kp;
    const int ldo = passes_of(c.idx, c.qmode, c.k, &kp) * kp;
    const size_t P = (size_t)c.nq * c.R;
    const size_t lists = align_up(P * ldo * 4, 256);
    if (c.ws_bytes < 2 * lists) {
        set_error("workspace %zu B < required %zu B", c.ws_bytes, 2 * lists);
        return LMI_E_WORKSPACE;
    }
    auto* ws = reinterpret_cast<unsigned char*>(c.workspace);
    float* ld = reinterpret_cast<float*>(ws);
    int32_t* lp = reinterpret_cast<int32_t*>(ws + lists);
    LMI_TRY(bucket_topk_wide({.idx = c.idx, .q = c.q, .nq = c.nq, .ldq = c.ldq, .classes = c.classes, .R = c.R,
                              .k = c.k, .qmode = c.qmode, .out_d = ld, .out_pos = lp, .status = c.status,
                              .workspace = ws + 2 * lists, .ws_bytes = c.ws_bytes - 2 * lists,
                              .stream = c.stream, .ldo = ldo}));
    hipLaunchKernelGGL(take_k_kernel, dim3((unsigned)((P * c.k + 255) / 256)), dim3(256), 0, c.stream, ld, lp,
                       (int64_t)P, ldo, c.k, c.out_d, c.out_pos);
    LMI_LAUNCH_CHECK("take_k_kernel");
    return LMI_OK;
}
}  // namespace lmi
