// The split mode's driver (gfx950; ABI 9, idx->corpus32: see include/lmi_hip.h):
// an fp16 scan of the rounded queries gives every pair a bound, a collect scan
// every row under it, and lmi_refine.hip's exact step the answer.  Every scan
// is a call of bucket_topk_impl (lmi_scan.hip).
#include "lmi_scan_internal.hpp"

#include <algorithm>
#include <cmath>

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// the split mode's kernels (bucket_topk_x below)
// ---------------------------------------------------------------------------
// One wave per query: q^ = q / |q| (float64 norm, sklearn's zero rule) rounded
// to fp16, written as float32 rows of d_pad (zero-padded) -- the fp16-exact
// queries the fp16 scan takes; float64 queries (q64) are rounded the same way.
__global__ __launch_bounds__(kThreads) void x_round_queries_kernel(const float* __restrict__ q, int32_t ldq,
                                                                   const double* __restrict__ q64,
                                                                   int32_t ldq64, int32_t nq, int32_t d,
                                                                   int32_t d_pad, float* __restrict__ out) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;
    double ss = 0.0;
    for (int e = lane; e < d; e += 64) {
        const double v = q64 ? q64[(size_t)row * ldq64 + e] : (double)q[(size_t)row * ldq + e];
        ss = fma(v, v, ss);
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    double n = sqrt(ss);
    if (n < 10.0 * 1.1920928955078125e-07) n = 1.0;
    for (int e = lane; e < d_pad; e += 64) {
        float h = 0.0f;
        if (e < d) {
            const double v = q64 ? q64[(size_t)row * ldq64 + e] : (double)q[(size_t)row * ldq + e];
            h = (float)(_Float16)(float)(v / n);
        }
        out[(size_t)row * d_pad + e] = h;
    }
}

// (+inf, -1) over every output entry (pairs whose class is out of range keep it)
__global__ __launch_bounds__(256) void x_prefill_kernel(int64_t n, void* __restrict__ out_d, int32_t out_f64,
                                                        int32_t* __restrict__ out_pos) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (out_f64) reinterpret_cast<double*>(out_d)[t] = __builtin_inf();
    else reinterpret_cast<float*>(out_d)[t] = __builtin_inff();
    out_pos[t] = -1;
}

// Per pair (by id): the collect bound d~_k + 2 eps as a distance ordinal,
// rounded up (every row whose rounded distance is at most the real sum
// passes); a list with fewer than k entries (a bucket shard of fewer rows)
// collects its whole shard.
__global__ __launch_bounds__(256) void x_bound_kernel(int64_t P, int32_t k, const float* __restrict__ ld,
                                                      double two_eps, uint32_t* __restrict__ bound_ord) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float dk = ld[(size_t)p * k + k - 1];
    if (!(dk < __builtin_inff())) {
        bound_ord[p] = 0xffffffffu;
        return;
    }
    const double b = (double)dk + two_eps;
    const float f = (float)b;
    // (the ordinal of the next float up when the float rounded the sum down)
    bound_ord[p] = f2ord(f) + ((double)f < b ? 1u : 0u);
}

// The split mode's sampled bound (k <= 15): the kw-th distance ordinal of the
// pair's sampled lists (kth_bound_kernel) + 2 eps, rounded up; all ones (a
// bucket collected whole) and 0 (no bound: fix[p], the whole shard exactly)
// stay as they are.
__global__ __launch_bounds__(256) void x_margin_kernel(int64_t P, double two_eps, uint32_t* __restrict__ bound_ord) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const uint32_t b = bound_ord[p];
    if (b == 0u || b == 0xffffffffu) return;
    const double v = (double)ord2f(b) + two_eps;
    const float f = (float)v;
    bound_ord[p] = f2ord(f) + ((double)f < v ? 1u : 0u);
}

// The split mode's sample (k <= 10): a descriptor of 2C buckets over the same
// rows -- bucket 2c = the first s_c rows of bucket c, s_c = min(n_c,
// max(chunk_rows, n_c / kXSampleDiv rounded up to 32 rows)), bucket 2c + 1 =
// the rest (no chunks, never probed) -- so the product scan gives every pair
// the k-th of its bucket's sample, an upper bound of its own (and the collect
// then finds about k n_c / s_c <= k kXSampleDiv rows under it, far inside
// its buffer at any bucket size).
//
// The collect scan's descriptor (x_collect_desc) skips the sample where it is
// at most a quarter of the bucket (LMI_X_SKIP_SHARE): bucket 2c = the sample (no chunks, never
// probed), 2c + 1 = the rest; a bucket with a larger sample is collected whole
// (2c empty, 2c + 1 = the bucket).  The skipped rows' candidates are the
// sample scan's own list (set_bound_kernel appends it): every skipped row the
// select needs is in it unless the pair's band reaches the sample's k-th
// (x_select_wave_kernel checks; 0.03% of the pairs on the 10M mixture,
// tools/x_sample_cover.py), and those pairs are scored exactly over their
// sample rows and candidates (x_fallback_kernel).
constexpr int kXSampleDiv = 16;
__global__ __launch_bounds__(64) void x_sample_desc_kernel(const int64_t* __restrict__ bucket_off, int32_t C,
                                                           int64_t chunk_rows, const int32_t* __restrict__ classes,
                                                           int32_t P, int64_t* __restrict__ off2,
                                                           int32_t* __restrict__ cf2, int32_t* __restrict__ classes2,
                                                           int64_t* __restrict__ off2b, int32_t* __restrict__ cf2b,
                                                           int32_t* __restrict__ classes2b, int32_t skip_share) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t nch = 0, nchb = 0;
        for (int c = 0; c < C; ++c) {
            const int64_t a = bucket_off[c], n = bucket_off[c + 1] - a;
            const int64_t want = std::max(chunk_rows, (n / kXSampleDiv + 31) / 32 * 32);
            const int64_t sc = n < want ? n : want;
            off2[2 * c] = a;
            off2[2 * c + 1] = a + sc;
            cf2[2 * c] = nch;
            nch += (int32_t)((sc + chunk_rows - 1) / chunk_rows);
            cf2[2 * c + 1] = nch;
            // (a sample of at most 1 / skip_share of the bucket, LMI_X_SKIP_SHARE)
            const int64_t skip = (skip_share > 0 && sc < n && sc * skip_share <= n) ? sc : 0;
            off2b[2 * c] = a;
            off2b[2 * c + 1] = a + skip;
            cf2b[2 * c] = nchb;
            cf2b[2 * c + 1] = nchb;
            nchb += (int32_t)((n - skip + chunk_rows - 1) / chunk_rows);
        }
        off2[2 * C] = bucket_off[C];
        cf2[2 * C] = nch;
        off2b[2 * C] = bucket_off[C];
        cf2b[2 * C] = nchb;
    }
    for (int i = blockIdx.x * 64 + threadIdx.x; i < P; i += gridDim.x * 64) {
        const int32_t c = classes[i];
        classes2[i] = c < 0 ? c : (c < C ? 2 * c : 2 * C);
        classes2b[i] = c < 0 ? c : (c < C ? 2 * c + 1 : 2 * C);
    }
}

}  // namespace


// |d~ - d| for every (query, row) of the split mode, d~ the fp16 scan's
// distance on the normalised, fp16-rounded vectors and d the exact one:
// rounding a unit vector to fp16 moves it by delta <= 2^-11 (relative, normal
// range; + 2^-22 for the float32 step before it) + sqrt(d) 2^-25 (absolute,
// the subnormal range), i.e. by an angle <= asin(delta); the angle between
// query and row moves by at most the two angles, and a cosine by at most the
// angle.  Plus the fp16 scan's own arithmetic on the rounded vectors
// (refine_eps of li/index.py, the fp16 path: gamma(2 (d_pad/16 + 16)) for the
// dot, the two norms, the scale and the final fma) and 2^-24 for rounding the
// exact value to float32 (ties of the rounded values then order by position).
double split_eps(int d_pad) {
    const double u = std::ldexp(1.0, -24);
    auto gamma = [&](double n) { return n * u / (1.0 - n * u); };
    const double delta = std::ldexp(1.0, -11) + std::ldexp(1.0, -22) + std::sqrt((double)d_pad) * std::ldexp(1.0, -25);
    const double h = 2.0 * (d_pad / 16 + 16), hq = 4.0 * ((d_pad + 255) / 256) + 6.0;
    const double scan = gamma(h) + gamma(2 * hq) / 2 + 4 * u + u + 2 * u + 2 * u;
    return 2.0 * std::asin(delta) + scan + u;
}

namespace {
struct XWs {
    size_t qr, ld, lpos, srow, bound, ccount, cand, failed, nfailed, wgl, sfl, spd, spg, fix, bins, sub_first, sub_rows, sub_take,
        off2, cf2, classes2, off2b, cf2b, classes2b, qn32, grp, tailq, goff, region, region_bytes, region_s,
        region_s_bytes, total;
    int32_t cap;
};
// k <= 10: the k-th of a per-bucket sample (the product scan over
// x_sample_desc); the device tables are filled by x_sample_desc_kernel
inline bool x_sample(int k) { return k <= 10; }
lmi_index_desc x_sample_desc(const lmi_index_desc* idx, const int64_t* off2, const int32_t* cf2) {
    lmi_index_desc d = *idx;
    d.n_buckets = 2 * idx->n_buckets;
    d.bucket_off = off2;
    d.chunk_first = cf2;
    // (host-side bounds for the workspace: a sample of at most n_c / 16 + 32
    // rows beyond one chunk)
    d.max_chunks = 2 + std::max(idx->max_chunks, 1) / kXSampleDiv;
    d.n_chunks = idx->n_buckets * d.max_chunks;
    d.chunk_centroid = nullptr;
    return d;
}
// the collect scan's: the rest of every bucket whose sample is skipped, the
// others whole (x_sample_desc_kernel)
lmi_index_desc x_collect_desc(const lmi_index_desc* idx, const int64_t* off2b, const int32_t* cf2b) {
    lmi_index_desc d = *idx;
    d.n_buckets = 2 * idx->n_buckets;
    d.bucket_off = off2b;
    d.chunk_first = cf2b;
    d.chunk_centroid = nullptr;
    return d;
}
// k <= 15: the k-th comes from a sampled bound scan (the wide path's chunk-list
// scan over two lists per bucket, each the first quarter of its rows), not a
// whole first scan
constexpr int kXLists = 2;
inline bool x_sampled(int k) { return k <= 15; }

XWs x_ws(const lmi_index_desc* idx, int nq, int R, int k) {
    XWs w{};
    const size_t P = (size_t)nq * R;
    // collect slots per pair: 2048 (the rows within 2 eps of the k-th, ~20 on
    // the clip768-like mixture), fewer for huge batches (<= 2 GiB of slots)
    int cap = 2048;
    while (cap > 256 && P * (size_t)cap * 8 > (size_t(2) << 30)) cap >>= 1;
    w.cap = cap;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    w.qr = take((size_t)nq * idx->d_pad * 4);
    w.ld = take(P * std::max(k, 15) * 4);
    w.lpos = take(P * std::max(k, 15) * 4);
    w.srow = take(P * std::max(k, 15) * 4);
    w.fix = take(P * 4);
    w.bins = take(P * 4);
    w.sub_first = take(((size_t)idx->n_buckets + 1) * 4);
    w.sub_rows = take((size_t)idx->n_buckets * 4);
    w.sub_take = take((size_t)idx->n_buckets * 4);
    w.off2 = take(((size_t)2 * idx->n_buckets + 1) * 8);
    w.cf2 = take(((size_t)2 * idx->n_buckets + 1) * 4);
    w.classes2 = take(P * 4);
    w.off2b = take(((size_t)2 * idx->n_buckets + 1) * 8);
    w.cf2b = take(((size_t)2 * idx->n_buckets + 1) * 4);
    w.classes2b = take(P * 4);
    w.qn32 = take((size_t)nq * idx->d_pad * 4);
    w.grp = take((size_t)R * idx->n_buckets * 4);
    w.tailq = take(P);
    w.goff = take(((size_t)idx->n_buckets + 1) * 8);
    w.bound = take(P * 4);
    w.ccount = take(P * 4);
    w.cand = take(P * (size_t)cap * 8);
    w.failed = take(P * 4);
    w.nfailed = take(256);  // (word 0: the failed pairs; word 8: the sfl pairs; word 16: the wgl pairs)
    w.wgl = take(P * 4);
    w.sfl = take(P * 4);
    // (the sliced sample fallback's lists)
    w.spd = take((size_t)kXSlicedPairs * kXSlices * k * 8);
    w.spg = take((size_t)kXSlicedPairs * kXSlices * k * 4);
    const lmi_index_desc bd = bound_desc(idx, kXLists, nullptr);
    const lmi_index_desc sd = x_sample_desc(idx, nullptr, nullptr);
    const lmi_index_desc cd = x_collect_desc(idx, nullptr, nullptr);
    w.region_bytes = std::max({scan_plan(idx, nq, R, k, LMI_Q_F16).total, scan_plan(idx, nq, R, 10, LMI_Q_F16).total,
                               scan_plan(&bd, nq, R, 15, LMI_Q_F16).total, scan_plan(&sd, nq, R, k, LMI_Q_F16).total,
                               scan_plan(&cd, nq, R, 10, LMI_Q_F16).total});
    w.region = take(w.region_bytes);
    // k <= 10: the sample scan's own region (ABI 11), so the plans of both
    // scans are laid down in one PLAN phase and the batch stream can run the
    // phases of one batch apart
    if (x_sample(k)) {
        w.region_s_bytes = scan_plan(&sd, nq, R, k, LMI_Q_F16).total;
        w.region_s = take(w.region_s_bytes);
    }
    w.total = off;
    return w;
}
}  // namespace

size_t x_ws_bytes(const lmi_index_desc* idx, int nq, int R, int k) { return x_ws(idx, nq, R, k).total; }
size_t x_nfailed_offset(const lmi_index_desc* idx, int nq, int R, int k) { return x_ws(idx, nq, R, k).nfailed; }

// The split mode: see lmi_index_desc.corpus32 (include/lmi_hip.h).  out_d is
// float (out_f64 = 0) or double [nq*R][k]; qmode is ignored (the queries are
// rounded here whatever their class).
int bucket_topk_x(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq, const double* q64,
                  int32_t ldq64, const int32_t* classes, int32_t R, int32_t k, void* out_d, int out_f64,
                  int32_t* out_pos, int32_t* status, void* workspace, size_t ws_bytes, hipStream_t s,
                  int phases) {
    LMI_CHECK_ARG(idx != nullptr, "null index");
    LMI_CHECK_ARG(idx->corpus32 != nullptr && idx->dtype == LMI_F16 && idx->d_pad == v2::D,
                  "split mode needs corpus32, an fp16 scan corpus and d_pad %d", v2::D);
    LMI_CHECK_ARG(k >= 1 && k <= LMI_MAX_K, "split mode: k=%d outside [1, %d]", k, LMI_MAX_K);
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < INT32_MAX, "bad nq/R");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG((q || q64) && classes && out_d && out_pos && status && workspace, "null pointer");
    LMI_CHECK_ARG(q64 ? ldq64 >= idx->d : ldq >= idx->d, "ldq < d");
    if (phases != kPhaseAll && !x_sample(k)) {
        set_error("split mode: phase flags need k <= 10 (the sample's bound)");
        return LMI_E_UNSUPPORTED;
    }
    const XWs w = x_ws(idx, nq, R, k);
    if (ws_bytes < w.total) {
        set_error("workspace %zu B < required %zu B", ws_bytes, w.total);
        return LMI_E_WORKSPACE;
    }
    const int P = nq * R;
    auto* ws = reinterpret_cast<unsigned char*>(workspace);
    float* qr = (float*)(ws + w.qr);
    float* ld = (float*)(ws + w.ld);
    int32_t* lpos = (int32_t*)(ws + w.lpos);
    auto* bound = (uint32_t*)(ws + w.bound);
    auto* ccount = (uint32_t*)(ws + w.ccount);
    auto* cand = (uint64_t*)(ws + w.cand);
    unsigned char* region = ws + w.region;
    const double two_eps = 2.0 * split_eps(idx->d_pad);
    const bool sampled = x_sampled(k);
    int32_t* fix = (int32_t*)(ws + w.fix);
    WideScan m2{2, bound, cand, ccount, w.cap, nullptr, 0, nullptr, nullptr};
    int32_t* srow = (int32_t*)(ws + w.srow);
    auto* off2b = (int64_t*)(ws + w.off2b);
    const lmi_index_desc cd = x_collect_desc(idx, off2b, (int32_t*)(ws + w.cf2b));
    // the scans: the rounded queries, lists into ld / lpos, the region
    const ScanCall whole{.idx = idx, .q = qr, .nq = nq, .ldq = idx->d_pad, .classes = classes, .R = R, .k = k,
                         .qmode = LMI_Q_F16, .out_d = ld, .out_pos = lpos, .status = status, .workspace = region,
                         .ws_bytes = w.region_bytes, .stream = s};
    // the collect scan (as the wide path's) and its plan: step 3 reads its
    // grouped pairs and counts from the region
    const ScanPlan l = scan_plan(x_sample(k) ? &cd : idx, nq, R, 10, LMI_Q_F16);
    ScanCall collect = whole;
    collect.k = 10;
    collect.prefill = false;
    collect.wide = &m2;
    collect.plan = &l;
    if (phases & kPhasePlan) {  // (k > 10: every phase, checked above)
        hipLaunchKernelGGL(x_round_queries_kernel, dim3((nq + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads),
                           0, s, q, ldq, q64, ldq64, nq, idx->d, idx->d_pad, qr);
        LMI_LAUNCH_CHECK("x_round_queries_kernel");
        LMI_TRY(fill_u32(ws + w.nfailed, 0u, 32, s));
    }
    if (x_sample(k)) {
        // (PLAN: the rounded queries and both scans' plans; SCAN: the sample
        // scan and its merge, the bound, the collect scan; MERGE: step 3)
        auto* off2 = (int64_t*)(ws + w.off2);
        auto* cf2 = (int32_t*)(ws + w.cf2);
        auto* classes2 = (int32_t*)(ws + w.classes2);
        const lmi_index_desc sd = x_sample_desc(idx, off2, cf2);
        auto* classes2b = (int32_t*)(ws + w.classes2b);
        // the sample scan: the product scan over the 2C-bucket sample
        // descriptor, in its own region
        ScanCall sample = whole;
        sample.idx = &sd;
        sample.classes = classes2;
        sample.out_row = srow;
        sample.workspace = ws + w.region_s;
        sample.ws_bytes = w.region_s_bytes;
        // (the collect skips the samples it can: their candidates are the
        // sample scan's lists, appended by set_bound_kernel)
        collect.idx = &cd;
        collect.classes = classes2b;
        m2.app_d = ld;
        m2.app_row = srow;
        m2.app_k = k;
        if (phases & kPhasePlan) {
            hipLaunchKernelGGL(x_sample_desc_kernel, dim3((unsigned)std::min(1024, (P + 63) / 64)), dim3(64), 0, s,
                               idx->bucket_off, idx->n_buckets, (int64_t)idx->chunk_rows, classes, P, off2, cf2,
                               classes2, off2b, (int32_t*)(ws + w.cf2b), classes2b,
                               std::max(0, env_config().x_skip));
            LMI_LAUNCH_CHECK("x_sample_desc_kernel");
            sample.phases = collect.phases = kPhasePlan;
            LMI_TRY(bucket_topk_impl(sample));
            LMI_TRY(bucket_topk_impl(collect));
        }
        if (phases & kPhaseScan) {
            // 1. the k-th of every pair's bucket sample (its first chunk_rows
            //    rows), then that k-th + 2 eps as the collect bound
            sample.phases = kPhaseScan | kPhaseMerge;
            LMI_TRY(bucket_topk_impl(sample));
            hipLaunchKernelGGL(x_bound_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (int64_t)P, k, ld, two_eps,
                               bound);
            LMI_LAUNCH_CHECK("x_bound_kernel");
            // 2. every row under the bound, over the rest of the buckets whose
            //    sample the collect skips
            collect.phases = kPhaseScan;
            LMI_TRY(bucket_topk_impl(collect));
        }
        if (!(phases & kPhaseMerge)) return LMI_OK;
    } else {
        if (sampled) {
            // 1. a bound per pair from a sample: the wide path's chunk-list scan
            //    (two lists per bucket, each scanning the first quarter of its
            //    rows, every list its part's own top-15), the 15th smallest entry
            //    (>= the pair's 15th >= its k-th), + 2 eps
            LMI_TRY(sampled_bound(whole, {.lists = kXLists, .nbins = 1, .kw = 15, .cap = w.cap,
                                          .sub_first = (int32_t*)(ws + w.sub_first),
                                          .sub_rows = (int32_t*)(ws + w.sub_rows),
                                          .sub_take = (int32_t*)(ws + w.sub_take), .bins = (uint32_t*)(ws + w.bins),
                                          .bound = bound, .fix = fix}));
            hipLaunchKernelGGL(x_margin_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (int64_t)P, two_eps, bound);
            LMI_LAUNCH_CHECK("x_margin_kernel");
        } else {
            // 1. the fp16 scan on the rounded vectors: every pair's approximate k-th
            LMI_TRY(bucket_topk_impl(whole));
            hipLaunchKernelGGL(x_bound_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (int64_t)P, k, ld, two_eps,
                               bound);
            LMI_LAUNCH_CHECK("x_bound_kernel");
        }
        // 2. every row under the bound
        collect.phases = kPhasePlan | kPhaseScan;
        LMI_TRY(bucket_topk_impl(collect));
    }
    // 3. the candidates' exact distances, sorted; overflowed pairs whole
    XArgs a{};
    a.rows32 = idx->corpus32;
    a.rows32n = idx->corpus32n;
    a.rows64 = out_f64 ? idx->corpus64 : nullptr;
    a.d = idx->d;
    a.d_pad = idx->d_pad;
    a.gpos = idx->gpos;
    a.bucket_off = idx->bucket_off;
    a.n_rows = idx->n_rows;
    a.q = q;
    a.ldq = ldq;
    a.q64 = out_f64 ? q64 : nullptr;
    a.ldq64 = ldq64;
    if (!a.q64 && !q) {
        set_error("split mode: float32 output needs the float32 queries");
        return LMI_E_INVALID;
    }
    a.classes = classes;
    a.nq = nq;
    a.R = R;
    a.k = k;
    a.pair_q = (const int32_t*)(region + l.pair_q);
    a.pair_bucket = (const int32_t*)(region + l.pair_bucket);
    a.cand = cand;
    a.ccount = ccount;
    a.cap = w.cap;
    a.out_d = out_d;
    a.out_f64 = out_f64;
    a.out_pos = out_pos;
    a.failed = (int32_t*)(ws + w.failed);
    a.n_failed = (int32_t*)(ws + w.nfailed);
    a.wgl = sampled ? (int32_t*)(ws + w.wgl) : nullptr;  // (two_eps > 0: the wave kernel runs)
    a.n_wgl = (int32_t*)(ws + w.nfailed) + 16;
    a.status = status;
    a.two_eps = sampled ? two_eps : 0.0;
    a.fix = sampled && !x_sample(k) ? fix : nullptr;
    // (ABI 10: the float32 output in the reference's own float32 order)
    a.qn32 = (!out_f64 && q) ? (const float*)(ws + w.qn32) : nullptr;
    a.grp = (const int32_t*)(ws + w.grp);
    a.nrows_c = idx->bucket_rows;
    a.C = idx->n_buckets;
    a.tailq = (const uint8_t*)(ws + w.tailq);
    a.goff = (const int64_t*)(ws + w.goff);
    a.plan_counts = (const int32_t*)(region + l.counts);
    a.plan_cm = x_sample(k) ? 2 : 1;
    if (x_sample(k)) {
        a.soff = off2b;
        a.skth = ld;
        a.sfailed = (int32_t*)(ws + w.sfl);
        a.n_sfailed = (int32_t*)(ws + w.nfailed) + 8;
        a.spd = (double*)(ws + w.spd);
        a.spg = (int32_t*)(ws + w.spg);
    }
    // (pairs whose class is out of range keep the prefill of step 1's prep:
    // the outputs are prefilled here, by pair id, in step 3's own buffers)
    hipLaunchKernelGGL(x_prefill_kernel, dim3((unsigned)(((int64_t)P * k + 255) / 256)), dim3(256), 0, s,
                       (int64_t)P * k, out_d, out_f64, out_pos);
    LMI_LAUNCH_CHECK("x_prefill_kernel");
    return launch_x_refine(a, P, s);
}
}  // namespace lmi

extern "C" double lmi_split_eps(int32_t d_pad) { return d_pad > 0 ? lmi::split_eps(d_pad) : 0.0; }
