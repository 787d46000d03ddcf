// K7 — index update: the row movement behind DeviceIndex.add / remove
// (lmi_index_move_rows, lmi_index_ingest_rows; DESIGN.md §3 "K7").
//
// An update writes a NEW bucket-sorted corpus next to the old one: the
// surviving rows of every bucket keep their order and are followed by the
// bucket's new rows in batch order (the reference's groupby visit order over
// the concatenated frame, LearnedIndex.py:143-145).  The host prepares the
// offsets (O(buckets + batch + removals)); these two kernels move the bytes.
//
//   move    old row i of bucket c -> new_off[c] + (i - old_off[c])
//                                    - #dropped rows of c before i
//           one read and one write of the corpus inside HBM, 16 bytes per lane
//   ingest  batch row j -> new_dst[j]: fp32 -> fp16 (or fp16 as it is), zero
//           padding to d_pad, 1/||y|| from the stored values in float64
//
// Every destination row is checked against [0, n_new) before it is written;
// a row that fails is skipped and LMI_STATUS_INTERNAL is raised.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "lmi_common.hpp"

namespace lmi {
namespace {

constexpr int kMoveThreads = 256;                    // 4 waves
constexpr int kMoveWaveRows = 8;                     // rows a wave moves per pass
constexpr int kMoveTileRows = kMoveWaveRows * (kMoveThreads / 64);  // 32 rows per workgroup
constexpr int kMoveMaxGrid = 2048;                   // grid cap: the rest is grid-strided
constexpr int kIngestThreads = 256;
constexpr int kIngestMaxGrid = 2048;

// first index in a[0..n) whose value is >= v (n when none)
__device__ inline int64_t lower_bound_i64(const int64_t* __restrict__ a, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Destination of old row i (-1: dropped).  off[c] <= i < off[c+1] picks the
// bucket (empty buckets share an offset: the LAST c with off[c] <= i).
__device__ inline int64_t move_dst(int64_t i, const int64_t* __restrict__ old_off,
                                   const int64_t* __restrict__ new_off, int32_t n_buckets,
                                   const int64_t* __restrict__ dropped, int64_t n_dropped,
                                   const int64_t* __restrict__ drop_before) {
    // c = (first index in old_off[1..C] with value > i) = upper bound
    int32_t lo = 0, hi = n_buckets;  // invariant: old_off[lo] <= i < old_off[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (old_off[mid] <= i) lo = mid; else hi = mid;
    }
    const int32_t c = lo;
    int64_t before = 0;
    if (n_dropped > 0) {
        const int64_t k = lower_bound_i64(dropped, n_dropped, i);
        if (k < n_dropped && dropped[k] == i) return -1;
        before = k - drop_before[c];
    }
    return new_off[c] + (i - old_off[c]) - before;
}

// One wave moves kMoveWaveRows consecutive old rows per pass: lane l < 8 finds
// the destination of row base + l (two binary searches, all lanes at once),
// then the wave's lanes stride over the rows' 16-byte pieces -- the source is
// one contiguous stream, the destination contiguous inside every run of
// surviving rows of a bucket.  `pieces` = d_pad * 2 / 16 per row.
__global__ __launch_bounds__(kMoveThreads) void move_rows_kernel(
    const uint4* __restrict__ src, const float* __restrict__ src_inv, int64_t n_old, int32_t pieces,
    const int64_t* __restrict__ old_off, const int64_t* __restrict__ new_off, int32_t n_buckets,
    const int64_t* __restrict__ dropped, int64_t n_dropped, const int64_t* __restrict__ drop_before,
    uint4* __restrict__ dst, float* __restrict__ dst_inv, int64_t n_new, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_tiles = (n_old + kMoveTileRows - 1) / kMoveTileRows;
    const int32_t total = kMoveWaveRows * pieces;  // 16-byte pieces of the wave's rows
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kMoveTileRows + (int64_t)wave * kMoveWaveRows;
        int64_t to = -1;
        if (lane < kMoveWaveRows && base + lane < n_old) {
            to = move_dst(base + lane, old_off, new_off, n_buckets, dropped, n_dropped, drop_before);
            if (to >= n_new) {  // (never, for offsets that describe the layouts)
                atomicOr(status, LMI_STATUS_INTERNAL);
                to = -1;
            }
            if (to >= 0) dst_inv[to] = src_inv[base + lane];
        }
        const uint4* __restrict__ s = src + base * pieces;
        // four 16-byte loads in flight per lane before the first store
        for (int32_t q0 = lane; q0 < total + lane; q0 += 4 * 64) {
            // (named registers, not arrays: no staging through LDS or scratch)
            auto at = [&](int32_t q) -> int64_t {  // piece q's place in dst, -1: none
                const int32_t r = q < total ? q / pieces : 0;
                const int64_t t = __shfl(to, r);   // (every lane takes part)
                return (q < total && t >= 0) ? t * pieces + (q - r * pieces) : -1;
            };
            const int64_t a0 = at(q0), a1 = at(q0 + 64), a2 = at(q0 + 128), a3 = at(q0 + 192);
            uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
            if (a0 >= 0) v0 = s[q0];
            if (a1 >= 0) v1 = s[q0 + 64];
            if (a2 >= 0) v2 = s[q0 + 128];
            if (a3 >= 0) v3 = s[q0 + 192];
            if (a0 >= 0) dst[a0] = v0;
            if (a1 >= 0) dst[a1] = v1;
            if (a2 >= 0) dst[a2] = v2;
            if (a3 >= 0) dst[a3] = v3;
        }
    }
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per batch row (grid-strided): lanes stride over the row's groups
// of 8 columns, convert, pad, sum the squares of the STORED values in float64
// and write 16 bytes each.  vec: the source rows take 16-byte loads (base and
// stride aligned); columns >= d read as zero either way.
template <typename T>
__global__ __launch_bounds__(kIngestThreads) void ingest_rows_kernel(
    const T* __restrict__ rows, int64_t m, int64_t ld, int32_t d, int32_t d_pad, int32_t vec,
    const int64_t* __restrict__ new_dst, uint4* __restrict__ dst, float* __restrict__ dst_inv,
    int64_t n_new, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (kIngestThreads / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kIngestThreads / 64);
    const int32_t pieces = d_pad / 8;
    bool inexact = false;
    for (int64_t j = wave0; j < m; j += n_waves) {
        const int64_t to = new_dst[j];
        if (to < 0 || to >= n_new) {
            if (lane == 0) atomicOr(status, LMI_STATUS_INTERNAL);
            continue;
        }
        const T* __restrict__ row = rows + j * ld;
        double acc = 0.0;
        for (int32_t p = lane; p < pieces; p += 64) {
            const int32_t c0 = p * 8;
            union { uint4 v; unsigned short h[8]; } o;  // fp16 bits
            if constexpr (sizeof(T) == 2) {
                if (vec && c0 + 8 <= d) {
                    o.v = *reinterpret_cast<const uint4*>(row + c0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        o.h[e] = c0 + e < d ? __half_as_ushort(row[c0 + e]) : (unsigned short)0;
                }
            } else {
                float f[8];
                if (vec && c0 + 8 <= d) {
                    const float4 a = *reinterpret_cast<const float4*>(row + c0);
                    const float4 b = *reinterpret_cast<const float4*>(row + c0 + 4);
                    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
                    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = c0 + e < d ? row[c0 + e] : 0.0f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const __half h = __float2half_rn(f[e]);
                    o.h[e] = __half_as_ushort(h);
                    inexact |= !(__half2float(h) == f[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double v = (double)__half2float(__ushort_as_half(o.h[e]));
                acc += v * v;
            }
            dst[to * pieces + p] = o.v;
        }
        // _inv_norm's rule: float64 norm of the stored values, norms below
        // 10 eps(float32) count as 1, one rounding to float32
        acc = wave_sum(acc);
        if (lane == 0) {
            double norm = sqrt(acc);
            if (norm < 10.0 * 0x1p-23) norm = 1.0;
            dst_inv[to] = (float)(1.0 / norm);
        }
    }
    if (inexact) atomicOr(status, LMI_STATUS_ROWS_NOT_F16);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace lmi

extern "C" int lmi_index_move_rows(const void* src_corpus, const float* src_inv_norm, int64_t n_old,
                                   int32_t d_pad, const int64_t* old_off, const int64_t* new_off,
                                   int32_t n_buckets, const int64_t* dropped, int64_t n_dropped,
                                   const int64_t* drop_before, void* dst_corpus, float* dst_inv_norm,
                                   int64_t n_new, int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(n_old >= 0 && n_new >= 0 && n_dropped >= 0 && n_dropped <= n_old,
                  "move rows: n_old=%lld n_new=%lld n_dropped=%lld", (long long)n_old, (long long)n_new,
                  (long long)n_dropped);
    LMI_CHECK_ARG(n_new >= n_old - n_dropped, "move rows: n_new=%lld holds fewer than the %lld survivors",
                  (long long)n_new, (long long)(n_old - n_dropped));
    LMI_CHECK_ARG(d_pad > 0 && d_pad % 32 == 0, "move rows: d_pad=%d (a positive multiple of 32)", d_pad);
    LMI_CHECK_ARG(n_buckets >= 1, "move rows: n_buckets=%d", n_buckets);
    if (n_old == 0 || n_old == n_dropped) return LMI_OK;  // nothing survives: nothing to move
    LMI_CHECK_ARG(src_corpus && src_inv_norm && old_off && new_off && dst_corpus && dst_inv_norm && status,
                  "move rows: null pointer");
    LMI_CHECK_ARG(n_dropped == 0 || (dropped && drop_before), "move rows: null dropped / drop_before");
    LMI_CHECK_ARG(src_corpus != dst_corpus && src_inv_norm != dst_inv_norm,
                  "move rows: source and destination must be different buffers");
    LMI_CHECK_ARG(aligned16(src_corpus) && aligned16(dst_corpus), "move rows: corpus not 16-byte aligned");
    const int64_t tiles = (n_old + kMoveTileRows - 1) / kMoveTileRows;
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, kMoveMaxGrid);
    hipLaunchKernelGGL(move_rows_kernel, dim3(grid), dim3(kMoveThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint4*>(src_corpus),
                       src_inv_norm, n_old, d_pad / 8, old_off, new_off, n_buckets, dropped, n_dropped,
                       drop_before, static_cast<uint4*>(dst_corpus), dst_inv_norm, n_new, status);
    LMI_LAUNCH_CHECK("move_rows_kernel");
    return LMI_OK;
}

extern "C" int lmi_index_ingest_rows(const void* rows, int32_t dtype, int64_t m, int64_t ld, int32_t d,
                                     int32_t d_pad, const int64_t* new_dst, void* dst_corpus,
                                     float* dst_inv_norm, int64_t n_new, int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(dtype == LMI_F16 || dtype == LMI_F32, "ingest rows: dtype=%d (LMI_F16 or LMI_F32)", dtype);
    LMI_CHECK_ARG(m >= 0 && n_new >= m, "ingest rows: m=%lld n_new=%lld", (long long)m, (long long)n_new);
    LMI_CHECK_ARG(d > 0 && d_pad >= d && d_pad % 32 == 0 && d_pad - d < 32,
                  "ingest rows: d=%d d_pad=%d (d rounded up to a multiple of 32)", d, d_pad);
    LMI_CHECK_ARG(ld >= d, "ingest rows: ld=%lld < d=%d", (long long)ld, d);
    if (m == 0) return LMI_OK;
    LMI_CHECK_ARG(rows && new_dst && dst_corpus && dst_inv_norm && status, "ingest rows: null pointer");
    LMI_CHECK_ARG(aligned16(dst_corpus), "ingest rows: corpus not 16-byte aligned");
    const int64_t el = dtype == LMI_F16 ? 2 : 4;
    const int32_t vec = aligned16(rows) && (ld * el) % 16 == 0;
    const unsigned grid = (unsigned)std::min<int64_t>((m + kIngestThreads / 64 - 1) / (kIngestThreads / 64),
                                                      kIngestMaxGrid);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == LMI_F16) {
        hipLaunchKernelGGL(ingest_rows_kernel<__half>, dim3(grid), dim3(kIngestThreads), 0, s,
                           static_cast<const __half*>(rows), m, ld, d, d_pad, vec, new_dst,
                           static_cast<uint4*>(dst_corpus), dst_inv_norm, n_new, status);
    } else {
        hipLaunchKernelGGL(ingest_rows_kernel<float>, dim3(grid), dim3(kIngestThreads), 0, s,
                           static_cast<const float*>(rows), m, ld, d, d_pad, vec, new_dst,
                           static_cast<uint4*>(dst_corpus), dst_inv_norm, n_new, status);
    }
    LMI_LAUNCH_CHECK("ingest_rows_kernel");
    return LMI_OK;
}
