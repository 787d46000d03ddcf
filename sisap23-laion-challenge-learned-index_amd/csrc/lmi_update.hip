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
//
// K9 (at the end of this file; DESIGN.md §3 "K9") is the same move with source
// and destination in ONE store that has room for the new rows
// (lmi_index_move_rows_inplace): slabs of rows in stream order, each moved
// directly or through a staging buffer.  Offered for add and remove only; a
// re-bucket (lmi_rebucket.hip) still writes a new corpus.
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
    bool inexact = false, low_norm = false;
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
            if (norm < 10.0 * 0x1p-23) {
                // under the float32 rule but not under the float64 one: the
                // float64 mode needs this row's true 1/||y|| (inv_norm64)
                low_norm |= norm >= 10.0 * 0x1p-52;
                norm = 1.0;
            }
            dst_inv[to] = (float)(1.0 / norm);
        }
    }
    if (inexact) atomicOr(status, LMI_STATUS_ROWS_NOT_F16);
    if (low_norm) atomicOr(status, LMI_STATUS_ROWS_LOW_NORM);
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

// K9 — the same update inside ONE buffer (lmi_index_move_rows_inplace; DESIGN.md
// §3 "K9").  An add shifts every old row right, a remove shifts every survivor
// left, both by an amount that does not decrease along the corpus, so the host
// cuts the shifted rows into slabs [a, b) (li.index.BucketLayout.inplace_slabs)
// and the slabs run one after the other in stream order -- an add from the end
// of the corpus backwards, a remove from the front forwards:
//
//   direct  the slab's destinations are disjoint from [a, b): one launch reads
//           the store and writes the store
//   staged  the slab is copied to the staging buffer first; a second launch
//           writes it from there to its destinations
//
// Destinations of a slab lie in its own (already staged) source range or in
// rows earlier slabs have vacated, never in rows a later slab still reads, and
// inside one launch no workgroup writes a row another one reads.  There is no
// barrier, flag or cooperative launch: the order between slabs is the stream's.
namespace lmi {
namespace {

constexpr int kCopyThreads = 256;
constexpr int kCopyMaxGrid = 4096;

// move_rows_kernel restricted to the old rows [a, b), read from `src` whose row
// 0 is old row src_row0 (the store: 0; the staging buffer: a).  src and dst may
// be the same buffer (a direct slab), so neither is __restrict__.  Before every
// write: the destination lies in [0, n_new), outside [a, b) for a direct slab,
// and on the declared side of the source row (direction > 0: right, < 0: left).
__global__ __launch_bounds__(kMoveThreads) void move_range_kernel(
    const uint4* src, const float* src_inv, int64_t src_row0, int64_t a, int64_t b, int32_t pieces,
    const int64_t* __restrict__ old_off, const int64_t* __restrict__ new_off, int32_t n_buckets,
    const int64_t* __restrict__ dropped, int64_t n_dropped, const int64_t* __restrict__ drop_before,
    uint4* dst, float* dst_inv, int64_t n_new, int32_t direction, int32_t direct,
    int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_tiles = (b - a + kMoveTileRows - 1) / kMoveTileRows;
    const int32_t total = kMoveWaveRows * pieces;  // 16-byte pieces of the wave's rows
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = a + tile * kMoveTileRows + (int64_t)wave * kMoveWaveRows;
        int64_t to = -1;
        if (lane < kMoveWaveRows && base + lane < b) {
            const int64_t i = base + lane;
            to = move_dst(i, old_off, new_off, n_buckets, dropped, n_dropped, drop_before);
            if (to >= 0) {  // (a dropped row goes nowhere)
                const bool bad = to >= n_new || (direct && to >= a && to < b) ||
                                 (direction > 0 ? to < i : to > i);
                if (bad) {  // (never, for tables and slabs that describe the update)
                    atomicOr(status, LMI_STATUS_INTERNAL);
                    to = -1;
                }
            }
            if (to >= 0) dst_inv[to] = src_inv[i - src_row0];
        }
        const uint4* s = src + (base - src_row0) * pieces;
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

// rows [0, n_rows) of src (n_pieces 16-byte pieces) and their 1/||y|| to the
// staging buffer: a contiguous copy, four loads in flight per thread
__global__ __launch_bounds__(kCopyThreads) void copy_slab_kernel(
    const uint4* __restrict__ src, const float* __restrict__ src_inv, int64_t n_pieces, int64_t n_rows,
    uint4* __restrict__ dst, float* __restrict__ dst_inv) {
    const int64_t step = (int64_t)gridDim.x * kCopyThreads * 4;
    for (int64_t q = (int64_t)blockIdx.x * kCopyThreads * 4 + threadIdx.x; q < n_pieces; q += step) {
        const bool p1 = q + kCopyThreads < n_pieces, p2 = q + 2 * kCopyThreads < n_pieces,
                   p3 = q + 3 * kCopyThreads < n_pieces;
        uint4 v0 = src[q], v1 = {}, v2 = {}, v3 = {};
        if (p1) v1 = src[q + kCopyThreads];
        if (p2) v2 = src[q + 2 * kCopyThreads];
        if (p3) v3 = src[q + 3 * kCopyThreads];
        dst[q] = v0;
        if (p1) dst[q + kCopyThreads] = v1;
        if (p2) dst[q + 2 * kCopyThreads] = v2;
        if (p3) dst[q + 3 * kCopyThreads] = v3;
    }
    for (int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x; i < n_rows;
         i += (int64_t)gridDim.x * kCopyThreads)
        dst_inv[i] = src_inv[i];
}

}  // namespace
}  // namespace lmi

extern "C" int lmi_index_move_rows_inplace(void* corpus, float* inv_norm, int64_t n_old, int64_t n_new,
                                           int64_t capacity, int32_t d_pad, const int64_t* old_off,
                                           const int64_t* new_off, int32_t n_buckets,
                                           const int64_t* dropped, int64_t n_dropped,
                                           const int64_t* drop_before, int32_t direction,
                                           const int64_t* slabs, int64_t n_slabs, void* stage_corpus,
                                           float* stage_inv_norm, int64_t stage_rows, int32_t flags,
                                           int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(direction == LMI_INPLACE_ADD || direction == LMI_INPLACE_REMOVE,
                  "move rows in place: direction=%d (LMI_INPLACE_ADD or LMI_INPLACE_REMOVE)", direction);
    LMI_CHECK_ARG((flags & ~LMI_INPLACE_MEMCPY) == 0, "move rows in place: flags=%d", flags);
    LMI_CHECK_ARG(n_old >= 0 && n_new >= 0 && n_dropped >= 0 && n_dropped <= n_old && n_slabs >= 0 &&
                      stage_rows >= 0,
                  "move rows in place: n_old=%lld n_new=%lld n_dropped=%lld n_slabs=%lld stage_rows=%lld",
                  (long long)n_old, (long long)n_new, (long long)n_dropped, (long long)n_slabs,
                  (long long)stage_rows);
    LMI_CHECK_ARG(n_old <= capacity && n_new <= capacity,
                  "move rows in place: n_old=%lld / n_new=%lld rows exceed the capacity of %lld rows",
                  (long long)n_old, (long long)n_new, (long long)capacity);
    if (direction == LMI_INPLACE_ADD)
        LMI_CHECK_ARG(n_dropped == 0 && n_new >= n_old,
                      "move rows in place: an add drops no row and does not shrink (n_dropped=%lld, "
                      "n_old=%lld, n_new=%lld)", (long long)n_dropped, (long long)n_old, (long long)n_new);
    else
        LMI_CHECK_ARG(n_new == n_old - n_dropped,
                      "move rows in place: a remove leaves n_old - n_dropped = %lld rows, n_new=%lld",
                      (long long)(n_old - n_dropped), (long long)n_new);
    LMI_CHECK_ARG(d_pad > 0 && d_pad % 32 == 0, "move rows in place: d_pad=%d (a positive multiple of 32)",
                  d_pad);
    LMI_CHECK_ARG(n_buckets >= 1, "move rows in place: n_buckets=%d", n_buckets);
    if (n_slabs == 0) return LMI_OK;  // no row moves
    LMI_CHECK_ARG(corpus && inv_norm && old_off && new_off && slabs && status,
                  "move rows in place: null pointer");
    LMI_CHECK_ARG(n_dropped == 0 || (dropped && drop_before),
                  "move rows in place: null dropped / drop_before");
    LMI_CHECK_ARG(aligned16(corpus), "move rows in place: corpus not 16-byte aligned");
    // the plan: slabs inside [0, n_old), disjoint, in the direction's order
    // (an add from the end backwards, a remove from the front forwards)
    bool any_staged = false;
    for (int64_t k = 0; k < n_slabs; ++k) {
        const int64_t a = slabs[3 * k], b = slabs[3 * k + 1], staged = slabs[3 * k + 2];
        LMI_CHECK_ARG(a >= 0 && a < b && b <= n_old && (staged == 0 || staged == 1),
                      "move rows in place: slab %lld = [%lld, %lld) staged=%lld outside [0, %lld)",
                      (long long)k, (long long)a, (long long)b, (long long)staged, (long long)n_old);
        if (k > 0) {
            const int64_t pa = slabs[3 * k - 3], pb = slabs[3 * k - 2];
            LMI_CHECK_ARG(direction == LMI_INPLACE_ADD ? b <= pa : a >= pb,
                          "move rows in place: slab %lld = [%lld, %lld) overlaps or is out of order "
                          "after [%lld, %lld)", (long long)k, (long long)a, (long long)b, (long long)pa,
                          (long long)pb);
        }
        LMI_CHECK_ARG(!staged || b - a <= stage_rows,
                      "move rows in place: staged slab %lld holds %lld rows, the staging buffer %lld",
                      (long long)k, (long long)(b - a), (long long)stage_rows);
        any_staged |= staged != 0;
    }
    LMI_CHECK_ARG(!any_staged || (stage_corpus && stage_inv_norm && aligned16(stage_corpus) &&
                                  stage_corpus != corpus && stage_inv_norm != inv_norm),
                  "move rows in place: staging buffers null, misaligned or the store itself");
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t pieces = d_pad / 8;
    uint4* const store = static_cast<uint4*>(corpus);
    uint4* const stage = static_cast<uint4*>(stage_corpus);
    for (int64_t k = 0; k < n_slabs; ++k) {
        const int64_t a = slabs[3 * k], b = slabs[3 * k + 1];
        const bool staged = slabs[3 * k + 2] != 0;
        if (staged) {
            const int64_t n_pieces = (b - a) * pieces;
            if (flags & LMI_INPLACE_MEMCPY) {
                LMI_HIP_TRY(hipMemcpyAsync(stage, store + a * pieces, (size_t)n_pieces * sizeof(uint4),
                                           hipMemcpyDeviceToDevice, s));
                LMI_HIP_TRY(hipMemcpyAsync(stage_inv_norm, inv_norm + a, (size_t)(b - a) * sizeof(float),
                                           hipMemcpyDeviceToDevice, s));
            } else {
                const int64_t per = (int64_t)kCopyThreads * 4;
                const unsigned grid = (unsigned)std::min<int64_t>((n_pieces + per - 1) / per, kCopyMaxGrid);
                hipLaunchKernelGGL(copy_slab_kernel, dim3(grid), dim3(kCopyThreads), 0, s,
                                   store + a * pieces, inv_norm + a, n_pieces, b - a, stage,
                                   stage_inv_norm);
                LMI_LAUNCH_CHECK("copy_slab_kernel");
            }
        }
        const int64_t tiles = (b - a + kMoveTileRows - 1) / kMoveTileRows;
        const unsigned grid = (unsigned)std::min<int64_t>(tiles, kMoveMaxGrid);
        hipLaunchKernelGGL(move_range_kernel, dim3(grid), dim3(kMoveThreads), 0, s,
                           staged ? stage : store, staged ? stage_inv_norm : inv_norm,
                           staged ? a : (int64_t)0, a, b, pieces, old_off, new_off, n_buckets, dropped,
                           n_dropped, drop_before, store, inv_norm, n_new, direction, staged ? 0 : 1,
                           status);
        LMI_LAUNCH_CHECK("move_range_kernel");
    }
    return LMI_OK;
}
