// K8 -- index re-bucket: the kernels behind DeviceIndex.relabel
// (lmi_bucket_sort_labels, lmi_index_gather_rows; DESIGN.md §3 "K8").
//
// A relabel gives every row of the index's row sequence a new bucket.  The new
// index is a permutation of the old one, made inside HBM:
//
//   sort    order[p] = the sequence row at new position p: the stable sort of
//           the labels (np.argsort(kind="stable")), as a counting sort --
//           every wave owns one interval of the sequence, so "rows of lower
//           waves first, then lower groups of 64, then lower lanes" is the
//           stable order:
//             hist   per-wave histogram in LDS -> counts[c][wave]
//             scan   rows of counts -> every wave's start inside every
//                    bucket, the bucket totals -> bucket_off
//             place  every wave walks its interval again, 64 labels at a
//                    time; a lane's rank among the equal labels of lower
//                    lanes is popc(ballot(label == c) & lanes below), found
//                    in a loop over the distinct labels of the 64; the
//                    wave's LDS cursor of c then moves on by the match count
//           (no atomic hands out a rank: atomics are not order-stable)
//   gather  dst row p = src row src_pos[p], destination-major: a wave writes
//           8 consecutive destination rows as one contiguous stream, 16
//           bytes per lane, and reads 8 whole source rows
//
// A label outside [0, n_buckets) writes nothing and raises
// LMI_STATUS_BAD_LABEL; a src_pos outside [0, n_src) skips the row and raises
// LMI_STATUS_INTERNAL.
#include <algorithm>

#include "lmi_common.hpp"

namespace lmi {
namespace {

constexpr int kSortThreads = 256;                    // 4 waves
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortMaxWaves = LMI_REBUCKET_MAX_WAVES;  // cap: the intervals grow instead
constexpr int kRebucketMaxBuckets = LMI_REBUCKET_MAX_BUCKETS;
// place_kernel's LDS: one int64 cursor per bucket and wave
static_assert(kRebucketMaxBuckets >= 1024 && kRebucketMaxBuckets * kSortWaves * 8 <= 64 * 1024,
              "the cursors of a workgroup's waves must fit 64 KiB of LDS");
static_assert(kSortMaxWaves % kSortWaves == 0, "whole workgroups");
constexpr int kScanThreads = 256;
constexpr int kGatherThreads = 256;                  // 4 waves
constexpr int kGatherWaveRows = 8;                   // destination rows a wave writes per pass
constexpr int kGatherTileRows = kGatherWaveRows * (kGatherThreads / 64);
constexpr int kGatherMaxGrid = LMI_GATHER_MAX_GRID;  // grid cap: the rest is grid-strided
static_assert(kGatherTileRows == LMI_GATHER_TILE_ROWS, "lmi_hip.h names the tile");

// The waves of a sort over n labels (a multiple of kSortWaves; 0 for n = 0)
// and the groups of 64 labels in every wave's interval.
struct SortPlan {
    int64_t groups;        // ceil(n / 64)
    int32_t waves;         // counts' row length
    int64_t wave_groups;   // wave w owns groups [w * wave_groups, (w+1) * wave_groups)
};

inline SortPlan sort_plan(int64_t n) {
    SortPlan p{};
    p.groups = (n + 63) / 64;
    const int64_t w = std::min<int64_t>(p.groups, kSortMaxWaves);
    p.waves = (int32_t)((w + kSortWaves - 1) / kSortWaves * kSortWaves);
    p.wave_groups = p.waves ? (p.groups + p.waves - 1) / p.waves : 0;
    return p;
}

// label of sequence row i as int64 (-1: no row); T = int32_t or int64_t
template <typename T>
__device__ inline int64_t label_at(const T* __restrict__ labels, int64_t i, int64_t n) {
    return i < n ? (int64_t)labels[i] : -1;
}

// hist: counts[c * waves + w] = #{rows of wave w's interval with label c}
template <typename T>
__global__ __launch_bounds__(kSortThreads) void hist_kernel(
    const T* __restrict__ labels, int64_t n, int32_t n_buckets, int32_t waves, int64_t wave_groups,
    int64_t groups, int64_t* __restrict__ counts, int32_t* __restrict__ status) {
    extern __shared__ uint32_t hist_lds[];               // [kSortWaves][n_buckets]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t* __restrict__ h = hist_lds + (size_t)wave * n_buckets;
    for (int32_t c = lane; c < n_buckets; c += 64) h[c] = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kSortWaves + wave;
    const int64_t g0 = w * wave_groups;
    const int64_t g1 = std::min<int64_t>(g0 + wave_groups, groups);
    bool bad = false;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t i = g * 64 + lane;
        const int64_t l = label_at(labels, i, n);
        if (i < n) {
            if (l >= 0 && l < n_buckets) atomicAdd(&h[l], 1u);   // (a count: any order)
            else bad = true;
        }
    }
    if (bad) atomicOr(status, LMI_STATUS_BAD_LABEL);
    __syncthreads();
    if (w < waves)
        for (int32_t c = lane; c < n_buckets; c += 64) counts[(int64_t)c * waves + w] = (int64_t)h[c];
}

// scan, rows: one workgroup per bucket c turns counts[c][0..waves) into its
// exclusive prefix sums, in place, and writes the row's sum to total[c].
__global__ __launch_bounds__(kScanThreads) void scan_rows_kernel(int64_t* __restrict__ counts,
                                                                 int32_t waves,
                                                                 int64_t* __restrict__ total) {
    __shared__ int64_t part[kScanThreads];
    int64_t* __restrict__ row = counts + (int64_t)blockIdx.x * waves;
    const int32_t per = (waves + kScanThreads - 1) / kScanThreads;
    const int32_t a = std::min<int32_t>(threadIdx.x * per, waves);
    const int32_t b = std::min<int32_t>(a + per, waves);
    int64_t sum = 0;
    for (int32_t i = a; i < b; ++i) sum += row[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    int64_t before = 0;
    for (int32_t t = 0; t < (int32_t)threadIdx.x; ++t) before += part[t];
    for (int32_t i = a; i < b; ++i) {
        const int64_t v = row[i];
        row[i] = before;
        before += v;
    }
    if (threadIdx.x == kScanThreads - 1) total[blockIdx.x] = before;
}

// scan, buckets: bucket_off[0..n_buckets] = exclusive prefix sums of total
// (one workgroup; n_buckets <= kRebucketMaxBuckets)
__global__ __launch_bounds__(1024) void scan_off_kernel(const int64_t* __restrict__ total,
                                                        int32_t n_buckets,
                                                        int64_t* __restrict__ bucket_off) {
    __shared__ int64_t t[kRebucketMaxBuckets];
    for (int32_t c = threadIdx.x; c < n_buckets; c += blockDim.x) t[c] = total[c];
    __syncthreads();
    for (int32_t c = threadIdx.x; c <= n_buckets; c += blockDim.x) {
        int64_t s = 0;
        for (int32_t j = 0; j < c; ++j) s += t[j];
        bucket_off[c] = s;
    }
}

// place: order[bucket_off[c] + start[c][w] + rank] = row, rank counted in
// sequence order inside wave w's interval.
template <typename T>
__global__ __launch_bounds__(kSortThreads) void place_kernel(
    const T* __restrict__ labels, int64_t n, int32_t n_buckets, int32_t waves, int64_t wave_groups,
    int64_t groups, const int64_t* __restrict__ start, const int64_t* __restrict__ bucket_off,
    int64_t* __restrict__ order, int32_t* __restrict__ status) {
    extern __shared__ int64_t cursor_lds[];              // [kSortWaves][n_buckets]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // (volatile: the lanes of a wave hand the cursors to each other through
    // LDS from one group to the next; the accesses stay in program order)
    volatile int64_t* cur = cursor_lds + (size_t)wave * n_buckets;
    const int64_t w = (int64_t)blockIdx.x * kSortWaves + wave;
    if (w >= waves) return;                              // (no workgroup barrier below)
    for (int32_t c = lane; c < n_buckets; c += 64) cur[c] = bucket_off[c] + start[(int64_t)c * waves + w];
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int64_t g0 = w * wave_groups;
    const int64_t g1 = std::min<int64_t>(g0 + wave_groups, groups);
    bool lost = false;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t i = g * 64 + lane;
        const int64_t l = label_at(labels, i, n);
        const bool valid = i < n && l >= 0 && l < n_buckets;
        const int32_t c = valid ? (int32_t)l : -1;
        const int64_t first = valid ? cur[c] : 0;        // the bucket's next free position
        int32_t rank = 0, same = 0;
        uint64_t todo = __ballot(valid);
        while (todo) {                                   // one turn per distinct label (wave-uniform)
            const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
            const int32_t cl = __builtin_amdgcn_readlane(c, leader);
            const uint64_t m = __ballot(c == cl);        // (c == -1 never matches a leader's label)
            if (c == cl) {
                rank = __builtin_popcountll(m & below);
                same = __builtin_popcountll(m);
            }
            todo &= ~m;
        }
        if (valid) {
            const int64_t p = first + rank;
            if (p >= 0 && p < n) order[p] = i;
            else lost = true;                            // (never, for counts of these labels)
            if (rank == same - 1) cur[c] = first + same; // the last of the equals moves the cursor
        }
    }
    if (lost) atomicOr(status, LMI_STATUS_INTERNAL);
}

// One wave writes kGatherWaveRows consecutive destination rows per pass: lane
// l < 8 reads and checks src_pos[base + l], then the wave's lanes stride over
// the rows' 16-byte pieces -- the destination is one contiguous stream, the
// source 8 whole rows.  `pieces` = d_pad * 2 / 16 per row.
__global__ __launch_bounds__(kGatherThreads) void gather_rows_kernel(
    const uint4* __restrict__ src, const float* __restrict__ src_inv, int64_t n_src, int32_t pieces,
    const int64_t* __restrict__ src_pos, uint4* __restrict__ dst, float* __restrict__ dst_inv,
    int64_t n_dst, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_tiles = (n_dst + kGatherTileRows - 1) / kGatherTileRows;
    const int32_t total = kGatherWaveRows * pieces;  // 16-byte pieces of the wave's rows
    // piece q = lane + 64 j of a pass lies in row r_j at piece c_j of it: (r, c)
    // advance by (64 / pieces, 64 % pieces) with one carry, no division per piece
    const int32_t step_r = 64 / pieces, step_c = 64 % pieces;
    const int32_t r0 = lane / pieces, c0 = lane - r0 * pieces;
    // src_pos of the pass after this one is read before this pass's rows (-1: no row)
    auto pos_of = [&](int64_t tile) -> int64_t {
        const int64_t p = tile * kGatherTileRows + (int64_t)wave * kGatherWaveRows + lane;
        return (tile < n_tiles && lane < kGatherWaveRows && p < n_dst) ? src_pos[p] : -1;
    };
    int64_t ahead = pos_of(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kGatherTileRows + (int64_t)wave * kGatherWaveRows;
        int64_t from = ahead;
        ahead = pos_of(tile + gridDim.x);
        if (lane < kGatherWaveRows && base + lane < n_dst) {
            if (from < 0 || from >= n_src) {
                atomicOr(status, LMI_STATUS_INTERNAL);
                from = -1;
            }
            if (from >= 0) dst_inv[base + lane] = src_inv[from];
        }
        uint4* __restrict__ o = dst + base * pieces;
        int32_t r = r0, c = c0;
        // four 16-byte loads in flight per lane before the first store
        for (int32_t q0 = lane; q0 < total + lane; q0 += 4 * 64) {
            // (named registers, not arrays: no staging through LDS or scratch)
            auto at = [&](int32_t q) -> int64_t {  // piece q's place in src, -1: none
                const int64_t f = __shfl(from, q < total ? r : 0);   // (every lane takes part)
                const int64_t a = (q < total && f >= 0) ? f * pieces + c : -1;
                r += step_r;
                c += step_c;
                if (c >= pieces) {
                    c -= pieces;
                    ++r;
                }
                return a;
            };
            const int64_t a0 = at(q0);
            const int64_t a1 = at(q0 + 64);
            const int64_t a2 = at(q0 + 128);
            const int64_t a3 = at(q0 + 192);
            uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
            if (a0 >= 0) v0 = src[a0];
            if (a1 >= 0) v1 = src[a1];
            if (a2 >= 0) v2 = src[a2];
            if (a3 >= 0) v3 = src[a3];
            if (a0 >= 0) o[q0] = v0;
            if (a1 >= 0) o[q0 + 64] = v1;
            if (a2 >= 0) o[q0 + 128] = v2;
            if (a3 >= 0) o[q0 + 192] = v3;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int sort_launch(const T* labels, int64_t n, int32_t C, const SortPlan& p, int64_t* counts, int64_t* total,
                int64_t* bucket_off, int64_t* order, int32_t* status, hipStream_t s) {
    const unsigned grid = (unsigned)(p.waves / kSortWaves);
    hipLaunchKernelGGL(hist_kernel<T>, dim3(grid), dim3(kSortThreads), (size_t)kSortWaves * C * 4, s, labels,
                       n, C, p.waves, p.wave_groups, p.groups, counts, status);
    LMI_LAUNCH_CHECK("hist_kernel");
    hipLaunchKernelGGL(scan_rows_kernel, dim3((unsigned)C), dim3(kScanThreads), 0, s, counts, p.waves, total);
    LMI_LAUNCH_CHECK("scan_rows_kernel");
    hipLaunchKernelGGL(scan_off_kernel, dim3(1), dim3(1024), 0, s, total, C, bucket_off);
    LMI_LAUNCH_CHECK("scan_off_kernel");
    hipLaunchKernelGGL(place_kernel<T>, dim3(grid), dim3(kSortThreads), (size_t)kSortWaves * C * 8, s, labels,
                       n, C, p.waves, p.wave_groups, p.groups, counts, bucket_off, order, status);
    LMI_LAUNCH_CHECK("place_kernel");
    return LMI_OK;
}

}  // namespace
}  // namespace lmi

extern "C" size_t lmi_bucket_sort_labels_ws_bytes(int64_t n, int32_t n_buckets) {
    using namespace lmi;
    if (n <= 0 || n_buckets < 1 || n_buckets > kRebucketMaxBuckets) return 0;
    const SortPlan p = sort_plan(n);
    return ((size_t)n_buckets * (size_t)p.waves + (size_t)n_buckets) * sizeof(int64_t);
}

extern "C" int lmi_bucket_sort_labels(const void* labels, int32_t label_bytes, int64_t n, int32_t n_buckets,
                                      int64_t* bucket_off, int64_t* order, int32_t* status,
                                      void* workspace, size_t ws_bytes, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(label_bytes == 4 || label_bytes == 8, "bucket sort: label_bytes=%d (4 or 8)", label_bytes);
    LMI_CHECK_ARG(n >= 0, "bucket sort: n=%lld", (long long)n);
    LMI_CHECK_ARG(n_buckets >= 1, "bucket sort: n_buckets=%d", n_buckets);
    if (n_buckets > kRebucketMaxBuckets) {
        set_error("bucket sort: n_buckets=%d is above LMI_REBUCKET_MAX_BUCKETS=%d", n_buckets,
                  kRebucketMaxBuckets);
        return LMI_E_UNSUPPORTED;
    }
    LMI_CHECK_ARG(bucket_off && status, "bucket sort: null pointer");
    LMI_CHECK_ARG(n == 0 || (labels && order), "bucket sort: null labels / order");
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0)  // no row: every bucket starts and ends at 0
        return fill_u32(bucket_off, 0u, 2 * ((size_t)n_buckets + 1), s);
    const size_t need = lmi_bucket_sort_labels_ws_bytes(n, n_buckets);
    if (!workspace || ws_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
        set_error("bucket sort: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
        return LMI_E_WORKSPACE;
    }
    const SortPlan p = sort_plan(n);
    int64_t* counts = static_cast<int64_t*>(workspace);
    int64_t* total = counts + (size_t)n_buckets * p.waves;
    if (label_bytes == 4)
        return sort_launch(static_cast<const int32_t*>(labels), n, n_buckets, p, counts, total, bucket_off,
                           order, status, s);
    return sort_launch(static_cast<const int64_t*>(labels), n, n_buckets, p, counts, total, bucket_off, order,
                       status, s);
}

extern "C" int lmi_index_gather_rows(const void* src_corpus, const float* src_inv_norm, int64_t n_src,
                                     int32_t d_pad, const int64_t* src_pos, void* dst_corpus,
                                     float* dst_inv_norm, int64_t n_dst, int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(n_src >= 0 && n_dst >= 0, "gather rows: n_src=%lld n_dst=%lld", (long long)n_src,
                  (long long)n_dst);
    LMI_CHECK_ARG(d_pad > 0 && d_pad % 32 == 0, "gather rows: d_pad=%d (a positive multiple of 32)", d_pad);
    if (n_dst == 0) return LMI_OK;
    LMI_CHECK_ARG(src_corpus && src_inv_norm && src_pos && dst_corpus && dst_inv_norm && status,
                  "gather rows: null pointer");
    LMI_CHECK_ARG(src_corpus != dst_corpus && src_inv_norm != dst_inv_norm,
                  "gather rows: source and destination must be different buffers");
    LMI_CHECK_ARG(aligned16(src_corpus) && aligned16(dst_corpus), "gather rows: corpus not 16-byte aligned");
    const int64_t tiles = (n_dst + kGatherTileRows - 1) / kGatherTileRows;
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, kGatherMaxGrid);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(kGatherThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint4*>(src_corpus),
                       src_inv_norm, n_src, d_pad / 8, src_pos, static_cast<uint4*>(dst_corpus),
                       dst_inv_norm, n_dst, status);
    LMI_LAUNCH_CHECK("gather_rows_kernel");
    return LMI_OK;
}
