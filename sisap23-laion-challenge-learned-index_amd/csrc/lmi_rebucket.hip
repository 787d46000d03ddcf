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

// ---- K10 -- re-bucket inside the index's own store (DESIGN.md §3 "K10") -----
// (lmi_perm_involutions, lmi_index_swap_rows: DeviceIndex.relabel(inplace=True))
//
// The gather new[p] = old[sigma[p]] as two passes of disjoint row swaps: every
// permutation is the product of two involutions.  On a cycle of sigma with the
// ranks e_0 = L (the smallest position), e_(t+1) = sigma(e_t) and length m the
// content of rank t + 1 has to reach rank t; pass 1 swaps rank t with rank -t,
// pass 2 swaps rank u with rank m - 1 - u, and t + 1 -> -(t + 1) -> t.
//
//   plan    pointer doubling over sigma in ceil(log2 n) rounds a stage, on
//           ping-pong buffers of (value, next) pairs (one 16-byte read per hop):
//             stage 1  leader: v = min(v, v[next]); next = next[next]
//             stage 2  distance to the leader on the lists cut at the leaders
//                      (next[L] = L, v[L] = 0): v += v[next]; next = next[next]
//                      -> m = v[sigma(L)] + 1, t = (m - v) mod m
//             stage 3  exclusive prefix sums of m over the leaders in position
//                      order: every cycle gets a range of the table E,
//                      E[base + t] = e_t; the partners are read from E
//           sigma is validated first (in range; inv[sigma[p]] = p written by
//           all, read back by all: two equal entries lose one write).  Every
//           hop goes through in_range(), so a sigma that is no permutation
//           costs a status bit and never an access outside the buffers.
//   swap    row j and row partner[j] for every j with partner[j] > j, mapped as
//           the gather is: a wave owns 8 consecutive rows j, 16 bytes per lane,
//           both pieces of four pairs in registers before the first store.
namespace lmi {
namespace {

constexpr int kPermThreads = 256;
constexpr int kPermMaxGrid = 2048;                   // elementwise kernels: grid-strided beyond
constexpr int kPermScanItems = 8;                    // values a thread sums in the prefix scan
constexpr int kPermScanTile = kPermThreads * kPermScanItems;
constexpr int kPermScanThreads = 1024;               // the one workgroup over the tile sums

struct alignas(16) PermPair {
    int64_t v;    // stage 1: smallest position seen; stage 2: distance to the leader
    int64_t nx;   // the position 2^round hops on
};

// sigma[p] when it names a position, p itself otherwise (a hop that stays)
__device__ inline int64_t in_range(const int64_t* __restrict__ sigma, int64_t p, int64_t n) {
    const int64_t v = sigma[p];
    return (v >= 0 && v < n) ? v : p;
}

inline int perm_rounds(int64_t n) {
    int r = 0;
    while (((int64_t)1 << r) < n) ++r;
    return r;
}

inline int64_t perm_tiles(int64_t n) { return (n + kPermScanTile - 1) / kPermScanTile; }

inline unsigned perm_grid(int64_t n) {
    return (unsigned)std::min<int64_t>((n + kPermThreads - 1) / kPermThreads, kPermMaxGrid);
}

#define LMI_PERM_FOR(p, n)                                                        \
    for (int64_t p = (int64_t)blockIdx.x * kPermThreads + threadIdx.x; p < (n);   \
         p += (int64_t)gridDim.x * kPermThreads)

// stage 1's start and the first half of the validation
__global__ __launch_bounds__(kPermThreads) void perm_init_kernel(const int64_t* __restrict__ sigma,
                                                                 int64_t n, PermPair* __restrict__ out,
                                                                 int64_t* __restrict__ inv,
                                                                 int32_t* __restrict__ status) {
    bool bad = false;
    LMI_PERM_FOR(p, n) {
        const int64_t v = sigma[p];
        const bool ok = v >= 0 && v < n;
        if (ok) inv[v] = p;
        else bad = true;
        out[p] = PermPair{p, ok ? v : p};
    }
    if (bad) atomicOr(status, LMI_STATUS_BAD_PERM);
}

// ... the second half: a value hit twice kept one of its two writers
__global__ __launch_bounds__(kPermThreads) void perm_check_kernel(const int64_t* __restrict__ sigma,
                                                                  int64_t n,
                                                                  const int64_t* __restrict__ inv,
                                                                  int32_t* __restrict__ status) {
    bool bad = false;
    LMI_PERM_FOR(p, n) {
        const int64_t v = sigma[p];
        if (v >= 0 && v < n && inv[v] != p) bad = true;
    }
    if (bad) atomicOr(status, LMI_STATUS_BAD_PERM);
}

// one doubling round, `in` -> `out` (never in place: a racing update reads a
// neighbour of another round); two independent hops in flight per lane
template <bool kMin>
__global__ __launch_bounds__(kPermThreads) void perm_double_kernel(const PermPair* __restrict__ in,
                                                                   PermPair* __restrict__ out,
                                                                   int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kPermThreads;
    for (int64_t p = (int64_t)blockIdx.x * kPermThreads + threadIdx.x; p < n; p += 2 * stride) {
        const int64_t p1 = p + stride;
        const bool two = p1 < n;
        const PermPair a0 = in[p];
        const PermPair a1 = two ? in[p1] : a0;
        const PermPair b0 = in[a0.nx];
        const PermPair b1 = in[a1.nx];
        out[p] = PermPair{kMin ? std::min(a0.v, b0.v) : a0.v + b0.v, b0.nx};
        if (two) out[p1] = PermPair{kMin ? std::min(a1.v, b1.v) : a1.v + b1.v, b1.nx};
    }
}

// stage 2's start: the leaders are kept in `leader`, the lists are cut there
__global__ __launch_bounds__(kPermThreads) void perm_cut_kernel(const int64_t* __restrict__ sigma,
                                                                int64_t n,
                                                                const PermPair* __restrict__ found,
                                                                int64_t* __restrict__ leader,
                                                                PermPair* __restrict__ out) {
    LMI_PERM_FOR(p, n) {
        const int64_t L = found[p].v;
        leader[p] = L;
        out[p] = (L == p) ? PermPair{0, p} : PermPair{1, in_range(sigma, p, n)};
    }
}

// the cycle of p: its length m and p's rank t along sigma from the leader L
struct PermRank {
    int64_t L, m, t;
};

__device__ inline PermRank perm_rank(const int64_t* __restrict__ sigma, int64_t n,
                                     const int64_t* __restrict__ leader,
                                     const PermPair* __restrict__ dist, int64_t p) {
    PermRank r;
    r.L = leader[p];
    r.m = dist[in_range(sigma, r.L, n)].v + 1;
    const int64_t t = (r.m - dist[p].v) % r.m;
    r.t = t < 0 ? t + r.m : t;                       // (negative only when sigma is no permutation)
    return r;
}

// stage 3's input: the cycle length at every leader, 0 elsewhere
__global__ __launch_bounds__(kPermThreads) void perm_length_kernel(const int64_t* __restrict__ sigma,
                                                                   int64_t n,
                                                                   const int64_t* __restrict__ leader,
                                                                   const PermPair* __restrict__ dist,
                                                                   int64_t* __restrict__ len) {
    LMI_PERM_FOR(p, n) len[p] = (leader[p] == p) ? dist[in_range(sigma, p, n)].v + 1 : 0;
}

// exclusive prefix sums of v[0..n) in place, in three launches: the sum of
// every tile, the prefix sums of those (one workgroup), the tiles again
__device__ inline int64_t perm_thread_sum(const int64_t* __restrict__ v, int64_t a, int64_t n) {
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < kPermScanItems; ++i)
        if (a + i < n) s += v[a + i];
    return s;
}

__global__ __launch_bounds__(kPermThreads) void perm_tile_sum_kernel(const int64_t* __restrict__ v,
                                                                     int64_t n,
                                                                     int64_t* __restrict__ tile_sum) {
    __shared__ int64_t part[kPermThreads];
    const int64_t a = (int64_t)blockIdx.x * kPermScanTile + (int64_t)threadIdx.x * kPermScanItems;
    part[threadIdx.x] = perm_thread_sum(v, a, n);
    __syncthreads();
    for (int w = kPermThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kPermScanThreads) void perm_tile_scan_kernel(int64_t* __restrict__ tile_sum,
                                                                          int64_t tiles) {
    __shared__ int64_t part[kPermScanThreads];
    const int64_t per = (tiles + kPermScanThreads - 1) / kPermScanThreads;
    const int64_t a = std::min<int64_t>((int64_t)threadIdx.x * per, tiles);
    const int64_t b = std::min<int64_t>(a + per, tiles);
    int64_t sum = 0;
    for (int64_t i = a; i < b; ++i) sum += tile_sum[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    int64_t before = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
    for (int64_t i = a; i < b; ++i) {
        const int64_t x = tile_sum[i];
        tile_sum[i] = before;
        before += x;
    }
}

__global__ __launch_bounds__(kPermThreads) void perm_tile_apply_kernel(int64_t* __restrict__ v, int64_t n,
                                                                       const int64_t* __restrict__ tile_sum) {
    __shared__ int64_t part[kPermThreads];
    const int64_t a = (int64_t)blockIdx.x * kPermScanTile + (int64_t)threadIdx.x * kPermScanItems;
    part[threadIdx.x] = perm_thread_sum(v, a, n);
    __syncthreads();
    int64_t before = tile_sum[blockIdx.x];
    for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
#pragma unroll
    for (int i = 0; i < kPermScanItems; ++i)
        if (a + i < n) {
            const int64_t x = v[a + i];
            v[a + i] = before;
            before += x;
        }
}

// E[base[L] + t] = e_t
__global__ __launch_bounds__(kPermThreads) void perm_place_kernel(const int64_t* __restrict__ sigma,
                                                                  int64_t n,
                                                                  const int64_t* __restrict__ leader,
                                                                  const PermPair* __restrict__ dist,
                                                                  const int64_t* __restrict__ base,
                                                                  int64_t* __restrict__ E) {
    LMI_PERM_FOR(p, n) {
        const PermRank r = perm_rank(sigma, n, leader, dist, p);
        const int64_t at = base[r.L] + r.t;
        if (at >= 0 && at < n) E[at] = p;            // (outside only when sigma is no permutation)
    }
}

__global__ __launch_bounds__(kPermThreads) void perm_partner_kernel(const int64_t* __restrict__ sigma,
                                                                    int64_t n,
                                                                    const int64_t* __restrict__ leader,
                                                                    const PermPair* __restrict__ dist,
                                                                    const int64_t* __restrict__ base,
                                                                    const int64_t* __restrict__ E,
                                                                    int64_t* __restrict__ partner1,
                                                                    int64_t* __restrict__ partner2) {
    LMI_PERM_FOR(p, n) {
        const PermRank r = perm_rank(sigma, n, leader, dist, p);
        const int64_t b = base[r.L];
        const int64_t i1 = b + (r.t ? r.m - r.t : 0);
        const int64_t i2 = b + r.m - 1 - r.t;
        partner1[p] = (i1 >= 0 && i1 < n) ? E[i1] : p;
        partner2[p] = (i2 >= 0 && i2 < n) ? E[i2] : p;
    }
}

// One wave owns kGatherWaveRows consecutive rows j per pass: lane l < 8 reads
// partner[base + l] and checks the pair, then the wave's lanes stride over the
// 16-byte pieces of the rows that swap (partner > j).  `corpus` and `inv_norm`
// are read and written through the same pointers (no __restrict__); a lane
// holds both pieces of a pair before it stores either.
__global__ __launch_bounds__(kGatherThreads) void swap_rows_kernel(uint4* corpus, float* inv_norm,
                                                                   int64_t n, int32_t pieces,
                                                                   const int64_t* __restrict__ partner,
                                                                   int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t n_tiles = (n + kGatherTileRows - 1) / kGatherTileRows;
    const int32_t total = kGatherWaveRows * pieces;
    const int32_t step_r = 64 / pieces, step_c = 64 % pieces;
    const int32_t r0 = lane / pieces, c0 = lane - r0 * pieces;
    // partner[j] of the pass after this one is read before this pass's rows (-1: no row)
    auto partner_of = [&](int64_t tile) -> int64_t {
        const int64_t j = tile * kGatherTileRows + (int64_t)wave * kGatherWaveRows + lane;
        return (tile < n_tiles && lane < kGatherWaveRows && j < n) ? partner[j] : -1;
    };
    int64_t ahead = partner_of(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kGatherTileRows + (int64_t)wave * kGatherWaveRows;
        const int64_t q = ahead;
        ahead = partner_of(tile + gridDim.x);
        int64_t to = -1;                             // the row that row base + lane swaps with
        if (lane < kGatherWaveRows && base + lane < n) {
            const int64_t j = base + lane;
            // the whole pair is checked before its first write: q in range
            // and partner[q] == j, so no row belongs to two pairs of a launch
            if (q < 0 || q >= n || partner[q] != j) atomicOr(status, LMI_STATUS_INTERNAL);
            else if (q > j) to = q;
            if (to >= 0) {
                const float a = inv_norm[j], b = inv_norm[to];
                inv_norm[j] = b;
                inv_norm[to] = a;
            }
        }
        if (!__ballot(to >= 0)) continue;            // (wave-uniform: none of the 8 rows moves)
        int32_t r = r0, c = c0;
        for (int32_t q0 = lane; q0 < total + lane; q0 += 4 * 64) {
            // (named registers, not arrays: no staging through LDS or scratch)
            int64_t x0, x1, x2, x3;                  // piece of row j, -1: none
            int64_t y0, y1, y2, y3;                  // the same piece of its partner
            auto at = [&](int32_t p, int64_t& x, int64_t& y) {
                const int64_t f = __shfl(to, p < total ? r : 0);    // (every lane takes part)
                const bool on = p < total && f >= 0;
                x = on ? (base + r) * pieces + c : -1;
                y = on ? f * pieces + c : -1;
                r += step_r;
                c += step_c;
                if (c >= pieces) {
                    c -= pieces;
                    ++r;
                }
            };
            at(q0, x0, y0);
            at(q0 + 64, x1, y1);
            at(q0 + 128, x2, y2);
            at(q0 + 192, x3, y3);
            uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {}, w0 = {}, w1 = {}, w2 = {}, w3 = {};
            if (x0 >= 0) { v0 = corpus[x0]; w0 = corpus[y0]; }
            if (x1 >= 0) { v1 = corpus[x1]; w1 = corpus[y1]; }
            if (x2 >= 0) { v2 = corpus[x2]; w2 = corpus[y2]; }
            if (x3 >= 0) { v3 = corpus[x3]; w3 = corpus[y3]; }
            if (x0 >= 0) { corpus[x0] = w0; corpus[y0] = v0; }
            if (x1 >= 0) { corpus[x1] = w1; corpus[y1] = v1; }
            if (x2 >= 0) { corpus[x2] = w2; corpus[y2] = v2; }
            if (x3 >= 0) { corpus[x3] = w3; corpus[y3] = v3; }
        }
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace
}  // namespace lmi

extern "C" size_t lmi_perm_involutions_ws_bytes(int64_t n) {
    using namespace lmi;
    if (n <= 0) return 0;
    // two ping-pong arrays of n pairs, the leaders, the tile sums of the scan
    return align_up((5 * (size_t)n + (size_t)perm_tiles(n)) * sizeof(int64_t), 16);
}

extern "C" int lmi_perm_involutions(const int64_t* src_pos, int64_t n, int64_t* partner1, int64_t* partner2,
                                    int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(n >= 0, "perm involutions: n=%lld", (long long)n);
    LMI_CHECK_ARG(status, "perm involutions: null status");
    if (n == 0) return LMI_OK;
    LMI_CHECK_ARG(src_pos && partner1 && partner2, "perm involutions: null pointer");
    LMI_CHECK_ARG(aligned8(src_pos) && aligned8(partner1) && aligned8(partner2) &&
                      (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                  "perm involutions: misaligned pointer");
    LMI_CHECK_ARG(partner1 != partner2 && src_pos != partner1 && src_pos != partner2,
                  "perm involutions: src_pos, partner1 and partner2 must be different buffers");
    const size_t need = lmi_perm_involutions_ws_bytes(n);
    if (!workspace || ws_bytes < need || !aligned16(workspace)) {
        set_error("perm involutions: workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes, need);
        return LMI_E_WORKSPACE;
    }
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int64_t* w = static_cast<int64_t*>(workspace);
    PermPair* P[2] = {reinterpret_cast<PermPair*>(w), reinterpret_cast<PermPair*>(w + 2 * n)};
    int64_t* leader = w + 4 * n;
    int64_t* tile_sum = w + 5 * n;
    const int rounds = perm_rounds(n);
    const unsigned grid = perm_grid(n);
    const unsigned tiles = (unsigned)perm_tiles(n);
    const dim3 blk(kPermThreads);
    // validation (inv lives in P[1] until the first round writes there) and stage 1
    int64_t* inv = w + 2 * n;
    hipLaunchKernelGGL(perm_init_kernel, dim3(grid), blk, 0, s, src_pos, n, P[0], inv, status);
    LMI_LAUNCH_CHECK("perm_init_kernel");
    hipLaunchKernelGGL(perm_check_kernel, dim3(grid), blk, 0, s, src_pos, n, inv, status);
    LMI_LAUNCH_CHECK("perm_check_kernel");
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(perm_double_kernel<true>, dim3(grid), blk, 0, s, P[r & 1], P[(r + 1) & 1], n);
        LMI_LAUNCH_CHECK("perm_double_kernel<min>");
    }
    // stage 2: from the array stage 1 ended in to the other one, then ping-pong
    PermPair* G[2] = {P[(rounds + 1) & 1], P[rounds & 1]};
    hipLaunchKernelGGL(perm_cut_kernel, dim3(grid), blk, 0, s, src_pos, n, G[1], leader, G[0]);
    LMI_LAUNCH_CHECK("perm_cut_kernel");
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(perm_double_kernel<false>, dim3(grid), blk, 0, s, G[r & 1], G[(r + 1) & 1], n);
        LMI_LAUNCH_CHECK("perm_double_kernel<add>");
    }
    const PermPair* dist = G[rounds & 1];
    // stage 3 in the array stage 2 did not end in: cycle lengths -> bases, and E
    int64_t* base = reinterpret_cast<int64_t*>(G[(rounds + 1) & 1]);
    int64_t* E = base + n;
    hipLaunchKernelGGL(perm_length_kernel, dim3(grid), blk, 0, s, src_pos, n, leader, dist, base);
    LMI_LAUNCH_CHECK("perm_length_kernel");
    hipLaunchKernelGGL(perm_tile_sum_kernel, dim3(tiles), blk, 0, s, base, n, tile_sum);
    LMI_LAUNCH_CHECK("perm_tile_sum_kernel");
    hipLaunchKernelGGL(perm_tile_scan_kernel, dim3(1), dim3(kPermScanThreads), 0, s, tile_sum, (int64_t)tiles);
    LMI_LAUNCH_CHECK("perm_tile_scan_kernel");
    hipLaunchKernelGGL(perm_tile_apply_kernel, dim3(tiles), blk, 0, s, base, n, tile_sum);
    LMI_LAUNCH_CHECK("perm_tile_apply_kernel");
    hipLaunchKernelGGL(perm_place_kernel, dim3(grid), blk, 0, s, src_pos, n, leader, dist, base, E);
    LMI_LAUNCH_CHECK("perm_place_kernel");
    hipLaunchKernelGGL(perm_partner_kernel, dim3(grid), blk, 0, s, src_pos, n, leader, dist, base, E, partner1,
                       partner2);
    LMI_LAUNCH_CHECK("perm_partner_kernel");
    return LMI_OK;
}

extern "C" int lmi_index_swap_rows(void* corpus, float* inv_norm, int64_t n, int32_t d_pad,
                                   const int64_t* partner, int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(n >= 0, "swap rows: n=%lld", (long long)n);
    LMI_CHECK_ARG(d_pad > 0 && d_pad % 8 == 0, "swap rows: d_pad=%d (a positive multiple of 8)", d_pad);
    if (n == 0) return LMI_OK;
    LMI_CHECK_ARG(corpus && inv_norm && partner && status, "swap rows: null pointer");
    LMI_CHECK_ARG(aligned16(corpus), "swap rows: corpus not 16-byte aligned");
    LMI_CHECK_ARG(aligned8(partner) && (reinterpret_cast<uintptr_t>(inv_norm) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                  "swap rows: misaligned pointer");
    const int64_t tiles = (n + kGatherTileRows - 1) / kGatherTileRows;
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, kGatherMaxGrid);
    hipLaunchKernelGGL(swap_rows_kernel, dim3(grid), dim3(kGatherThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<uint4*>(corpus), inv_norm, n,
                       d_pad / 8, partner, status);
    LMI_LAUNCH_CHECK("swap_rows_kernel");
    return LMI_OK;
}
