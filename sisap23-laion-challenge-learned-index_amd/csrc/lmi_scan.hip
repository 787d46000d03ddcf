// K2 — per-(query, probe) exact top-k inside the probed bucket (gfx950).
//
// Replaces, for every probe r < R of every query, the reference's
//   utils.py:10-11   pairwise_cosine = 1 - sklearn cosine_similarity
//                    (normalize both sides, BLAS GEMM),
//   LearnedIndex.py:170-172  full-row argsort, first k,
//   LearnedIndex.py:152-153, :168  pandas .loc gathers of the bucket rows,
// with one bucket-major pass over the corpus.
//
// Pipeline (all on one stream, no host synchronisation, no allocation):
//   prep_kernel        queries -> fp16 (or fp32) padded rows + 1/||q||;
//                      output lists pre-filled with (+inf, -1)
//   plan_count_kernel  (query, probe) pairs per bucket
//   plan_fill_kernel   pairs grouped by bucket (ascending q), and the tile
//                      list: tile = (bucket, chunk of <= chunk_rows rows,
//                      block of <= QB pairs), chunk-major so the query blocks
//                      that re-read one chunk run back to back (L2 / MALL)
//                      (with chunk centroids: nearest chunk first, pref_kernel
//                      .. tile3_fill_kernel; else tail_split_kernel cuts each
//                      queue's last tiles into row parts)
//   scan3_kernel       (lmi_scan3.hpp) persistent, 8 waves; each workgroup
//                      dequeues tiles.  The tile's queries live in registers
//                      as MFMA B fragments, the chunk's rows are staged once
//                      per workgroup through an LDS ring by DMA and shared by
//                      the waves (v_mfma_f32_32x32x16_f16: exact fp16
//                      products, fp32 accumulation).  The top-k epilogue runs
//                      on the accumulators: d = 1 - dot/(|q||y|), a filter
//                      against the pair's bound (thr_g, shared by the pair's
//                      tiles), survivors inserted into per-lane register
//                      lists; the tile's list is written as its chunk list.
//                      It takes an fp16 corpus, fp16-exact queries and
//                      d_pad == 768 with 10- or 15-entry lists; every other
//                      shape runs scan2_kernel (the 4-wave ring) or
//                      scan_kernel (general) of lmi_scan_v12.hip.
//   chunk_merge_kernel per pair: merge its bucket's chunk lists -> top-k,
//                      positions -> global positions.
// scan_plan() makes every choice of one scan (kernel family, list length, tile
// width, split parts, workspace offsets) and bucket_topk_impl runs it; k > 16
// is lmi_scan_wide.hip, the split mode lmi_scan_split.hip.
#include "lmi_scan_internal.hpp"
#include "lmi_quant.hpp"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <type_traits>
#include <vector>

// diagnostic hook: defined by lmi_scan_abl.hip in the `make ablation` library
// (the ABL != 0 instantiations of scan3_kernel), absent from the product
extern "C" __attribute__((weak)) int lmi_abl_launch_scan3(int kl, int abl, const void* args,
                                                          void* stream);

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// prep
// ---------------------------------------------------------------------------
// One wave per query (4 per workgroup: a latency-bound pass over 30 MB at
// 10k queries; round 1's 256-thread workgroup per query took 19 us, most of
// it workgroup launch and block reductions): each lane takes runs of 4
// consecutive elements, float4 loads when the rows allow (VEC).
// Word fills of the plan's per-pair arrays, folded into prep (one kernel
// launch instead of one per array): array f gets value v[f] in words
// [row * per_q[f], (row + 1) * per_q[f]) from the wave of query `row`.
struct PrepFills {
    uint32_t* p[5];
    uint32_t v[5];
    int32_t per_q[5];
    int32_t n;
};

template <bool F16, bool VEC>
__global__ __launch_bounds__(kThreads) void prep_kernel(const float* __restrict__ q, int32_t nq,
                                                        int32_t ldq, int32_t d, int32_t d_pad,
                                                        void* __restrict__ qbuf,
                                                        float* __restrict__ invq,
                                                        int32_t* __restrict__ status,
                                                        float* __restrict__ out_d,
                                                        int32_t* __restrict__ out_pos,
                                                        int32_t* __restrict__ out_row,
                                                        int32_t out_per_q, PrepFills fills) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;  // (wave-uniform; no block-wide barrier below)
    const float* src = q + (size_t)row * ldq;
    float ss = 0.0f;
    bool inexact = false;
    for (int c0 = 4 * lane; c0 < d_pad; c0 += 256) {  // d_pad is a multiple of 32
        float v[4];
        if (VEC && c0 + 3 < d) {
            const float4 f = *reinterpret_cast<const float4*>(src + c0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (c0 + e < d) ? src[c0 + e] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(v[e], v[e], ss);
        if constexpr (F16) {
            _Float16 h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = (_Float16)v[e];
                inexact |= ((float)h[e] != v[e]);
            }
            uint2 pk;
            pk.x = (uint32_t)__builtin_bit_cast(uint16_t, h[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, h[1]) << 16);
            pk.y = (uint32_t)__builtin_bit_cast(uint16_t, h[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, h[3]) << 16);
            *reinterpret_cast<uint2*>(reinterpret_cast<_Float16*>(qbuf) + (size_t)row * d_pad + c0) = pk;
        } else {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(qbuf) + (size_t)row * d_pad + c0) =
                make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if constexpr (F16) {
        if (__any(inexact) && lane == 0) atomicOr(status, LMI_STATUS_QUERY_NOT_F16);
    }
    if (lane == 0) {
        const float n = sqrtf(ss);
        // sklearn _handle_zeros_in_scale: norms < 10*eps are replaced by 1
        invq[row] = (n < 10.0f * 1.1920929e-07f) ? 1.0f : 1.0f / n;
    }
    for (int e = lane; e < out_per_q; e += 64) {
        out_d[(size_t)row * out_per_q + e] = __builtin_inff();
        out_pos[(size_t)row * out_per_q + e] = -1;
        if (out_row) out_row[(size_t)row * out_per_q + e] = -1;
    }
    for (int f = 0; f < fills.n; ++f)
        for (int e = lane; e < fills.per_q[f]; e += 64)
            fills.p[f][(size_t)row * fills.per_q[f] + e] = fills.v[f];
}

// prep_kernel for an LMI_I8 scan: qbuf = the int8 codes [nq][d_pad] of every
// query and invq = the codes' 1/||c||, by the rows' own device function
// (quantize_row_i8); the output prefill and the PrepFills as above.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void prep_i8_kernel(const float* __restrict__ q, int32_t nq,
                                                           int32_t ldq, int32_t d, int32_t d_pad,
                                                           int8_t* __restrict__ qbuf,
                                                           float* __restrict__ invq,
                                                           float* __restrict__ out_d,
                                                           int32_t* __restrict__ out_pos,
                                                           int32_t* __restrict__ out_row,
                                                           int32_t out_per_q, PrepFills fills) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;  // (wave-uniform; no block-wide barrier below)
    const float inv = quantize_row_i8<float, VEC>(q + (size_t)row * ldq, d, d_pad, lane,
                                                  qbuf + (size_t)row * d_pad);
    if (lane == 0) invq[row] = inv;
    for (int e = lane; e < out_per_q; e += 64) {
        out_d[(size_t)row * out_per_q + e] = __builtin_inff();
        out_pos[(size_t)row * out_per_q + e] = -1;
        if (out_row) out_row[(size_t)row * out_per_q + e] = -1;
    }
    for (int f = 0; f < fills.n; ++f)
        for (int e = lane; e < fills.per_q[f]; e += 64)
            fills.p[f][(size_t)row * fills.per_q[f] + e] = fills.v[f];
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
template <int NT = kThreads>
__device__ inline int block_sum(int v, int* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < NT / 64; ++w) t += sh[w];
    return t;
}

// The two plan kernels: one workgroup per bucket reads all P classes, a
// latency-bound pass, so they run 16 waves wide (4x fewer dependent rounds)
constexpr int kPlanThreads = 1024;

__global__ __launch_bounds__(kPlanThreads) void plan_count_kernel(const int32_t* __restrict__ classes,
                                                              int32_t P, int32_t* __restrict__ counts) {
    __shared__ int sh[kPlanThreads / 64];
    const int c = blockIdx.x;
    int n = 0;
    for (int e0 = threadIdx.x; e0 < P; e0 += 8 * kPlanThreads) {  // eight loads in flight
        int v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (e0 + u * kPlanThreads < P) ? classes[e0 + u * kPlanThreads] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) n += (v[u] == c) ? 1 : 0;
    }
    n = block_sum<kPlanThreads>(n, sh);
    if (threadIdx.x == 0) counts[c] = n;
}

// Tile list layout (a permutation of all tiles):
//   8 groups, group x = tiles whose global chunk index (chunk_first[c] + j)
//   is = x mod 8; inside a group, every bucket's chunk-0 tiles first, then
//   the other chunks, bucket-major, chunk-major, query-block-minor.
// The persistent scan dequeues from group (blockIdx.x mod 8) — the blocks that
// share an XCD under the observed round-robin placement — and steals from the
// other groups when its own is empty; the query blocks of one chunk therefore
// run back to back on one XCD and re-read the chunk from its L2.  Placement
// only affects speed.  Chunk-0 tiles first: they publish each pair's k-th key
// early, so later chunks start with a tight bound.
//   meta[0..7] group offsets, meta[8..15] group sizes, meta[16] total
//   work[0..7] group dequeue counters, work[8] the single counter of v1
__device__ inline int count_mod(int a, int n, int x, int ng) {
    // #{t in [0, n) : (a + t) mod ng == x}, ng a power of two
    if (n <= 0) return 0;
    const int first = (x - a) & (ng - 1);
    return n / ng + ((first < (n & (ng - 1))) ? 1 : 0);
}

__global__ __launch_bounds__(kPlanThreads) void plan_fill_kernel(
    const int32_t* __restrict__ classes, int32_t P, int32_t C, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ chunk_first, int32_t QB, int32_t* __restrict__ pair_q,
    int32_t* __restrict__ pair_bucket, Tile* __restrict__ tiles, int32_t* __restrict__ meta,
    int32_t* __restrict__ work, int32_t ng, int32_t* __restrict__ pair_pos, int32_t qpad) {
    __shared__ int sh[kPlanThreads / 64];
    __shared__ int wcnt[kPlanThreads / 64];
    __shared__ int g0_all[kGroups], gr_all[kGroups], g0_lt[kGroups], gr_lt[kGroups];
    const int c = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < kGroups) g0_all[tid] = gr_all[tid] = g0_lt[tid] = gr_lt[tid] = 0;
    __syncthreads();
    int off = 0;
    for (int b = tid; b < C; b += kPlanThreads) {
        const int nch = chunk_first[b + 1] - chunk_first[b];
        const int nqb = nch > 0 ? (counts[b] + QB - 1) / QB : 0;
        if (b < c) off += counts[b];
        if (nqb == 0) continue;
        const int cf = chunk_first[b];
        atomicAdd(&g0_all[cf & (ng - 1)], nqb);
        if (b < c) atomicAdd(&g0_lt[cf & (ng - 1)], nqb);
        for (int x = 0; x < ng; ++x) {
            const int r = nqb * count_mod(cf + 1, nch - 1, x, ng);
            if (r) {
                atomicAdd(&gr_all[x], r);
                if (b < c) atomicAdd(&gr_lt[x], r);
            }
        }
    }
    off = block_sum<kPlanThreads>(off, sh);  // (contains the __syncthreads the atomics need)
    int goff[kGroups];
    {
        int acc = 0;
        for (int x = 0; x < kGroups; ++x) {
            goff[x] = acc + x * qpad;  // (each queue region followed by qpad free slots)
            acc += g0_all[x] + gr_all[x];
        }
        if (c == C - 1 && tid == 0) {
            for (int x = 0; x < kGroups; ++x) {
                meta[x] = goff[x];
                meta[kGroups + x] = g0_all[x] + gr_all[x];
                meta[2 * kGroups + 1 + x] = g0_all[x];  // the group's chunk-0 (seed) tiles
                work[x] = 0;
            }
            meta[2 * kGroups] = acc;
            work[kGroups] = 0;
        }
    }
    const int cnt = counts[c];
    const int nch = chunk_first[c + 1] - chunk_first[c];
    const int nqb = (cnt + QB - 1) / QB;
    if (cnt == 0) return;
    // ordered fill of this bucket's pairs (ascending pair id = ascending q):
    // every wave takes a contiguous segment, reads it coalesced (64 pairs per
    // instruction) and ranks its matches by ballot; a wave's base is the
    // count of the segments before it
    {
        const int lane = tid & 63, w = tid >> 6;
        const int seg = ((P + kPlanThreads / 64 - 1) / (kPlanThreads / 64) + 63) & ~63;
        const int sa = min(P, w * seg), sb = min(P, sa + seg);
        constexpr int kU = 8;  // loads in flight per lane (each pass is latency-bound)
        int n = 0;
        for (int e0 = sa; e0 < sb; e0 += kU * 64) {
            int v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int e = e0 + 64 * u + lane;
                v[u] = e < sb ? classes[e] : -1;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) n += __popcll(__ballot(v[u] == c));
        }
        if (lane == 0) wcnt[w] = n;
        __syncthreads();
        int o = off;
        for (int i = 0; i < w; ++i) o += wcnt[i];
        const uint64_t lt = (1ull << lane) - 1ull;
        for (int e0 = sa; e0 < sb; e0 += kU * 64) {
            int v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int e = e0 + 64 * u + lane;
                v[u] = e < sb ? classes[e] : -1;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const uint64_t m = __ballot(v[u] == c);
                if (v[u] == c) {
                    pair_q[o + __popcll(m & lt)] = e0 + 64 * u + lane;
                    pair_bucket[o + __popcll(m & lt)] = c;
                    if (pair_pos) pair_pos[e0 + 64 * u + lane] = o + __popcll(m & lt);
                }
                o += __popcll(m);
            }
        }
    }
    const int cf = chunk_first[c];
    for (int i = tid; i < nch * nqb; i += kPlanThreads) {
        const int j = i / nqb, b = i - j * nqb;
        const int x = (cf + j) & (ng - 1);
        Tile t;
        t.c = c;
        t.pp0 = off + b * QB;
        t.np = min(QB, cnt - b * QB);
        t.chunk = j;
        int pos;
        if (j == 0) {
            pos = goff[x] + g0_lt[x] + b;
        } else {
            // chunks 1 .. j-1 of this bucket that fall in group x, before this one
            pos = goff[x] + g0_all[x] + gr_lt[x] + nqb * count_mod(cf + 1, j - 1, x, ng) + b;
        }
        tiles[pos] = t;
    }
}

// Tail split (scan v3; LMI_SCAN_SPLIT): the last K tiles of every group queue
// are replaced by S row parts each (LMI_SCAN_SPLIT_PARTS, default 2), so the
// launch ends on small tiles.  The scan kernel is unchanged: a part is an
// ordinary tile whose bucket is a virtual entry of an extended bucket table,
// chosen so that the scan's own
//     row0 = off[c] + chunk * chunk_rows,  rows = min(chunk_rows, off[c + 1] - row0)
// give the part's rows, and whose chunk is its partial-list slot: part s of
// chunk j writes slot s*X + j (X = max_chunks, the stride is S*X; part 0 keeps
// chunk j's slot); bit j of mask[pp] tells the chunk merge to read slots
// X + j .. (S-1)*X + j too (chunks j < 32 only).  Every part but the last has
// a whole number of 32-row blocks, and at least two.  In place: plan_fill left
// K (S - 1) free slots after every queue, so only the last K tiles move.
__global__ __launch_bounds__(256) void tail_split_kernel(Tile* __restrict__ tiles,
                                                         int32_t* __restrict__ meta,
                                                         const int64_t* __restrict__ bucket_off,
                                                         int64_t* __restrict__ ext_off, int32_t C,
                                                         int32_t chunk_rows, int32_t X, int32_t K,
                                                         int32_t S, uint32_t* __restrict__ mask) {
    __shared__ int wsp[4];
    __shared__ int s_pp0[256], s_np[256], s_bit[256];  // the split tiles' pair blocks
    const int x = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (x == 0)
        for (int i = tid; i <= C; i += 256) ext_off[i] = bucket_off[i];
    const int o = meta[x], n = meta[kGroups + x];
    const int seeds = meta[2 * kGroups + 1 + x];
    const int k2 = max(0, min(K, n - seeds));  // the candidates: the queue's last k2 tiles
    Tile t{};
    int64_t rs = 0, re = 0;
    bool sp = false;
    if (tid < k2) {
        t = tiles[o + n - k2 + tid];
        rs = bucket_off[t.c] + (int64_t)t.chunk * chunk_rows;
        re = min(rs + (int64_t)chunk_rows, bucket_off[t.c + 1]);
        sp = re - rs >= 2 * 32 * S && t.chunk < 32;
        s_pp0[tid] = t.pp0;
        s_np[tid] = sp ? t.np : 0;
        s_bit[tid] = 1 << (t.chunk & 31);
    }
    const uint64_t m = __ballot(sp);
    if (lane == 0) wsp[w] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
    for (int v = 0; v < 4; ++v) {
        before += (v < w) ? wsp[v] : 0;
        total += wsp[v];
    }
    if (tid < k2) {
        const int at = o + (n - k2) + tid + before * (S - 1);
        if (!sp) {
            tiles[at] = t;
        } else {
            const int pr = (int)((re - rs) / (32 * S)) * 32;  // rows of every part but the last
            const int v = C + 1 + 2 * S * (x * K + tid);
            for (int p = 0; p < S; ++p) {
                const int64_t a0 = rs + (int64_t)p * pr;
                const int slot = p * X + t.chunk;
                ext_off[v + 2 * p] = a0 - (int64_t)slot * chunk_rows;
                ext_off[v + 2 * p + 1] = (p == S - 1) ? re : a0 + pr;
                tiles[at + p] = Tile{v + 2 * p, t.pp0, t.np, slot};
            }
        }
    }
    // the pairs of every split tile: bit chunk of their mask (the whole
    // workgroup per tile, fire-and-forget atomics)
    for (int i = 0; i < k2; ++i)
        for (int e = tid; e < s_np[i]; e += 256) atomicOr(&mask[s_pp0[i] + e], (uint32_t)s_bit[i]);
    __syncthreads();  // (every thread read meta[x] above)
    if (tid == 0) {
        meta[kGroups + x] = n + total * (S - 1);
        atomicAdd(&meta[2 * kGroups], total * (S - 1));
    }
}

// ---------------------------------------------------------------------------
// nearest-chunk-first plan (scan v3, index with chunk centroids)
//
// Each (query, probe) pair scans every chunk of its bucket; the order only
// decides how early its pruning bound gets tight.  With the bucket's rows
// laid out by sub-cluster (one sub-cluster per chunk), a pair's nearest
// neighbours sit mostly in the chunk whose centroid is nearest, so:
//   pref_kernel       pair -> its nearest chunk (max cosine to the centroid)
//   pref_sort_kernel  the bucket's pairs re-ordered by (nearest chunk, pair),
//                     so a 256-pair tile group shares few nearest chunks
//   tile3_fill_kernel the tile list: one "seed" tile per group first (the
//                     nearest chunk of the group's median pair; they publish
//                     each pair's bound through thr_g), then the rest
//                     chunk-major
// ---------------------------------------------------------------------------
__device__ inline int bucket_pair_off(const int32_t* counts, int c, int* sh) {
    int off = 0;
    for (int b = threadIdx.x; b < c; b += kThreads) off += counts[b];
    return block_sum(off, sh);
}

__global__ __launch_bounds__(kThreads) void pref_kernel(
    const int32_t* __restrict__ pair_bucket, const int32_t* __restrict__ chunk_first,
    const float* __restrict__ centroid, int32_t d_pad, const _Float16* __restrict__ qbuf,
    const int32_t* __restrict__ pair_q, int32_t R, int32_t P, int32_t* __restrict__ pref) {
    // one wave per pair (thousands of waves hide the L2 latency of the loads)
    const int lane = threadIdx.x & 63;
    const int pp = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (pp >= P) return;
    const int c = pair_bucket[pp];
    if (c < 0) return;
    const int c0 = chunk_first[c], nch = chunk_first[c + 1] - c0;
    if (nch <= 1) {
        if (lane == 0) pref[pp] = 0;
        return;
    }
    const _Float16* qr = qbuf + (size_t)(pair_q[pp] / R) * d_pad;
    float best = -3.0f;
    int bj = 0;
    for (int j = 0; j < nch; ++j) {
        const float* cr = centroid + (size_t)(c0 + j) * d_pad;
        float s = 0.0f;
        for (int e = lane; e < d_pad; e += 64) s = fmaf((float)qr[e], cr[e], s);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (s > best) {  // wave-uniform after the butterfly; ties -> lower chunk
            best = s;
            bj = j;
        }
    }
    if (lane == 0) pref[pp] = bj;
}

__global__ __launch_bounds__(kThreads) void pref_sort_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ chunk_first,
    int32_t* __restrict__ pair_q, int32_t* __restrict__ pref, int32_t* __restrict__ tmp,
    int32_t* __restrict__ tmp_pref, int32_t QB, int32_t* __restrict__ n_seed) {
    __shared__ int sh[kThreads / 64];
    __shared__ int wcnt[kThreads / 64];
    const int c = blockIdx.x;
    const int off = bucket_pair_off(counts, c, sh);
    const int cnt = counts[c];
    const int nch = chunk_first[c + 1] - chunk_first[c];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (nch <= 1) {  // nothing to order (an empty bucket has no tiles at all)
        if (tid == 0) n_seed[c] = (nch == 1) ? (cnt + QB - 1) / QB : 0;
        return;
    }
    // stable counting sort by pref: one ordered compaction pass per chunk
    int run = 0;
    for (int j = 0; j < nch; ++j) {
        for (int base = 0; base < cnt; base += kThreads) {
            const int e = base + tid;
            const bool pred = (e < cnt) && (pref[off + e] == j);
            const uint64_t m = __ballot(pred);
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) wcnt[w] = __popcll(m);
            __syncthreads();
            int wpre = 0, tot = 0;
            for (int i = 0; i < kThreads / 64; ++i) {
                wpre += (i < w) ? wcnt[i] : 0;
                tot += wcnt[i];
            }
            if (pred) {
                tmp[off + run + wpre + rank] = pair_q[off + e];
                tmp_pref[off + run + wpre + rank] = j;
            }
            run += tot;
        }
    }
    __syncthreads();
    for (int e = tid; e < cnt; e += kThreads) {
        pair_q[off + e] = tmp[off + e];
        pref[off + e] = tmp_pref[off + e];
    }
    // one seed tile per group of QB pairs (see tile3_fill_kernel)
    if (tid == 0) n_seed[c] = (cnt + QB - 1) / QB;
}

__global__ __launch_bounds__(kThreads) void tile3_fill_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ chunk_first,
    const int32_t* __restrict__ pref, const int32_t* __restrict__ n_seed, int32_t C, int32_t QB,
    Tile* __restrict__ tiles, int32_t* __restrict__ meta, int32_t* __restrict__ work) {
    __shared__ int sh[kThreads / 64];
    const int c = blockIdx.x;
    const int tid = threadIdx.x;
    int s_lt = 0, r_lt = 0, s_all = 0, r_all = 0, off = 0;
    for (int b = tid; b < C; b += kThreads) {
        const int nch = chunk_first[b + 1] - chunk_first[b];
        const int ng = nch > 0 ? (counts[b] + QB - 1) / QB : 0;
        const int rest = ng * nch - n_seed[b];
        s_all += n_seed[b];
        r_all += rest;
        if (b < c) {
            s_lt += n_seed[b];
            r_lt += rest;
            off += counts[b];
        }
    }
    s_lt = block_sum(s_lt, sh);
    r_lt = block_sum(r_lt, sh);
    s_all = block_sum(s_all, sh);
    r_all = block_sum(r_all, sh);
    off = block_sum(off, sh);
    if (c == 0 && tid == 0) {
        for (int x = 0; x < kGroups; ++x) {
            meta[x] = 0;
            meta[kGroups + x] = (x == 0) ? s_all + r_all : 0;
            work[x] = 0;
        }
        meta[2 * kGroups] = s_all + r_all;
        work[kGroups] = 0;
    }
    if (tid != 0) return;  // per-bucket tile lists are short: one thread writes them
    const int cnt = counts[c];
    const int nch = chunk_first[c + 1] - chunk_first[c];
    if (cnt == 0 || nch == 0) return;
    // the seed chunk of group g: the nearest chunk of its median pair (the
    // group's pairs are sorted by nearest chunk, so it is the most common one)
    const int ngr = (cnt + QB - 1) / QB;
    int ps = s_lt, pr = s_all + r_lt;
    for (int g = 0; g < ngr; ++g) {
        const int n = min(QB, cnt - g * QB);
        tiles[ps++] = Tile{c, off + g * QB, n, pref[off + g * QB + n / 2]};
    }
    for (int j = 0; j < nch; ++j)
        for (int g = 0; g < ngr; ++g) {
            const int n = min(QB, cnt - g * QB);
            if (j != pref[off + g * QB + n / 2]) tiles[pr++] = Tile{c, off + g * QB, n, j};
        }
}


// LMI_Q_SEED_ROUND0: per grouped pair position pp, the grouped position of
// its round-0 pair (q, 0), or -1 for r = 0 pairs (pair_pos: grouped position
// of every pair id, plan_fill_kernel; pairs of out-of-range classes keep -1)
__global__ __launch_bounds__(256) void seed_pos_kernel(const int32_t* __restrict__ pair_q,
                                                       const int32_t* __restrict__ pair_pos,
                                                       int32_t P, int32_t R,
                                                       int32_t* __restrict__ seed_pos) {
    const int pp = blockIdx.x * 256 + threadIdx.x;
    if (pp >= P) return;
    // (positions past the grouped pairs -- classes out of range -- hold stale
    // pair ids that no tile reads; any id outside [0, P) maps to -1)
    const int p = pair_q[pp];
    seed_pos[pp] = (p < 0 || p >= P || p % R == 0) ? -1 : pair_pos[p - p % R];
}

}  // namespace
}  // namespace lmi

#include "lmi_scan3.hpp"  // scan3_kernel (scan v3) and its helpers

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// chunk merge
// ---------------------------------------------------------------------------
// kMergeLanes lanes per pair (round 6; was one thread per pair): lane s of a
// pair merges the pair's chunk lists j = s, s + kMergeLanes, ... into a
// register list (each list read with all its loads in flight, then its global
// positions gathered the same way; the next list's keys load while this
// one's positions are gathered), then the lanes' lists are merged by a
// butterfly of shuffles (log2 kMergeLanes rounds: insert the partner lane's
// entries).  Every lane ends with the same list: the KL smallest keys of the
// union, exactly the one-thread merge's.  At 40,000 pairs one thread per pair
// was 625 waves for 1,024 SIMDs -- latency-bound, ~41 us at W = 8 (58 at
// W = 1) on the finish chain's critical path.
constexpr int kMergeLanes = 8;
constexpr int kMergeBlock = 256;

// slot of the pair's j-th list: chunks 0 .. nch_c - 1, then the other parts
// (1 .. S-1) of the tail-split chunks in ascending chunk order (bit b of the
// pair's mask: chunk b was split; part p lives at slot p * X + b)
__device__ inline int chunk_slot(int j, int nch_c, uint32_t sm, int S, int X) {
    if (j < nch_c) return j;
    const int idx = j - nch_c;
    int n = idx / (S - 1);
    const int part = 1 + idx % (S - 1);
    while (n-- > 0) sm &= sm - 1u;
    return part * X + __builtin_ctz(sm);
}

// (the pair's list keys are (distance, local row) in the partial lists and
// (distance, global position) in M; rows inside a chunk ascend in global
// position, so mapping keeps each list ordered and the merge is by the
// reference's (distance, g.index) order)
//
// The merges are bitonic over kMergeN = 16 register slots: two ascending
// lists A, B -> A[i] = min(A[i], B[15 - i]) is bitonic and holds the union's
// 16 smallest; four half-cleaner stages sort it.  48 compare-exchanges a merge
// where inserting a list entry by entry cost up to 16 shifting inserts of 16
// (the band lists' merge, 16 slots, took 2.4x the plain 10-slot merge's time
// at W = 8: ~126 against 53 us after the scan, profiles/r06aj_w8_*_trace.txt).
constexpr int kMergeN = 16;
__device__ inline void bitonic_top(uint64_t (&A)[kMergeN], int32_t (&AW)[kMergeN], const uint64_t (&B)[kMergeN],
                                   const int32_t (&BW)[kMergeN]) {
#pragma unroll
    for (int i = 0; i < kMergeN; ++i) {
        const bool t = B[kMergeN - 1 - i] < A[i];
        A[i] = t ? B[kMergeN - 1 - i] : A[i];
        AW[i] = t ? BW[kMergeN - 1 - i] : AW[i];
    }
#pragma unroll
    for (int d = kMergeN / 2; d > 0; d >>= 1) {
#pragma unroll
        for (int i = 0; i < kMergeN; ++i) {
            if ((i & d) == 0) {
                const uint64_t x = A[i], y = A[i + d];
                const int32_t xw = AW[i], yw = AW[i + d];
                const bool sw = y < x;
                A[i] = sw ? y : x;
                A[i + d] = sw ? x : y;
                AW[i] = sw ? yw : xw;
                AW[i + d] = sw ? xw : yw;
            }
        }
    }
}

// one ascending list K of NE (distance, local row) entries into M (its first
// KL exact): entries past M's KL-th distance are dropped before the gather
template <int KL, int NE>
__device__ inline void merge_chunk_list(const uint64_t (&K)[NE], uint64_t (&M)[kMergeN], int32_t (&W)[kMergeN],
                                        const int32_t* __restrict__ gpos, int64_t n_rows,
                                        int32_t* __restrict__ status) {
    static_assert(NE <= kMergeN && KL <= kMergeN, "merge slots");
    const uint32_t thr = (uint32_t)(M[KL - 1] >> 32);
    uint64_t B[kMergeN];
    int32_t BW[kMergeN];
#pragma unroll
    for (int i = 0; i < kMergeN; ++i) {
        B[i] = kEmptyKey;
        BW[i] = -1;
    }
    int32_t g[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const uint32_t lp = (uint32_t)K[i];
        const bool live = K[i] != kEmptyKey && (uint32_t)(K[i] >> 32) <= thr;
        const bool ok = lp < (uint32_t)n_rows;
        if (live && !ok) atomicOr(status, LMI_STATUS_INTERNAL);  // never for a sound scan
        g[i] = (live && ok) ? gpos[lp] : -1;
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        if (g[i] >= 0) {
            B[i] = (K[i] & 0xffffffff00000000ull) | (uint32_t)g[i];
            BW[i] = (int32_t)(uint32_t)K[i];
        }
    }
    bitonic_top(M, W, B, BW);
}

// The lanes of a pair merge their lists (xor butterfly inside the pair's
// kMergeLanes-lane group): after the rounds every lane holds the union's
// kMergeN smallest keys
__device__ inline void merge_lanes(uint64_t (&M)[kMergeN], int32_t (&W)[kMergeN]) {
#pragma unroll
    for (int off = 1; off < kMergeLanes; off <<= 1) {
        uint64_t o[kMergeN];
        int32_t ow[kMergeN];
#pragma unroll
        for (int i = 0; i < kMergeN; ++i) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)M[i], off);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(M[i] >> 32), off);
            o[i] = ((uint64_t)hi << 32) | lo;
            ow[i] = __shfl_xor(W[i], off);
        }
        bitonic_top(M, W, o, ow);
    }
}

// one pair's lists -> the merged list in M/W (every lane of the pair's group);
// NE entries read per list (KL, or the band lists' kBandSlot - 1), the
// list's slot stride LS; BAND: *ub = the smallest of the lists' bound slots
template <int KL, int NE, int LS, bool BAND>
__device__ inline void merge_pair(const uint64_t* __restrict__ partial, int32_t max_chunks, int pp, int nch_c,
                                  uint32_t sm, int S, const int32_t* __restrict__ gpos, int64_t n_rows,
                                  int32_t* __restrict__ status, int sub, uint64_t (&M)[KL], int32_t (&W)[KL],
                                  uint32_t* ub) {
    const int nch = nch_c + (S - 1) * __popc(sm);
    const int X = max_chunks / S;
    uint64_t MM[kMergeN];
    int32_t WW[kMergeN];
#pragma unroll
    for (int i = 0; i < kMergeN; ++i) {
        MM[i] = kEmptyKey;
        WW[i] = -1;
    }
    uint64_t Kn[NE];
    uint32_t ubn = 0xffffffffu;
    auto load = [&](int j) {
        const uint64_t* src = partial + ((size_t)pp * max_chunks + chunk_slot(j, nch_c, sm, S, X)) * LS;
#pragma unroll
        for (int i = 0; i < NE; ++i) Kn[i] = src[i];
        if constexpr (BAND) ubn = (uint32_t)(src[LS - 1] >> 32);
    };
    if (sub < nch) load(sub);
    for (int j = sub; j < nch; j += kMergeLanes) {
        uint64_t K[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) K[i] = Kn[i];
        if constexpr (BAND) *ub = std::min(*ub, ubn);
        if (j + kMergeLanes < nch) load(j + kMergeLanes);
        merge_chunk_list<KL, NE>(K, MM, WW, gpos, n_rows, status);
    }
    merge_lanes(MM, WW);
#pragma unroll
    for (int i = 0; i < KL; ++i) {
        M[i] = MM[i];
        W[i] = WW[i];
    }
}

template <int KL, bool ROWS>
__global__ __launch_bounds__(kMergeBlock) void chunk_merge_kernel(
    const uint64_t* __restrict__ partial, int32_t max_chunks, const int32_t* __restrict__ pair_q,
    const int32_t* __restrict__ pair_bucket, const int32_t* __restrict__ chunk_first,
    const int32_t* __restrict__ gpos, int32_t P, int32_t k, int32_t ldo, float* __restrict__ out_d,
    int32_t* __restrict__ out_pos, int32_t* __restrict__ out_row, int64_t n_rows,
    int32_t* __restrict__ status, const uint32_t* __restrict__ split_mask, int32_t S) {
    const int gt = blockIdx.x * kMergeBlock + threadIdx.x;
    const int pp = gt / kMergeLanes, sub = gt % kMergeLanes;
    // (a pair's lanes are one aligned group of a wave: they return together)
    if (pp >= P) return;
    const int c = pair_bucket[pp];
    if (c < 0) return;
    const int nch_c = chunk_first[c + 1] - chunk_first[c];
    const uint32_t sm = split_mask != nullptr ? split_mask[pp] : 0u;
    uint64_t M[KL];
    int32_t W[KL];
    merge_pair<KL, KL, KL, false>(partial, max_chunks, pp, nch_c, sm, S, gpos, n_rows, status, sub, M, W,
                                  nullptr);
    const size_t o = (size_t)pair_q[pp] * ldo;
#pragma unroll
    for (int i = 0; i < KL; ++i) {
        if (i < k && i % kMergeLanes == sub) {
            const uint64_t key = M[i];
            const bool empty = key == kEmptyKey;
            out_d[o + i] = empty ? __builtin_inff() : ord2f((uint32_t)(key >> 32));
            out_pos[o + i] = empty ? -1 : (int32_t)(uint32_t)key;
            if constexpr (ROWS) out_row[o + i] = empty ? -1 : W[i];
        }
    }
}

// The float64 mode's band lists (scan3_kernel MODE 3): per pair, its parts'
// 15-entry lists merged to the first 15 by (distance, global position), and
// out_bound[pair id] = the smallest of the parts' bounds and of the merge's
// 16th distance: every row of the pair's shard not in its list either failed
// the scan's widened filter or has d32 >= out_bound (refine_kernel falls back
// to the whole shard when that bound enters the float64 band).
__global__ __launch_bounds__(kMergeBlock) void chunk_merge_band_kernel(
    const uint64_t* __restrict__ partial, int32_t max_chunks, const int32_t* __restrict__ pair_q,
    const int32_t* __restrict__ pair_bucket, const int32_t* __restrict__ chunk_first,
    const int32_t* __restrict__ gpos, int32_t P, int32_t k, int32_t ldo, float* __restrict__ out_d,
    int32_t* __restrict__ out_pos, int32_t* __restrict__ out_row, float* __restrict__ out_bound,
    int64_t n_rows, int32_t* __restrict__ status, const uint32_t* __restrict__ split_mask, int32_t S,
    float* __restrict__ kth_out, int32_t kth_k, const int32_t* __restrict__ classes, int32_t C) {
    constexpr int NB = kBandSlot, KB = kBandSlot - 1;
    const int gt = blockIdx.x * kMergeBlock + threadIdx.x;
    const int pp = gt / kMergeLanes, sub = gt % kMergeLanes;
    if (pp >= P) return;
    // (kth_out of a pair whose class is out of range -- it has no grouped
    // position -- is +inf: lane 1 of grouped position pp takes pair id pp)
    if (kth_out != nullptr && sub == 1) {
        const int cl = classes[pp];
        if (cl < 0 || cl >= C)
            for (int i = 0; i < kth_k; ++i) kth_out[(size_t)pp * kth_k + i] = __builtin_inff();
    }
    const int c = pair_bucket[pp];
    if (c < 0) return;
    const int nch_c = chunk_first[c + 1] - chunk_first[c];
    const uint32_t sm = split_mask != nullptr ? split_mask[pp] : 0u;
    uint64_t M[NB];
    int32_t W[NB];
    uint32_t ub = 0xffffffffu;
    merge_pair<NB, KB, NB, true>(partial, max_chunks, pp, nch_c, sm, S, gpos, n_rows, status, sub, M, W, &ub);
#pragma unroll
    for (int off = 1; off < kMergeLanes; off <<= 1) ub = std::min(ub, (uint32_t)__shfl_xor((int)ub, off));
    ub = std::min(ub, (uint32_t)(M[NB - 1] >> 32));
    const int pid = pair_q[pp];
    const size_t o = (size_t)pid * ldo;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (i < k && i % kMergeLanes == sub) {
            const uint64_t key = M[i];
            const bool empty = key == kEmptyKey;
            const float dv = empty ? __builtin_inff() : ord2f((uint32_t)(key >> 32));
            out_d[o + i] = dv;
            out_pos[o + i] = empty ? -1 : (int32_t)(uint32_t)key;
            out_row[o + i] = empty ? -1 : W[i];
            if (kth_out != nullptr && i < kth_k) kth_out[(size_t)pid * kth_k + i] = dv;
        }
    }
    if (sub == 0) out_bound[pid] = ub == 0xffffffffu ? __builtin_inff() : ord2f(ub);
}

// the collect scan's per-grouped-pair bound (thr_g: the distance ordinal in
// the high word) and candidate count; a pair whose bucket has skipped rows in
// front of it (WideScan::app_d) starts with the skipped rows' own list
__global__ __launch_bounds__(256) void set_bound_kernel(const int32_t* __restrict__ pair_q, int32_t P,
                                                        const uint32_t* __restrict__ bound_ord,
                                                        unsigned long long* __restrict__ thr_g,
                                                        uint32_t* __restrict__ ccount,
                                                        const int32_t* __restrict__ pair_bucket,
                                                        const int64_t* __restrict__ bucket_off,
                                                        const float* __restrict__ app_d,
                                                        const int32_t* __restrict__ app_row, int32_t app_k,
                                                        uint64_t* __restrict__ cand, int32_t cap) {
    const int pp = blockIdx.x * 256 + threadIdx.x;
    if (pp >= P) return;
    const int p = pair_q[pp];
    const uint32_t b = (p < 0 || p >= P) ? 0u : bound_ord[p];
    thr_g[pp] = ((unsigned long long)b << 32) | 0xffffffffull;
    uint32_t n = 0u;
    const int c = pair_bucket[pp];
    if (app_d && b != 0u && c > 0 && (c & 1) && bucket_off[c - 1] < bucket_off[c]) {
        for (int i = 0; i < app_k && (int)n < cap; ++i) {
            const float dv = app_d[(size_t)p * app_k + i];
            const int32_t r = app_row[(size_t)p * app_k + i];
            if (r < 0 || !(dv < __builtin_inff())) continue;
            cand[(size_t)pp * cap + n++] = ((uint64_t)f2ord(dv) << 32) | (uint32_t)r;
        }
    }
    ccount[pp] = n;
}

// the tagged scan on the 8-wave ring (scan3_kernel MODE 4): every query's
// (1/|q|, value, mask) as one triple
__global__ __launch_bounds__(256) void want_pack_kernel(const float* __restrict__ invq,
                                                        const uint32_t* __restrict__ value,
                                                        const uint32_t* __restrict__ mask, int32_t nq,
                                                        uint32_t* __restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) {
        out[3 * (size_t)q] = __float_as_uint(invq[q]);
        out[3 * (size_t)q + 1] = value[q];
        out[3 * (size_t)q + 2] = mask[q];
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
thread_local int t_i8_lists16 = 0;  // lmi_scan_set_i8_lists16 (0: k = 11..16 stay on scan_i8_kernel)
}  // namespace

int split_parts() {
    return std::max(2, std::min(kSplitMaxParts, env_config().scan_split_parts));
}

ScanPlan scan_plan(const lmi_index_desc* idx, int nq, int R, int k, int qmode, bool lo, bool tagged) {
    ScanPlan w{};
    w.f16math = (idx->dtype == LMI_F16) && (qmode == LMI_Q_F16);
    w.i8 = (idx->dtype == LMI_I8) && (qmode == LMI_Q_I8);
    // the rings take an fp16 corpus, fp16-exact queries and d_pad == 768; the
    // diagnostic switches LMI_SCAN_V1 / LMI_SCAN_V2 force the general kernel /
    // the 4-wave ring.  The 8-wave ring has 10- and 15-entry lists; the
    // lower-bound passes (k > 16) run on it or on the general kernel
    // (tagged: the 8-wave ring's 10-entry lists or the general kernel)
    const bool ring4 = w.f16math && idx->d_pad == v2::D && !env_config().scan_v1;
    const bool ring8 = ring4 && !env_config().scan_v2;
    w.kl = k <= 10 ? 10 : (k <= 15 && ring8 && !tagged) ? 15 : 16;
    // (the 8-bit storage has a ring of its own at the same width, plain and
    // tagged: 10-entry lists, and 16-entry ones for the threads that asked
    // for them -- lmi_scan_set_i8_lists16, the over-fetch of a re-rank; by
    // default k = 11..16 keep the plan they had, scan_i8_kernel's.
    // LMI_SCAN_V1 forces scan_i8_kernel, LMI_SCAN_V2 does nothing there)
    const bool ring8i8 = w.i8 && idx->d_pad == v3::D && (w.kl == 10 || (w.kl == 16 && t_i8_lists16 != 0)) &&
                         !env_config().scan_v1;
    w.family = ring8i8 ? ScanKernel::Ring8I8
               : ring8 && w.kl != 16 ? ScanKernel::Ring8
               : ring4 && !lo && !tagged ? ScanKernel::Ring4 : ScanKernel::General;
    const bool v3 = w.family == ScanKernel::Ring8;
    w.qb = v3 || ring8i8 ? v3::QB : w.family == ScanKernel::Ring4 ? v2::QB : (w.f16math || w.i8 ? 64 : 32);
    const size_t P = (size_t)nq * R;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    w.qbuf = take((size_t)nq * idx->d_pad * (w.i8 ? 1 : w.f16math ? 2 : 4));
    w.invq = take((size_t)nq * 4);
    w.counts = take((size_t)idx->n_buckets * 4);
    w.pair_q = take(P * 4);
    w.pair_bucket = take(P * 4);
    // tiles <= sum_c nch_c * ceil(cnt_c/QB) <= sum_c nch_c * (cnt_c/QB + 1)
    const size_t X = (size_t)std::max(idx->max_chunks, 1);
    const size_t mt = (P / w.qb + 1) * X + (size_t)idx->n_chunks;
    w.max_tiles = (int32_t)std::min<size_t>(mt, (size_t)INT32_MAX);
    // the tail split is off (one part) off the 8-wave ring, under the
    // nearest-chunk-first plan and with LMI_SCAN_SPLIT < 0
    w.nearest_first = v3 && idx->chunk_centroid && !env_config().scan_no_pref;
    w.split_s = v3 && !w.nearest_first && env_config().scan_split >= 0 ? split_parts() : 1;
    w.list_stride = w.split_s * (int32_t)X;
    // (the buffers are sized for split_parts() on the 8-wave ring whether the
    // split is on or not, so the total and every offset do not depend on the
    // LMI_SCAN_SPLIT / LMI_SCAN_NO_PREF knobs or on the index's centroids:
    // a workspace sized once fits every call)
    const size_t S = v3 ? (size_t)split_parts() : 1;
    // (+ K (S - 1) free slots after every queue: the tail split's parts, in place)
    w.tiles = take(((size_t)w.max_tiles + (size_t)kGroups * kSplitMaxK * (S - 1)) * sizeof(Tile));
    w.ntiles = take(4 * (3 * kGroups + 1));
    w.work = take(4 * (kGroups + 1));
    // (x S: the other parts of tail-split chunks, slot s * max_chunks + j)
    // (15-entry lists: room for the float64 mode's band slots, kBandSlot)
    w.partial = take(P * (S * X) * (w.kl == 15 ? kBandSlot : w.kl) * sizeof(uint64_t));
    w.ext_off = take(((size_t)idx->n_buckets + 1 + 2 * S * (size_t)kGroups * kSplitMaxK) * 8);
    w.split_mask = take(P * 4);
    w.thr_g = take(P * sizeof(uint64_t));
    w.pref = take(P * 4);
    w.pref_tmp = take(P * 4);
    w.pref_tmp2 = take(P * 4);
    w.n_seed = take((size_t)idx->n_buckets * 4);
    w.pair_pos = take(P * 4);
    w.seed_pos = take(P * 4);
    w.total = off;
    return w;
}

int i8_gate(const char* fn, const lmi_index_desc* idx, int32_t k, int32_t qmode) {
    const int32_t base = qmode & ~(LMI_Q_SEED_ROUND0 | (7 << 9) | LMI_Q_PHASE_SCAN_JOIN | LMI_Q_PHASE_REFINE);
    const bool i8 = idx != nullptr && idx->dtype == LMI_I8;
    if (!i8 && base != LMI_Q_I8) return LMI_OK;
    LMI_CHECK_ARG(i8 && base == LMI_Q_I8,
                  "%s: LMI_I8 (the 8-bit storage) and LMI_Q_I8 come together (dtype=%d, qmode=0x%x)", fn,
                  idx ? idx->dtype : -1, qmode);
    LMI_CHECK_ARG(k >= 1 && k <= LMI_MAX_K, "%s: LMI_I8 takes k in [1, %d], not %d", fn, LMI_MAX_K, k);
    LMI_CHECK_ARG(!(qmode & LMI_Q_SEED_ROUND0), "%s: LMI_I8 is never seeded (LMI_Q_SEED_ROUND0)", fn);
    LMI_CHECK_ARG(!(qmode & LMI_Q_PHASE_SCAN_JOIN), "%s: LMI_I8 takes no join workgroups (LMI_Q_PHASE_SCAN_JOIN)", fn);
    LMI_CHECK_ARG(!idx->corpus32 && !idx->corpus64,
                  "%s: LMI_I8 with corpus32 / corpus64 (the 8-bit storage keeps the codes alone)", fn);
    LMI_CHECK_ARG(!idx->chunk_centroid, "%s: LMI_I8 takes no sub-cluster layout (chunk_centroid)", fn);
    LMI_CHECK_ARG(idx->d_pad >= 32 && idx->d_pad % 32 == 0 && idx->d_pad <= kI8MaxDPad,
                  "%s: LMI_I8 takes d_pad a multiple of 32 up to %d, not %d", fn, kI8MaxDPad, idx->d_pad);
    return LMI_OK;
}

int i8_refuse(const char* fn, const lmi_index_desc* idx) {
    LMI_CHECK_ARG(idx == nullptr || idx->dtype != LMI_I8,
                  "%s: LMI_I8 (the 8-bit storage) is served by lmi_bucket_topk and lmi_bucket_topk_masked alone", fn);
    return LMI_OK;
}

bool band_capable(const lmi_index_desc* idx, int qmode) {
    return scan_plan(idx, 0, 1, 10, qmode).family == ScanKernel::Ring8;
}

namespace {
thread_local int t_scan_wgs = 0;  // lmi_scan_set_workgroups (0: env / every CU)
thread_local int t_join_wgs = 0;  // lmi_scan_set_join_workgroups (0: one launch)
thread_local int t_grid = 0;      // ScanGrid: the grid of the launch under way (0: num_cus())
}  // namespace

int join_wgs() { return t_join_wgs; }

int join_gate(int& phases, bool joinable, bool* done) {
    *done = false;
    if (t_join_wgs == 0) {
        phases &= ~kPhaseJoin;
        *done = phases == 0;
        return LMI_OK;
    }
    if ((phases & (kPhaseScan | kPhaseJoin)) && !joinable) {
        set_error("this scan does not take join workgroups (j = %d): the 8-wave ring's 10- and 15-entry "
                  "lists and band lists do", t_join_wgs);
        return LMI_E_INVALID;
    }
    return LMI_OK;
}

int scan_grid() { return t_grid > 0 ? t_grid : num_cus(); }
ScanGrid::ScanGrid(int wgs) { t_grid = wgs; }
ScanGrid::~ScanGrid() { t_grid = 0; }

int num_cus() {
    static int n = 0;
    static std::once_flag once;
    std::call_once(once, [] {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
    });
    const int cus = n > 0 ? n : 256;
    const int w = t_scan_wgs > 0 ? t_scan_wgs : env_config().scan_wgs;
    return w > 0 ? std::min(w, cus) : cus;
}

// ---- optional event timing of the scan kernel ------------------------------
Timing& timing() {
    static Timing t;
    return t;
}

int timing_record(hipStream_t s, bool start, std::pair<hipEvent_t, hipEvent_t>& pr) {
    if (start) {
        Timing& t = timing();
        std::lock_guard<std::mutex> g(t.mu);
        if (!t.pool.empty()) {
            pr = t.pool.back();
            t.pool.pop_back();
        } else {
            LMI_HIP_TRY(hipEventCreate(&pr.first));
            LMI_HIP_TRY(hipEventCreate(&pr.second));
        }
        LMI_HIP_TRY(hipEventRecord(pr.first, s));
    } else {
        LMI_HIP_TRY(hipEventRecord(pr.second, s));
        Timing& t = timing();
        std::lock_guard<std::mutex> g(t.mu);
        t.pending.push_back(pr);
    }
    return LMI_OK;
}

namespace {

template <int KL>
int launch_scan3(const Scan2Args& b, hipStream_t s) {
    // the diagnostic variants (LMI_SCAN_ABL) live in lmi_scan_abl.hip, linked
    // only into the `make ablation` library; the product ignores the switch
    const int abl = env_config().scan_abl;
    if (abl != 0 && lmi_abl_launch_scan3 != nullptr) return lmi_abl_launch_scan3(KL, abl, &b, s);
    return launch_scan3_v<KL, 0>(b, s);
}

// The kernel of one call: the instantiation that serves the plan's family and
// list length, the wide mode (WideScan::mode, 0: none), lower bounds (lo) and
// band lists (band); neither where none does -- a caller's mistake: the wide
// scans and the band lists take the 8-wave ring with 15 entries (10: the
// collect), the lower-bound passes its 15 or the general kernel's 16
struct ScanLaunch {
    int (*ring)(const Scan2Args&, hipStream_t);
    int (*general)(const ScanArgs&, int, hipStream_t);
};
ScanLaunch pick_launch(const ScanPlan& p, const ScanCall& c) {
    const int kl = p.kl, mode = c.wide ? c.wide->mode : 0;
    const bool lo = c.lo_g != nullptr, band = c.out_bound != nullptr, corpus_f16 = c.idx->dtype == LMI_F16;
    const bool plain = mode == 0 && !lo && !band;
    if (p.i8) {
        // the 8-bit scan: plain or tagged lists, nothing else
        if (!plain) return {nullptr, nullptr};
        if (p.family == ScanKernel::Ring8I8)
            return {c.tags != nullptr ? (kl == 10 ? launch_scan3_i8<10, true> : launch_scan3_i8<16, true>)
                                      : (kl == 10 ? launch_scan3_i8<10, false> : launch_scan3_i8<16, false>),
                    nullptr};
        if (c.tags != nullptr)
            return {nullptr, kl == 10 ? launch_scan_i8<10, true> : launch_scan_i8<16, true>};
        return {nullptr, kl == 10 ? launch_scan_i8<10, false> : launch_scan_i8<16, false>};
    }
    if (c.tags != nullptr) {
        // the tagged scan: the 8-wave ring's MODE 4 or the general kernel's TAG
        if (!plain) return {nullptr, nullptr};
        if (p.family == ScanKernel::Ring8)
            return {kl == 10 ? launch_scan3_v<10, 0, false, 4> : nullptr, nullptr};
        if (p.family != ScanKernel::General) return {nullptr, nullptr};
        if (p.f16math)
            return {nullptr, kl == 10 ? launch_scan<10, true, _Float16, false, true>
                                      : launch_scan<16, true, _Float16, false, true>};
        if (corpus_f16)
            return {nullptr, kl == 10 ? launch_scan<10, false, _Float16, false, true>
                                      : launch_scan<16, false, _Float16, false, true>};
        return {nullptr, kl == 10 ? launch_scan<10, false, float, false, true>
                                  : launch_scan<16, false, float, false, true>};
    }
    if (p.family == ScanKernel::Ring8) {
        if (mode == 1 && !lo && !band && kl == 15) return {launch_scan3_v<15, 0, false, 1>, nullptr};
        if (mode == 2 && !lo && !band && kl == 10) return {launch_scan3_v<10, 0, false, 2>, nullptr};
        if (mode == 0 && lo && !band && kl == 15) return {launch_scan3_v<15, 0, true>, nullptr};
        if (mode == 0 && !lo && band && kl == 15) return {launch_scan3_v<10, 0, false, 3>, nullptr};
        if (plain) return {kl == 10 ? launch_scan3<10> : launch_scan3<15>, nullptr};
    } else if (p.family == ScanKernel::Ring4) {
        if (plain) return {kl == 10 ? launch_scan2<10> : launch_scan2<16>, nullptr};
    } else if (mode == 0 && lo && !band && kl == 16) {
        return {nullptr, p.f16math                  ? launch_scan<16, true, _Float16, true>
                         : corpus_f16   ? launch_scan<16, false, _Float16, true>
                                        : launch_scan<16, false, float, true>};
    } else if (plain && p.f16math) {
        return {nullptr, kl == 10 ? launch_scan<10, true, _Float16> : launch_scan<16, true, _Float16>};
    } else if (plain && corpus_f16) {
        return {nullptr, kl == 10 ? launch_scan<10, false, _Float16> : launch_scan<16, false, _Float16>};
    } else if (plain) {
        return {nullptr, kl == 10 ? launch_scan<10, false, float> : launch_scan<16, false, float>};
    }
    return {nullptr, nullptr};
}

}  // namespace
}  // namespace lmi

extern "C" int32_t lmi_plan_chunks(const int64_t* bucket_off_host, int32_t n_buckets,
                                   int32_t chunk_rows, int32_t* chunk_first_out) {
    using namespace lmi;
    if (!bucket_off_host || !chunk_first_out || n_buckets < 1 || chunk_rows < 32 || chunk_rows % 32) {
        set_error("lmi_plan_chunks: bad arguments");
        return -LMI_E_INVALID;
    }
    int32_t maxc = 0;
    int64_t acc = 0;
    for (int c = 0; c < n_buckets; ++c) {
        chunk_first_out[c] = (int32_t)acc;
        const int64_t n = bucket_off_host[c + 1] - bucket_off_host[c];
        if (n < 0) {
            set_error("lmi_plan_chunks: bucket offsets not ascending at %d", c);
            return -LMI_E_INVALID;
        }
        const int64_t nch = (n + chunk_rows - 1) / chunk_rows;
        maxc = std::max<int32_t>(maxc, (int32_t)nch);
        acc += nch;
    }
    chunk_first_out[n_buckets] = (int32_t)acc;
    return maxc;
}

size_t lmi::scan_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k,
                                 int32_t qmode, bool lo) {
    if (!idx || nq < 0 || R < 1 || k < 1) return 0;
    return scan_plan(idx, nq, R, k, qmode, lo).total;
}

extern "C" size_t lmi_scan_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R,
                                           int32_t k, int32_t qmode) {
    using namespace lmi;
    if (i8_gate("lmi_scan_workspace_bytes", idx, k, qmode) != LMI_OK) return 0;
    qmode &= ~LMI_Q_SEED_ROUND0;
    take_phases(qmode);
    if (!idx || nq < 0 || R < 1 || k < 1 || k > LMI_MAX_K_PASSES) return 0;
    if (idx->corpus32) return k <= LMI_MAX_K ? x_ws_bytes(idx, nq, R, k) : 0;
    if (k <= LMI_MAX_K) return scan_workspace_bytes(idx, nq, R, k, qmode);
    int kp;
    const int ldo = passes_of(idx, qmode, k, &kp) * kp;
    return 2 * align_up((size_t)nq * R * ldo * 4, 256) + wide_ws_bytes(idx, nq, R, k, qmode, ldo);
}

namespace {
// tuning knobs (defaults are the tuned values; results do not depend on them)
int clamp_knob(int v, int dflt, int lo, int hi) { return v == 0 && dflt != 0 ? dflt : std::max(lo, std::min(hi, v)); }
}  // namespace

extern "C" int lmi_bucket_topk(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                               const int32_t* classes, int32_t R, int32_t k, int32_t qmode,
                               float* out_d, int32_t* out_pos, int32_t* status, void* workspace,
                               size_t ws_bytes, void* stream) {
    using namespace lmi;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    LMI_TRY(i8_gate("lmi_bucket_topk", idx, k, qmode));
    const bool seed = (qmode & LMI_Q_SEED_ROUND0) != 0;
    qmode &= ~LMI_Q_SEED_ROUND0;
    int phases = take_phases(qmode);
    // (the split mode and k > LMI_MAX_K refuse join workgroups before they
    // launch anything; bucket_topk_impl gates its own call)
    if (idx && (idx->corpus32 || k > LMI_MAX_K)) {
        bool done;
        LMI_TRY(join_gate(phases, false, &done));
        if (done) return LMI_OK;
    }
    if (idx && idx->corpus32)  // (phases: k <= 10, ABI 11)
        return bucket_topk_x(idx, q, nq, ldq, nullptr, 0, classes, R, k, out_d, 0, out_pos, status, workspace,
                             ws_bytes, s, phases);
    const ScanCall c{.idx = idx, .q = q, .nq = nq, .ldq = ldq, .classes = classes, .R = R, .k = k,
                     .qmode = qmode, .out_d = out_d, .out_pos = out_pos, .status = status,
                     .workspace = workspace, .ws_bytes = ws_bytes, .stream = s, .seed_r0 = seed,
                     .phases = phases};
    return k <= LMI_MAX_K ? bucket_topk_impl(c) : bucket_topk_wide_k(c);
}

extern "C" size_t lmi_scan_tagged_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R,
                                                  int32_t k, int32_t qmode) {
    using namespace lmi;
    if (!idx || nq < 0 || R < 1 || k < 1 || k > LMI_MAX_K) return 0;
    if (idx->corpus32 || idx->corpus64 || idx->chunk_centroid) return 0;
    if (i8_gate("lmi_scan_tagged_workspace_bytes", idx, k, qmode) != LMI_OK) return 0;
    if (qmode != LMI_Q_F16 && qmode != LMI_Q_F32 && qmode != LMI_Q_I8) return 0;
    return scan_plan(idx, nq, R, k, qmode, false, true).total;
}

namespace lmi {
namespace {
// lmi_bucket_topk_tagged (mask = want) and lmi_bucket_topk_masked, `fn` the
// entry's name for the messages
int topk_masked(const char* fn, const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* value,
                const uint32_t* mask, const float* q, int32_t nq, int32_t ldq, const int32_t* classes, int32_t R,
                int32_t k, int32_t qmode, float* out_d, int32_t* out_pos, int32_t* status, void* workspace,
                size_t ws_bytes, void* stream) {
    // (every refusal comes before any launch and needs no device)
    LMI_CHECK_ARG(idx != nullptr, "null index");
    LMI_CHECK_ARG(tags != nullptr && value != nullptr && mask != nullptr, "%s: null tags or want", fn);
    LMI_TRY(i8_gate(fn, idx, k, qmode));  // (the 8-bit storage's own refusals, by name)
    LMI_CHECK_ARG(k >= 1 && k <= LMI_MAX_K, "%s: k=%d outside [1, %d]", fn, k, LMI_MAX_K);
    LMI_CHECK_ARG(!idx->corpus32 && !idx->corpus64, "%s: the split mode (corpus32 / corpus64) takes no tags", fn);
    LMI_CHECK_ARG(!idx->chunk_centroid, "%s: sub-cluster layouts (chunk_centroid) take no tags", fn);
    LMI_CHECK_ARG(qmode == LMI_Q_F16 || qmode == LMI_Q_F32 || qmode == LMI_Q_I8,
                  "%s: qmode 0x%x: LMI_Q_F16, LMI_Q_F32 or LMI_Q_I8 alone (no phase, join or seed flag)", fn, qmode);
    const ScanCall c{.idx = idx, .q = q, .nq = nq, .ldq = ldq, .classes = classes, .R = R, .k = k,
                     .qmode = qmode, .out_d = out_d, .out_pos = out_pos, .status = status,
                     .workspace = workspace, .ws_bytes = ws_bytes,
                     .stream = reinterpret_cast<hipStream_t>(stream), .tags = tags, .want = value, .mask = mask};
    // (with join workgroups set on this thread bucket_topk_impl refuses the
    // call: the tagged scan runs in one launch)
    return bucket_topk_impl(c);
}
}  // namespace

int masked_words_check(const char* fn, const uint32_t* host_value, const uint32_t* host_mask, int32_t nq) {
    LMI_CHECK_ARG((host_value != nullptr) == (host_mask != nullptr), "%s: host_value and host_mask come together", fn);
    if (host_value == nullptr) return LMI_OK;
    for (int32_t i = 0; i < nq; ++i)
        LMI_CHECK_ARG((host_value[i] & ~host_mask[i]) == 0u,
                      "%s: query %d: value 0x%x has bits outside mask 0x%x (a bit both wanted and avoided)", fn, i,
                      host_value[i], host_mask[i]);
    return LMI_OK;
}
}  // namespace lmi

extern "C" int lmi_bucket_topk_tagged(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* want,
                                      const float* q, int32_t nq, int32_t ldq, const int32_t* classes,
                                      int32_t R, int32_t k, int32_t qmode, float* out_d, int32_t* out_pos,
                                      int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
    return lmi::topk_masked("lmi_bucket_topk_tagged", idx, tags, want, want, q, nq, ldq, classes, R, k, qmode, out_d,
                            out_pos, status, workspace, ws_bytes, stream);
}

extern "C" int lmi_bucket_topk_masked(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* value,
                                      const uint32_t* mask, const uint32_t* host_value,
                                      const uint32_t* host_mask, const float* q, int32_t nq, int32_t ldq,
                                      const int32_t* classes, int32_t R, int32_t k, int32_t qmode, float* out_d,
                                      int32_t* out_pos, int32_t* status, void* workspace, size_t ws_bytes,
                                      void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(idx != nullptr, "null index");
    LMI_CHECK_ARG(tags != nullptr && value != nullptr && mask != nullptr,
                  "lmi_bucket_topk_masked: null tags, value or mask");
    LMI_CHECK_ARG(nq >= 0, "lmi_bucket_topk_masked: nq < 0");
    LMI_TRY(masked_words_check("lmi_bucket_topk_masked", host_value, host_mask, nq));
    return topk_masked("lmi_bucket_topk_masked", idx, tags, value, mask, q, nq, ldq, classes, R, k, qmode, out_d,
                       out_pos, status, workspace, ws_bytes, stream);
}

int lmi::bucket_topk_impl(const ScanCall& c) {
    using namespace lmi;
    const lmi_index_desc* idx = c.idx;
    const int32_t nq = c.nq, ldq = c.ldq, R = c.R, k = c.k, qmode = c.qmode, ldo = c.ldo > 0 ? c.ldo : k;
    const int32_t* classes = c.classes;
    const unsigned long long* lo_g = c.lo_g;
    const WideScan* wide = c.wide;
    float *out_d = c.out_d, *out_bound = c.out_bound, *kth_out = c.kth_out;
    int32_t *out_pos = c.out_pos, *out_row = c.out_row, *status = c.status;
    hipStream_t s = c.stream;
    LMI_CHECK_ARG(idx != nullptr, "null index");
    LMI_CHECK_ARG(idx->dtype == LMI_F16 || idx->dtype == LMI_F32 || idx->dtype == LMI_I8, "bad corpus dtype");
    // (the 8-bit storage: the checks of the entry points again, for the
    // internal callers -- the wide path, the float64 mode, the range search --
    // none of which it takes)
    LMI_TRY(i8_gate("bucket_topk", idx, k, qmode | (c.seed_r0 ? LMI_Q_SEED_ROUND0 : 0)));
    LMI_CHECK_ARG(idx->dtype != LMI_I8 || (c.lo_g == nullptr && c.wide == nullptr && c.out_bound == nullptr &&
                                           c.range == nullptr && !(c.phases & kPhaseJoin)),
                  "LMI_I8 takes plain and tagged lists alone (no lower bounds, wide scans, band lists, range "
                  "scan or join phase)");
    LMI_CHECK_ARG(idx->d >= 1 && idx->d_pad >= idx->d && idx->d_pad % 32 == 0, "bad d/d_pad");
    LMI_CHECK_ARG(idx->n_buckets >= 1, "n_buckets < 1");
    LMI_CHECK_ARG(idx->chunk_rows >= 32 && idx->chunk_rows % 32 == 0, "chunk_rows must be a multiple of 32");
    LMI_CHECK_ARG(idx->n_rows >= 0 && idx->n_rows < (int64_t)UINT32_MAX, "n_rows out of range");
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < INT32_MAX, "bad nq/R");
    LMI_CHECK_ARG(k >= 1 && k <= LMI_MAX_K, "k=%d outside [1, %d]", k, LMI_MAX_K);
    LMI_CHECK_ARG(qmode == LMI_Q_F16 || qmode == LMI_Q_F32 || qmode == LMI_Q_I8, "bad qmode");
    LMI_CHECK_ARG(ldq >= idx->d, "ldq < d");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(c.q && classes && out_d && out_pos && status && c.workspace, "null pointer");
    LMI_CHECK_ARG(idx->n_rows == 0 || (idx->corpus && idx->inv_norm && idx->gpos), "null corpus arrays");
    LMI_CHECK_ARG(idx->bucket_off && idx->chunk_first, "null bucket tables");

    LMI_CHECK_ARG((c.tags != nullptr) == (c.want != nullptr) && (c.tags != nullptr) == (c.mask != nullptr),
                  "tags, value and mask come together");
    const ScanPlan w = c.plan ? *c.plan : scan_plan(idx, nq, R, k, qmode, lo_g != nullptr, c.tags != nullptr);
    if (c.ws_bytes < w.total) {
        set_error("workspace %zu B < required %zu B", c.ws_bytes, w.total);
        return LMI_E_WORKSPACE;
    }
    const bool ring = w.family != ScanKernel::General, v3 = w.family == ScanKernel::Ring8;
    // (the range search's collect form runs the general family's plan; its
    // kernel is launch_range_scan, lmi_range.hip)
    if (c.range != nullptr && (ring || c.wide != nullptr || lo_g != nullptr || out_bound != nullptr)) {
        set_error("the range scan takes the general kernel's plan alone");
        return LMI_E_UNSUPPORTED;
    }
    const ScanLaunch launch = c.range ? ScanLaunch{nullptr, nullptr} : pick_launch(w, c);
    if (!c.range && !launch.ring && !launch.general) {
        set_error("no scan kernel takes this call's wide mode, lower bounds or band lists with %d-entry lists", w.kl);
        return LMI_E_UNSUPPORTED;
    }
    // The scan in two launches (lmi_scan_set_join_workgroups, j > 0): the SCAN
    // phase launches the grid less j workgroups, the SCAN_JOIN phase the same
    // kernel with j on the workspace as it stands -- extra workers of the same
    // tile queues.  The product lists of the 8-wave ring take it (plain 10- and
    // 15-entry lists, the band lists); the plan below never sees j
    int phases = c.phases;
    {
        bool done;
        LMI_TRY(join_gate(phases, v3 && wide == nullptr && lo_g == nullptr && c.tags == nullptr, &done));
        if (done) return LMI_OK;
    }
    const bool do_plan = phases & kPhasePlan, do_scan = phases & kPhaseScan, do_merge = phases & kPhaseMerge;
    // (at least one workgroup stays in the main launch; phases & kPhaseJoin is
    // set only with j > 0)
    const int join_n = std::min(join_wgs(), num_cus() - 1);
    const bool do_join = (phases & kPhaseJoin) && join_n > 0;
    auto* ws = reinterpret_cast<unsigned char*>(c.workspace);
    const int P = nq * R;

    // the plan's per-pair initial values, written by prep: pair_bucket = -1
    // (pairs whose class is out of range are never filled), pair_pos = -1 (the
    // seed), split_mask = 0, the per-pair bounds thr_g = all ones (scan v2/v3)
    PrepFills fills{};
    const bool seed = c.seed_r0 && v3 && !(lo_g != nullptr) && R > 1;
    // the float64 mode's band lists (out_bound: every pair's bound of its
    // unlisted rows, +inf until the merge writes it)
    const bool band = out_bound != nullptr;
    auto add = [&](void* ptr, uint32_t v, int per_q) {
        fills.p[fills.n] = reinterpret_cast<uint32_t*>(ptr);
        fills.v[fills.n] = v;
        fills.per_q[fills.n] = per_q;
        ++fills.n;
    };
    if (band) add(out_bound, 0x7f800000u, R);
    if (c.range) add(c.range->ccount, 0u, R);
    if (idx->n_rows > 0) {
        add(ws + w.pair_bucket, 0xffffffffu, R);
        if (seed) add(ws + w.pair_pos, 0xffffffffu, R);
        add(ws + w.split_mask, 0u, R);
        if (ring) add(ws + w.thr_g, 0xffffffffu, 2 * R);
    }
    if (do_plan && w.i8) {
        const dim3 pg((nq + kThreads / 64 - 1) / (kThreads / 64));
        const bool vec = ((uintptr_t)c.q % 16 == 0) && (ldq % 4 == 0);
        hipLaunchKernelGGL(vec ? prep_i8_kernel<true> : prep_i8_kernel<false>, pg, dim3(kThreads), 0, s, c.q, nq,
                           ldq, idx->d, idx->d_pad, (int8_t*)(ws + w.qbuf), (float*)(ws + w.invq), out_d, out_pos,
                           out_row, c.prefill ? R * ldo : 0, fills);
        LMI_LAUNCH_CHECK("prep_i8_kernel");
    } else if (do_plan) {
        const dim3 pg((nq + kThreads / 64 - 1) / (kThreads / 64));
        const bool vec = ((uintptr_t)c.q % 16 == 0) && (ldq % 4 == 0);
        auto* kp = w.f16math ? (vec ? prep_kernel<true, true> : prep_kernel<true, false>)
                             : (vec ? prep_kernel<false, true> : prep_kernel<false, false>);
        hipLaunchKernelGGL(kp, pg, dim3(kThreads), 0, s, c.q, nq, ldq, idx->d, idx->d_pad,
                           (void*)(ws + w.qbuf), (float*)(ws + w.invq), status, out_d, out_pos,
                           out_row, c.prefill ? R * ldo : 0, fills);
        LMI_LAUNCH_CHECK("prep_kernel");
    }
    if (idx->n_rows == 0) {
        // (an empty shard lists nothing: its kth block is all +inf)
        if (kth_out != nullptr && do_merge) LMI_TRY(fill_u32(kth_out, 0x7f800000u, (size_t)P * c.kth_k, s));
        return LMI_OK;
    }

    int32_t* counts = (int32_t*)(ws + w.counts);
    int32_t* pair_q = (int32_t*)(ws + w.pair_q);
    int32_t* pair_bucket = (int32_t*)(ws + w.pair_bucket);
    Tile* tiles = (Tile*)(ws + w.tiles);
    int32_t* meta = (int32_t*)(ws + w.ntiles);
    int32_t* work = (int32_t*)(ws + w.work);
    const int C = idx->n_buckets;
    int ng = clamp_knob(env_config().scan_groups, kGroups, 1, kGroups);
    while (ng & (ng - 1)) ng &= ng - 1;

    // (pair_bucket = -1 marks pairs whose class is out of range: never filled)
    if (do_plan) {
        hipLaunchKernelGGL(plan_count_kernel, dim3(C), dim3(kPlanThreads), 0, s, classes, P, counts);
        LMI_LAUNCH_CHECK("plan_count_kernel");
    }
    // (the seed reads the pair position of every (q, 0); pairs whose class is
    // out of range keep -1)
    int32_t* pair_pos = seed ? (int32_t*)(ws + w.pair_pos) : nullptr;
    // tail split (where the plan has parts): K = the queue's share of the grid;
    // plan_fill leaves K (S - 1) free slots after every queue for its parts
    // (not in the wide path's bound scan: its lists are the bucket's own)
    const int split_k = w.split_s < 2 || (wide && wide->mode == 1) ? 0
                        : std::min(kSplitMaxK, env_config().scan_split > 0 ? env_config().scan_split
                                                                            : (num_cus() + ng - 1) / ng);
    const int qpad = split_k * (w.split_s - 1);
    if (do_plan) {
        hipLaunchKernelGGL(plan_fill_kernel, dim3(C), dim3(kPlanThreads), 0, s, classes, P, C, counts,
                           idx->chunk_first, w.qb, pair_q, pair_bucket, tiles, meta, work, ng, pair_pos,
                           qpad);
        LMI_LAUNCH_CHECK("plan_fill_kernel");
    }
    int32_t* seed_pos = seed ? (int32_t*)(ws + w.seed_pos) : nullptr;
    if (seed && do_plan) {
        hipLaunchKernelGGL(seed_pos_kernel, dim3((P + 255) / 256), dim3(256), 0, s, pair_q, pair_pos,
                           P, R, seed_pos);
        LMI_LAUNCH_CHECK("seed_pos_kernel");
    }
    if (do_plan && w.nearest_first) {
        int32_t* pref = (int32_t*)(ws + w.pref);
        int32_t* n_seed = (int32_t*)(ws + w.n_seed);
        hipLaunchKernelGGL(pref_kernel, dim3((P + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads),
                           0, s, pair_bucket, idx->chunk_first, idx->chunk_centroid, idx->d_pad,
                           (const _Float16*)(ws + w.qbuf), pair_q, R, P, pref);
        LMI_LAUNCH_CHECK("pref_kernel");
        hipLaunchKernelGGL(pref_sort_kernel, dim3(C), dim3(kThreads), 0, s, counts, idx->chunk_first,
                           pair_q, pref, (int32_t*)(ws + w.pref_tmp), (int32_t*)(ws + w.pref_tmp2), w.qb,
                           n_seed);
        LMI_LAUNCH_CHECK("pref_sort_kernel");
        hipLaunchKernelGGL(tile3_fill_kernel, dim3(C), dim3(kThreads), 0, s, counts, idx->chunk_first,
                           pref, n_seed, C, w.qb, tiles, meta, work);
        LMI_LAUNCH_CHECK("tile3_fill_kernel");
    }
    if (w.nearest_first) ng = 1;  // one queue: seed tiles strictly first

    // tail split (scan v3; not after the nearest-chunk-first plan: its queue
    // has no seed count)
    uint32_t* split_mask = (uint32_t*)(ws + w.split_mask);
    const int64_t* scan_off = idx->bucket_off;
    if (split_k > 0) {
        if (do_plan)
            hipLaunchKernelGGL(tail_split_kernel, dim3(kGroups), dim3(256), 0, s, tiles, meta,
                               idx->bucket_off, (int64_t*)(ws + w.ext_off), C, idx->chunk_rows,
                               std::max(idx->max_chunks, 1), split_k, w.split_s, split_mask);
        LMI_LAUNCH_CHECK("tail_split_kernel");
        scan_off = (const int64_t*)(ws + w.ext_off);
    }

    // the collect scan: every grouped pair's fixed bound (0 = takes nothing)
    // and its candidate count
    if (wide && wide->mode == 2 && do_scan) {
        hipLaunchKernelGGL(set_bound_kernel, dim3((P + 255) / 256), dim3(256), 0, s, pair_q, P,
                           wide->bound_ord, (unsigned long long*)(ws + w.thr_g), wide->ccount, pair_bucket,
                           idx->bucket_off, wide->app_d, wide->app_row, wide->app_k, wide->cand, wide->cap);
        LMI_LAUNCH_CHECK("set_bound_kernel");
    }

    ScanArgs a{};
    a.corpus = idx->corpus;
    a.d_pad = idx->d_pad;
    a.inv_norm = idx->inv_norm;
    a.bucket_off = idx->bucket_off;
    a.chunk_rows = idx->chunk_rows;
    a.max_chunks = w.list_stride;  // the partial-list stride (+ split parts)
    a.qbuf = ws + w.qbuf;
    a.invq = (const float*)(ws + w.invq);
    a.pair_q = pair_q;
    a.R = R;
    a.tiles = tiles;
    a.meta = meta;
    a.work = work;
    a.partial = (uint64_t*)(ws + w.partial);
    a.gpos = idx->gpos;
    a.lo_g = lo_g;
    a.tags = c.tags;
    if (c.tags != nullptr) {
        // every tagged kernel reads (1/|q|, value, mask) triples: packed behind
        // the plan's pair arrays, in the nearest-chunk-first plan's scratch
        // (pref, pref_tmp, pref_tmp2: laid out one after the other, 3 P words
        // >= 3 nq), which a tagged call never uses.  The 8-wave ring takes them
        // as its invq (no pointer more in its scalar registers), the general
        // kernel and the range scan as their want.
        uint32_t* iw = reinterpret_cast<uint32_t*>(ws + w.pref);
        if (do_plan) {
            hipLaunchKernelGGL(want_pack_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, a.invq, c.want, c.mask,
                               nq, iw);
            LMI_LAUNCH_CHECK("want_pack_kernel");
        }
        a.want = iw;
    }

    // (the phases split the general kernel's call as they split the rings':
    // everything a later phase reads -- the rounded queries, the tile plan,
    // the work counter, the partial lists -- lives in the workspace)
    if (ring && (do_scan || do_join)) {
        Scan2Args b{};
        b.corpus = reinterpret_cast<const _Float16*>(idx->corpus);
        b.inv_norm = idx->inv_norm;
        b.bucket_off = scan_off;
        b.chunk_rows = idx->chunk_rows;
        b.max_chunks = a.max_chunks;
        b.qbuf = reinterpret_cast<const _Float16*>(ws + w.qbuf);
        b.invq = a.invq;
        b.pair_q = pair_q;
        b.R = R;
        b.tiles = tiles;
        b.meta = meta;
        b.work = work;
        b.partial = a.partial;
        b.thr_g = reinterpret_cast<unsigned long long*>(ws + w.thr_g);  // (reset by prep)
        b.gpos = idx->gpos;
        b.lo_g = lo_g;
        b.pair_pos = seed_pos;
        b.seed_margin = c.seed_margin;
        // (MODE 3: 2 eps = the seed margin of the float64 mode, rounded up,
        // + 2^-22 for the rounding of bound + band, distances being < 4)
        b.band = band ? c.seed_margin * (1.0f + 0x1p-20f) + 0x1p-22f : 0.0f;
        b.ng = ng;
        b.lag = std::max(0, std::min(3, env_config().scan_lag));
        if (c.tags != nullptr) {
            // (MODE 4 reads the triples packed above in place of 1/|q| alone)
            b.invq = reinterpret_cast<const float*>(a.want);
            b.tags = c.tags;
        }
        if (wide) {
            b.cand = wide->cand;
            b.ccount = wide->ccount;
            b.cap = wide->cap;
            b.bins = wide->bins;
            b.nbins = wide->nbins;
            b.sub_rows = wide->sub_rows;
            b.sub_take = wide->sub_take;
        }
        if (do_scan && join_n > 0) {
            const ScanGrid grid(num_cus() - join_n);
            LMI_TRY(launch.ring(b, s));
        } else if (do_scan) {
            LMI_TRY(launch.ring(b, s));
        }
        if (do_join) {
            const ScanGrid grid(join_n);
            LMI_TRY(launch.ring(b, s));
        }
    } else if (c.range && do_scan) {
        const RangeArgs ra{a, c.range->bound, c.range->cand, c.range->ccount, c.range->cap};
        LMI_TRY(launch_range_scan(ra, w.f16math, idx->dtype == LMI_F16, s));
    } else if (!ring && do_scan) {
        LMI_TRY(launch.general(a, idx->d_pad, s));
    }
    if (!do_merge) return LMI_OK;

    const int grid = (int)(((int64_t)P * kMergeLanes + kMergeBlock - 1) / kMergeBlock);
    if (band) {
        hipLaunchKernelGGL(chunk_merge_band_kernel, dim3(grid), dim3(kMergeBlock), 0, s, a.partial, a.max_chunks,
                           pair_q, pair_bucket, idx->chunk_first, idx->gpos, P, k, ldo, out_d, out_pos,
                           out_row, out_bound, idx->n_rows, status, split_mask, w.split_s, kth_out, c.kth_k,
                           classes, C);
        LMI_LAUNCH_CHECK("chunk_merge_band_kernel");
        return LMI_OK;
    }
#define LMI_CM(KLV, ROWSV)                                                                         \
    hipLaunchKernelGGL((chunk_merge_kernel<KLV, ROWSV>), dim3(grid), dim3(kMergeBlock), 0, s, a.partial, \
                       a.max_chunks, pair_q, pair_bucket, idx->chunk_first, idx->gpos, P, k, ldo,  \
                       out_d, out_pos, out_row, idx->n_rows, status, split_mask, w.split_s)
    if (w.kl == 10) {
        if (out_row) LMI_CM(10, true); else LMI_CM(10, false);
    } else if (w.kl == 15) {
        if (out_row) LMI_CM(15, true); else LMI_CM(15, false);
    } else {
        if (out_row) LMI_CM(16, true); else LMI_CM(16, false);
    }
#undef LMI_CM
    LMI_LAUNCH_CHECK("chunk_merge_kernel");
    return LMI_OK;
}

extern "C" int32_t lmi_scan_set_workgroups(int32_t wgs) {
    const int prev = lmi::t_scan_wgs;
    lmi::t_scan_wgs = wgs > 0 ? wgs : 0;
    return prev;
}

extern "C" int32_t lmi_scan_set_join_workgroups(int32_t j) {
    const int prev = lmi::t_join_wgs;
    lmi::t_join_wgs = j > 0 ? j : 0;
    return prev;
}

extern "C" int32_t lmi_scan_set_i8_lists16(int32_t on) {
    const int prev = lmi::t_i8_lists16;
    lmi::t_i8_lists16 = on != 0 ? 1 : 0;
    return prev;
}

extern "C" int lmi_scan_joinable(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k, int32_t qmode) {
    using namespace lmi;
    qmode &= ~LMI_Q_SEED_ROUND0;
    take_phases(qmode);
    if (i8_refuse("lmi_scan_joinable", idx) != LMI_OK) return 0;  // (a predicate: "no", and the message)
    if (!idx || idx->corpus32 || nq < 0 || R < 1 || k < 1 || k > LMI_MAX_K) return 0;
    return scan_plan(idx, nq, R, k, qmode).family == ScanKernel::Ring8 ? 1 : 0;
}

extern "C" int32_t lmi_scan_family(const lmi_index_desc* idx, int32_t k, int32_t qmode, int32_t tagged) {
    using namespace lmi;
    if (!idx) {
        set_error("lmi_scan_family: null index");
        return -LMI_E_INVALID;
    }
    if (const int rc = i8_gate("lmi_scan_family", idx, k, qmode); rc != LMI_OK) return -rc;
    qmode &= ~LMI_Q_SEED_ROUND0;
    take_phases(qmode);
    if (k < 1 || k > LMI_MAX_K || (qmode != LMI_Q_F16 && qmode != LMI_Q_F32 && qmode != LMI_Q_I8)) {
        set_error("lmi_scan_family: k=%d outside [1, %d] or qmode 0x%x not a query class", k, LMI_MAX_K, qmode);
        return -LMI_E_INVALID;
    }
    return (int32_t)scan_plan(idx, 0, 1, k, qmode, false, tagged != 0).family;
}

extern "C" int lmi_timing_enable(int32_t on) {
    lmi::Timing& t = lmi::timing();
    std::lock_guard<std::mutex> g(t.mu);
    t.on = on != 0;
    return LMI_OK;
}

extern "C" int32_t lmi_timing_read(float* ms_out, int32_t max_n) {
    using namespace lmi;
    Timing& t = timing();
    std::lock_guard<std::mutex> g(t.mu);
    int32_t n = 0;
    for (auto& pr : t.pending) {
        if (hipEventSynchronize(pr.second) != hipSuccess) {
            set_error("hipEventSynchronize failed");
            return -LMI_E_HIP;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) != hipSuccess) {
            set_error("hipEventElapsedTime failed");
            return -LMI_E_HIP;
        }
        if (ms_out && n < max_n) ms_out[n] = ms;
        ++n;
        t.pool.push_back(pr);
    }
    t.pending.clear();
    return std::min(n, max_n);
}
