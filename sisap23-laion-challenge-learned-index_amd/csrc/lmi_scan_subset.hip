// The subset scan (include/lmi_hip.h, lmi_bucket_topk_subset): K2 over the rows
// of an explicit allow-list alone.  Every other scan reads all rows of a probed
// bucket and, filtered, tests a tag word in its epilogue; this one fetches the
// allowed rows by position, so its bytes follow the subset, not the corpus.  It
// is the many-query, indirect-row sibling of scan_few_kernel (lmi_scan_few.hip):
// the same query image, ring, MFMA order, epilogue and lists.  Its own:
//
//   input      sub_pos [n_sub] the allowed rows, ascending (so sorted by
//              bucket), and sub_off [C + 1]: bucket c's are sub_pos[sub_off[c]
//              .. sub_off[c + 1]) -- its range.
//   item       (bucket c, a group of <= 32 of the pairs probing c, a slice of
//              sub_rows entries of c's range).  subset_plan_kernel lists the
//              (bucket, group)s of the scan's grouped pairs with their first
//              item, for any number of pairs and buckets (one workgroup, a
//              prefix sum over the buckets); a persistent grid of one workgroup
//              per CU takes items in that order, so a workgroup that stays
//              inside a group stages its queries once.  A bucket probed by
//              more than 32 pairs has several groups, and each group reads the
//              bucket's subset rows again: g groups of a range of n entries
//              move g * n * 2 d_pad bytes, of which n * 2 d_pad come from HBM
//              and the rest out of L2 while the groups' items run side by side
//              (10 000 queries, R = 4 on 122 buckets: 328 pairs = 11 groups a
//              bucket, so 1/64 of 10M x 768 rows is 0.24 GB from HBM and
//              2.6 GB through L2; the whole index 15.4 GB and 169 GB -- past a
//              few groups a bucket the tiled scans, 256 pairs a tile, are the
//              better kernels, and nothing picks this one for the caller).
//   rows       a wave owns whole 32-entry blocks of the slice (block b: wave b
//              mod 4).  Lane l loads entry l & 31 of a block, its row (taken
//              relative to the bucket's first); a ds_bpermute hands row 4 u + (lane >> 4)
//              to the lanes of DMA u, whose source address is row * 2 d_pad +
//              the XOR-swizzled chunk -- the few scan's 256-B row image and
//              three-stage ring, with a per-lane row.  The block's norms are
//              gathered the same way (row * 4).  Entries past the slice's end
//              are clamped to its last; the epilogue takes lanes below
//              valid_rows alone.  The buffer descriptors span the bucket's rows
//              and no more, so whatever sub_pos holds, nothing outside the
//              bucket is read (hence a bucket below 2 GiB).
//   positions  live in registers, one a lane and block, in a queue of four: the
//              blocks the wave computes (0), may issue (0 .. 2: the ring is two
//              stages ahead, each a block of its own at d_pad <= 128) and the
//              one in flight (3), loaded when the wave moves on to its next
//              block -- at least one stage before a DMA consumes it.  LDS has
//              no room: at d_pad 992 the query image and the rings fill all
//              160 KiB.  And a position in LDS would have to be read back
//              inside the ring, by asm the compiler cannot count, where a
//              register load is waited for by the compiler's own vmcnt.  Loads
//              return in order, so the wait a block's first issue needs covers
//              the stage consumed next and could leave the newer stage in
//              flight; hipcc's count there is the conservative one (all but
//              the newest load), so the ring is one stage shallower at a block
//              boundary -- once per nseg stages.  Not tuned further.
//   epilogue   the few scan's; the key's position is the gathered row (a
//              bpermute of the block's register), not the slice-local one.
//   merge      few_merge_kernel itself, on sub_off and sub_rows: a pair's
//              slice lists -> k by (distance, position).
#include "lmi_few_lds.hpp"
#include "lmi_scan_internal.hpp"

#include <algorithm>

namespace lmi {
namespace {

// (the ring's shape and the group table's are the few scan's: namespace few, lmi_few_lds.hpp)
namespace sub {
using namespace few;
constexpr int PLAN_THREADS = 1024;
}  // namespace sub

struct SubArgs {
    const _Float16* corpus;
    const float* inv_norm;
    const int64_t* bucket_off;
    const int32_t* sub_pos;  // [n_sub] rows, ascending
    const int64_t* sub_off;  // [C + 1] the buckets' ranges of sub_pos
    int32_t d_pad, sub_rows, max_slices, R;
    const _Float16* qbuf;   // [nq][d_pad]
    const float* invq;      // [nq]
    const int32_t* pair_q;  // [P] pair ids grouped by bucket (the scan's plan)
    const int32_t* tab;     // subset_plan_kernel's groups: (c, pp0, np, item0, slices)
    int32_t* work;          // the item counter
    unsigned long long* thr_g;  // [P] the pairs' bounds (grouped position)
    uint64_t* partial;      // [P][max_slices][KL]
};

size_t sub_lds_bytes(int d_pad) {
    return (size_t)32 * (d_pad + sub::QPAD) * 2 + (size_t)kWaves * sub::NSLOT * (sub::STAGE + sub::NORMB);
}

// The (bucket, group)s of a call and each one's first item, from the plan's
// pairs per bucket (counts; the grouped pairs of bucket c start at the sum of
// the counts before it) and the buckets' ranges.  One workgroup: thread t takes
// the buckets [t bpt, (t + 1) bpt), an inclusive scan over the threads' sums of
// (pairs, groups, items) places them.  A bucket with no pair or no entry has no
// group.  It also clears the item counter and the bounds.  A range longer than
// max_slices slices (the caller's max_range was wrong) gets no item, its pairs
// leave the merge (pair_bucket = -1) and the status says so.
__global__ __launch_bounds__(sub::PLAN_THREADS) void subset_plan_kernel(
    const int32_t* __restrict__ counts, const int64_t* __restrict__ sub_off, int32_t C, int32_t P, int32_t sub_rows,
    int32_t max_slices, int32_t* __restrict__ pair_bucket, int32_t* __restrict__ tab, int32_t* __restrict__ work,
    unsigned long long* __restrict__ thr_g, int32_t* __restrict__ status) {
    using namespace sub;
    __shared__ int sp[PLAN_THREADS], sg[PLAN_THREADS], si[PLAN_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += PLAN_THREADS) thr_g[i] = kEmptyKey;
    if (tid == 0) work[0] = 0;
    const int bpt = (C + PLAN_THREADS - 1) / PLAN_THREADS;
    const int c0 = std::min(C, tid * bpt), c1 = std::min(C, c0 + bpt);
    auto slices_of = [&](int c) {
        const int64_t ns = (sub_off[c + 1] - sub_off[c] + sub_rows - 1) / sub_rows;
        return ns > max_slices ? -1 : (int)ns;
    };
    int npair = 0, ngrp = 0, nitem = 0;
    for (int c = c0; c < c1; ++c) {
        const int cnt = counts[c], ns = std::max(0, slices_of(c));
        const int g = ns > 0 ? (cnt + 31) / 32 : 0;
        npair += cnt;
        ngrp += g;
        nitem += g * ns;
    }
    sp[tid] = npair;
    sg[tid] = ngrp;
    si[tid] = nitem;
    __syncthreads();
    for (int off = 1; off < PLAN_THREADS; off <<= 1) {
        const int a = tid >= off ? sp[tid - off] : 0, b = tid >= off ? sg[tid - off] : 0,
                  c = tid >= off ? si[tid - off] : 0;
        __syncthreads();
        sp[tid] += a;
        sg[tid] += b;
        si[tid] += c;
        __syncthreads();
    }
    int pp = sp[tid] - npair, g = sg[tid] - ngrp, item = si[tid] - nitem;
    for (int c = c0; c < c1; ++c) {
        const int cnt = counts[c], ns = slices_of(c);
        if (ns < 0 && cnt > 0) {
            atomicOr(status, LMI_STATUS_INTERNAL);
            for (int i = 0; i < cnt; ++i) pair_bucket[pp + i] = -1;
        }
        for (int p0 = 0; ns > 0 && p0 < cnt; p0 += 32) {
            int32_t* e = tab + TAB_HDR + TAB_ENT * g;
            e[0] = c;
            e[1] = pp + p0;
            e[2] = std::min(32, cnt - p0);
            e[3] = item;
            e[4] = ns;
            ++g;
            item += ns;
        }
        pp += cnt;
    }
    if (tid == PLAN_THREADS - 1) {
        tab[0] = sg[tid];
        tab[1] = si[tid];
    }
}

template <int KL>
__global__ __launch_bounds__(kThreads, 1) void scan_subset_kernel(SubArgs a) {
    using namespace sub;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int d_pad = a.d_pad;
    const int ldq = d_pad + QPAD;
    const uint32_t qs_bytes = 32u * (uint32_t)ldq * 2u;
    _Float16* Qs = reinterpret_cast<_Float16*>(smem);
    // (the item and its group wait in the last query row's pad, as in the few scan)
    int* s_ctl = reinterpret_cast<int*>(smem + qs_bytes - 16);
    unsigned char* ring_all = smem + qs_bytes;
    unsigned char* norm_all = ring_all + kWaves * NSLOT * STAGE;
    uint64_t* mergebuf = reinterpret_cast<uint64_t*>(ring_all);  // over the drained rings
    static_assert((size_t)32 * 2 * kWaves * 16 * sizeof(uint64_t) <= (size_t)kWaves * NSLOT * STAGE, "merge buffer");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int col = lane & 31;
    unsigned char* ring = ring_all + wave * NSLOT * STAGE;
    unsigned char* norms = norm_all + wave * NSLOT * NORMB;
    const uint32_t ring_a = (uint32_t)(uintptr_t)ring;
    const uint32_t norm_a = (uint32_t)(uintptr_t)norms + (uint32_t)h * 16u;
    // A fragment s of a stage: row col, chunk 2 s + h, stored at chunk ^ (col & 15)
    uint32_t aoff[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) aoff[s] = (uint32_t)(col * ROWB + (((2 * s + h) ^ (col & 15)) * 16));
    // B fragment s of segment j: query col, k = 128 j + 16 s + 8 h
    const uint32_t q_a = (uint32_t)(uintptr_t)Qs + (uint32_t)(col * ldq * 2 + h * 16);
    const int nseg = (d_pad + KSEG - 1) / KSEG;
    const uint32_t row_bytes = (uint32_t)d_pad * 2u;
    const int n_groups = a.tab[0], n_items = a.tab[1];

    int cur_group = -1;
    for (;;) {
        if (tid == 0) {
            const int it = atomicAdd(a.work, 1);
            int g = -1;
            if (it < n_items) {
                int lo = 0, hi = n_groups - 1;  // the last group whose first item is <= it
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (a.tab[TAB_HDR + TAB_ENT * mid + 3] <= it) lo = mid;
                    else hi = mid - 1;
                }
                g = lo;
            }
            s_ctl[0] = it;
            s_ctl[1] = g;
        }
        __syncthreads();
        const int item = __builtin_amdgcn_readfirstlane(s_ctl[0]);
        const int g = __builtin_amdgcn_readfirstlane(s_ctl[1]);
        if (g < 0) break;
        const int32_t* e = a.tab + TAB_HDR + TAB_ENT * g;
        const int c = e[0], pp0 = e[1], np = e[2];
        const int slice = item - e[3];
        const int64_t e0 = a.sub_off[c] + (int64_t)slice * a.sub_rows;
        const int nent =
            __builtin_amdgcn_readfirstlane((int)std::min<int64_t>(a.sub_rows, a.sub_off[c + 1] - e0));
        const int32_t* spos = a.sub_pos + e0;
        const int64_t brow0 = a.bucket_off[c];
        const uint32_t brows = (uint32_t)(a.bucket_off[c + 1] - brow0);

        // ---- the group's queries, once per group --------------------------
        if (g != cur_group) {
            const int vpr = d_pad / 8;
            for (int i = tid; i < 32 * vpr; i += kThreads) {
                const int r = i / vpr, v = i - r * vpr;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (r < np) {
                    const int q = a.pair_q[pp0 + r] / a.R;
                    val = *reinterpret_cast<const uint4*>(a.qbuf + (size_t)q * d_pad + v * 8);
                }
                *reinterpret_cast<uint4*>(Qs + r * ldq + v * 8) = val;
            }
            cur_group = g;
        }
        const bool live = col < np;
        const float my_invq = live ? a.invq[a.pair_q[pp0 + col] / a.R] : 0.0f;
        // the lane's bound: the pair's (distance part: slices run concurrently)
        // until its own list fills; dead slots reject everything
        uint64_t thr = live ? (__hip_atomic_load(&a.thr_g[pp0 + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                               0xffffffffull)
                            : 0ull;
        __syncthreads();

        uint64_t L[KL];
        list_clear<KL>(L);

        // (the bucket's rows and no more: a row outside them reads zeros)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.corpus + brow0 * d_pad), (short)0, (int)(brows * row_bytes), 0x00020000);
        const __amdgpu_buffer_rsrc_t rn =
            __builtin_amdgcn_make_buffer_rsrc((void*)(a.inv_norm + brow0), (short)0, (int)(brows * 4u), 0x00020000);
        const int nblk = (nent + 31) / 32;
        const int nmy = nblk > wave ? (nblk - wave + kWaves - 1) / kWaves : 0;  // blocks wave, wave + 4, ..
        const int nst = nmy * nseg;

        // entry lane & 31 of the wave's block bi (past the slice's end: its last
        // entry): its row.  Nothing is computed on it here and no branch joins
        // it: a use would wait for the load
        const uint32_t brow_lo = (uint32_t)brow0;
        auto load_pos = [&](int bi) -> uint32_t {
            return (uint32_t)spos[std::min((wave + kWaves * bi) * 32 + col, nent - 1)];
        };
        // the wave's blocks cb .. cb + 3
        uint32_t p0 = load_pos(0), p1 = load_pos(1), p2 = load_pos(2), p3 = load_pos(3);
        int cb = 0;
        // the issuing block's row offsets of DMA u (row 4 u + (lane >> 4)) and of the norm DMA
        uint32_t ro[8], rno = 0;

        // stage t = (the wave's block t / nseg, segment t % nseg) into slot t % 3
        // (pq: the queue entry of its block, chosen by the caller -- a lambda
        // that chose among captured registers would keep them in memory)
        auto issue = [&](int t, uint32_t pq) {
            const int bi = t / nseg, j = t - bi * nseg;
            const int slot = t % NSLOT;
            const int cv = std::min(16, (d_pad - j * KSEG) / 8);  // the segment's chunks of a row
            if (j == 0) {
                const uint32_t pv = pq - brow_lo;
                rno = pv * 4u;
#pragma unroll
                for (int u = 0; u < STAGE / 1024; ++u)
                    ro[u] = (uint32_t)__shfl((int)pv, 4 * u + (lane >> 4)) * row_bytes;
            }
#pragma unroll
            for (int u = 0; u < STAGE / 1024; ++u) {
                const int rb = 4 * u + (lane >> 4);
                int cs = (lane & 15) ^ (rb & 15);
                cs = cs < cv ? cs : 0;
                const uint32_t vo = ro[u] + (uint32_t)(j * ROWB + cs * 16);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(ring + slot * STAGE + u * 1024), 16, vo, 0, 0,
                                                         0);
            }
            // (every stage brings its block's norms to its own slot: one DMA
            // count per stage, whatever the width)
            if (lane < 32)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rn, (lds_t)(norms + slot * NORMB), 4, rno, 0, 0, 0);
        };
        if (nst > 0) issue(0, p0);
        if (nst > 1) issue(1, nseg > 1 ? p0 : p1);

        f32x16 acc;
        for (int t = 0; t < nst; ++t) {
            const int bi = t / nseg, j = t - bi * nseg;
            if (t + 2 < nst) {
                const int dq = (t + 2) / nseg - cb;
                issue(t + 2, dq == 0 ? p0 : dq == 1 ? p1 : p2);
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * DMAS));
            } else if (t + 1 < nst) {
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(DMAS));
            } else {
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
            }
            if (j == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            }
            const int slot = t % NSLOT;
            const uint32_t sa = ring_a + (uint32_t)(slot * STAGE);
            half8 A[8], B[8];
            lds_read4(A, 0, sa + aoff[0], sa + aoff[1], sa + aoff[2], sa + aoff[3]);
            lds_read4(A, 4, sa + aoff[4], sa + aoff[5], sa + aoff[6], sa + aoff[7]);
            const int nm = std::min(8, (d_pad - j * KSEG) / 16);  // (the last segment may be short: 2, 4 or 6)
            const uint32_t qa = q_a + (uint32_t)(j * ROWB);
            if (nm == 8) {
                lds_read8_affine(B, qa);
            } else {
                lds_read2_affine<0>(B, qa);
                if (nm > 2) lds_read2_affine<2>(B, qa);
                if (nm > 4) lds_read2_affine<4>(B, qa);
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s < nm) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[s], B[s], acc, 0, 0, 0);
            if (j + 1 < nseg) continue;

            // ---- the block's epilogue (lane: column col, rows (reg & 3) + 8 (reg >> 2) + 4 h)
            const int b = wave + kWaves * bi;
            const int valid_rows = nent - b * 32;
            f32x4 n4[4];
            lds_read_norms(n4, norm_a + (uint32_t)(slot * NORMB));
            const float bound = key_dist_bound(thr);
            float dv[16];
            uint32_t mask = 0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                dv[reg] = fmaf(-acc[reg], my_invq * n4[reg >> 2][reg & 3], 1.0f);
                mask |= (i < valid_rows && dv[reg] <= bound) ? 1u << reg : 0u;
            }
            if (__any(mask != 0)) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const bool ok = (mask >> reg) & 1u;
                    if (__any(ok)) {
                        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        // (the gathered row: entry i of the block is in lane i's register)
                        const uint32_t row = (uint32_t)__shfl((int)p0, i);
                        const uint64_t key = make_key(dv[reg], row);
                        if (ok && key < L[KL - 1]) list_insert<KL>(L, key);
                    }
                }
            }
            thr = std::min(thr, L[KL - 1]);
            // the wave moves on to its next block
            p0 = p1;
            p1 = p2;
            p2 = p3;
            p3 = load_pos(bi + 4);
            ++cb;
        }
        __syncthreads();  // every wave's ring is drained and read

        // ---- the column's 2 * kWaves lists -> the (pair, slice) list -------
        {
            uint64_t* dst = mergebuf + ((size_t)col * (2 * kWaves) + 2 * wave + h) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) dst[i] = L[i];
        }
        __syncthreads();
        if (tid < np) {
            const uint64_t* src = mergebuf + (size_t)tid * (2 * kWaves) * KL;
            uint64_t M[KL];
#pragma unroll
            for (int i = 0; i < KL; ++i) M[i] = src[i];
            for (int l = 1; l < 2 * kWaves; ++l) {
                for (int i = 0; i < KL; ++i) {
                    const uint64_t key = src[l * KL + i];
                    if (key >= M[KL - 1]) break;
                    list_insert<KL>(M, key);
                }
            }
            uint64_t* out = a.partial + ((size_t)(pp0 + tid) * a.max_slices + slice) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) out[i] = M[i];
            if (M[KL - 1] != kEmptyKey) atomicMin(&a.thr_g[pp0 + tid], (unsigned long long)M[KL - 1]);
        }
        __syncthreads();  // the merge buffer is the next item's rings
    }
}

// ---- host ---------------------------------------------------------------------
// The call's layout: the scan's own plan (whose plan phase rounds the queries,
// fills the outputs and groups the pairs) and, behind it, this path's arrays.
struct SubPlan {
    ScanPlan base;
    int32_t kl, sub_rows, max_slices;
    size_t n_tab, tab, work, thr_g, partial, total;
};

// the (bucket, group)s a call can have: a group per 32 pairs and one more per probed bucket
size_t sub_max_groups(const lmi_index_desc* idx, int32_t nq, int32_t R) {
    const int64_t P = (int64_t)nq * R;
    return (size_t)(P / 32 + std::min<int64_t>(P, idx->n_buckets) + 1);
}

// sub_rows = 0: slices such that the call cuts into about six items per CU,
// taking the probed buckets for distinct, their pairs for evenly spread and
// their ranges for the mean one; floor 256 entries, cap the longest range.
int32_t sub_rows_of(const lmi_index_desc* idx, int64_t n_sub, int32_t max_range, int32_t nq, int32_t R,
                    int32_t sub_rows) {
    const int64_t cap = std::max<int64_t>(32, ((int64_t)max_range + 31) / 32 * 32);
    if (sub_rows > 0) return (int32_t)std::min<int64_t>(sub_rows, cap);
    const int64_t P = std::max<int64_t>(1, (int64_t)nq * R), C = idx->n_buckets;
    const int64_t probed = std::min(P, C);
    const int64_t groups = probed * (((P + probed - 1) / probed + 31) / 32);
    const int64_t per = groups * ((n_sub + C - 1) / C) / (6 * (int64_t)num_cus());
    return (int32_t)std::min<int64_t>(std::max<int64_t>(256, (per + 31) / 32 * 32), cap);
}

int sub_gate(const char* fn, const lmi_index_desc* idx, int64_t n_sub, int32_t max_range, int32_t nq, int32_t R,
             int32_t k, int32_t sub_rows) {
    LMI_CHECK_ARG(idx != nullptr, "%s: null index", fn);
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < ((int64_t)1 << 30), "%s: bad nq/R (%d, %d)", fn, nq, R);
    LMI_CHECK_ARG(sub_rows >= 0 && sub_rows % 32 == 0,
                  "%s: the subset scan takes sub_rows=%d as a positive multiple of 32 (0: the call chooses)", fn,
                  sub_rows);
    LMI_CHECK_ARG(k >= 1, "%s: the subset scan takes k >= 1, not %d", fn, k);
    LMI_CHECK_ARG(idx->d >= 1 && idx->d_pad >= idx->d && idx->d_pad % 32 == 0, "%s: bad d/d_pad", fn);
    LMI_CHECK_ARG(idx->n_buckets >= 1, "%s: n_buckets < 1", fn);
    LMI_CHECK_ARG(idx->chunk_rows >= 32 && idx->chunk_rows % 32 == 0, "%s: chunk_rows must be a multiple of 32", fn);
    LMI_CHECK_ARG(n_sub >= 0 && n_sub <= std::max<int64_t>(idx->n_rows, 0) && max_range >= 0 && max_range <= n_sub,
                  "%s: the subset scan takes 0 <= max_range <= n_sub <= n_rows (%d, %lld)", fn, max_range,
                  (long long)n_sub);
    LMI_CHECK_ARG(join_wgs() == 0, "%s: the subset scan takes no join workgroups (lmi_scan_set_join_workgroups)", fn);
    auto unsupported = [&](bool bad, const char* what) {
        if (bad) set_error("%s: the subset scan takes %s", fn, what);
        return bad;
    };
    const int64_t bucket_bytes = (int64_t)std::max(idx->max_chunks, 1) * idx->chunk_rows * idx->d_pad * 2;
    if (unsupported(k > LMI_MAX_K, "k <= 16") ||
        unsupported(idx->dtype != LMI_F16, "the fp16 storage alone (LMI_F16)") ||
        unsupported(idx->d_pad > kFewMaxDPad, "d_pad <= 992") ||
        unsupported(idx->corpus32 || idx->corpus64, "no split mode and no float64 rows (corpus32 / corpus64)") ||
        unsupported(idx->chunk_centroid != nullptr, "no sub-cluster layout (chunk_centroid)") ||
        unsupported(bucket_bytes >= ((int64_t)1 << 31), "buckets below 2 GiB of rows (max_chunks * chunk_rows)"))
        return LMI_E_UNSUPPORTED;
    const int64_t slices = (std::max<int64_t>(max_range, 1) + 31) / 32;  // (at most: the smallest slice)
    if (unsupported((int64_t)sub_max_groups(idx, nq, R) * slices >= ((int64_t)1 << 31), "fewer than 2^31 work items"))
        return LMI_E_UNSUPPORTED;
    return LMI_OK;
}

SubPlan sub_plan(const lmi_index_desc* idx, int64_t n_sub, int32_t max_range, int32_t nq, int32_t R, int32_t k,
                 int32_t sub_rows) {
    SubPlan f{};
    f.base = scan_plan(idx, nq, R, k, LMI_Q_F16);
    f.kl = k <= 10 ? 10 : 16;
    f.sub_rows = sub_rows_of(idx, n_sub, max_range, nq, R, sub_rows);
    f.max_slices = std::max(1, (max_range + f.sub_rows - 1) / f.sub_rows);
    f.n_tab = sub_max_groups(idx, nq, R);
    const size_t P = (size_t)nq * R;
    size_t off = f.base.total;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    f.tab = take((sub::TAB_HDR + sub::TAB_ENT * f.n_tab) * 4);
    f.work = take(4);
    f.thr_g = take(P * 8);
    f.partial = take(P * (size_t)f.max_slices * f.kl * 8);
    f.total = off;
    return f;
}

template <int KL>
int launch_scan_subset(const SubArgs& a, hipStream_t s) {
    const size_t lds = sub_lds_bytes(a.d_pad);
    return launch_dyn_lds<scan_subset_kernel<KL>>("scan_subset_kernel", dim3(num_cus()), dim3(kThreads), lds, s, a);
}

}  // namespace

static_assert(32 * (kFewMaxDPad + sub::QPAD) * 2 + kWaves * sub::NSLOT * (sub::STAGE + sub::NORMB) <= kLdsMax,
              "LDS budget");

}  // namespace lmi

extern "C" size_t lmi_scan_subset_workspace_bytes(const lmi_index_desc* idx, int64_t n_sub, int32_t max_range,
                                                  int32_t nq, int32_t R, int32_t k, int32_t sub_rows) {
    using namespace lmi;
    if (sub_gate("lmi_scan_subset_workspace_bytes", idx, n_sub, max_range, nq, R, k, sub_rows) != LMI_OK) return 0;
    return sub_plan(idx, n_sub, max_range, nq, R, k, sub_rows).total;
}

extern "C" int lmi_bucket_topk_subset(const lmi_index_desc* idx, const int32_t* sub_pos, const int64_t* sub_off,
                                      int64_t n_sub, int32_t max_range, const float* q, int32_t nq, int32_t ldq,
                                      const int32_t* classes, int32_t R, int32_t k, int32_t sub_rows, void* workspace,
                                      size_t ws_bytes, float* out_d, int32_t* out_pos, int32_t* status,
                                      void* stream) {
    using namespace lmi;
    const char* fn = "lmi_bucket_topk_subset";
    // (every refusal comes before any launch and needs no device)
    LMI_TRY(sub_gate(fn, idx, n_sub, max_range, nq, R, k, sub_rows));
    LMI_CHECK_ARG(idx->n_rows >= 0 && idx->n_rows < (int64_t)INT32_MAX, "%s: n_rows out of range", fn);
    LMI_CHECK_ARG(ldq >= idx->d, "%s: ldq < d", fn);
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(q && classes && out_d && out_pos && status && workspace, "%s: null pointer", fn);
    LMI_CHECK_ARG(n_sub == 0 || (sub_pos && sub_off), "%s: null subset tables", fn);
    const SubPlan f = sub_plan(idx, n_sub, max_range, nq, R, k, sub_rows);
    if (ws_bytes < f.total) {
        set_error("%s: workspace %zu B < required %zu B", fn, ws_bytes, f.total);
        return LMI_E_WORKSPACE;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the scan's own plan phase: prep_kernel (queries -> fp16 + 1/|q|, the
    // status bit, the (+inf, -1) prefill) and the pairs grouped by bucket
    const ScanCall c{.idx = idx, .q = q, .nq = nq, .ldq = ldq, .classes = classes, .R = R, .k = k,
                     .qmode = LMI_Q_F16, .out_d = out_d, .out_pos = out_pos, .status = status,
                     .workspace = workspace, .ws_bytes = f.base.total, .stream = s, .phases = kPhasePlan,
                     .plan = &f.base};
    LMI_TRY(bucket_topk_impl(c));
    if (idx->n_rows == 0 || n_sub == 0) return LMI_OK;  // (the prefill is the answer)

    auto* ws = reinterpret_cast<unsigned char*>(workspace);
    const int P = nq * R;
    const int32_t* pair_q = (const int32_t*)(ws + f.base.pair_q);
    int32_t* pair_bucket = (int32_t*)(ws + f.base.pair_bucket);
    hipLaunchKernelGGL(subset_plan_kernel, dim3(1), dim3(sub::PLAN_THREADS), 0, s,
                       (const int32_t*)(ws + f.base.counts), sub_off, idx->n_buckets, P, f.sub_rows, f.max_slices,
                       pair_bucket, (int32_t*)(ws + f.tab), (int32_t*)(ws + f.work),
                       (unsigned long long*)(ws + f.thr_g), status);
    LMI_LAUNCH_CHECK("subset_plan_kernel");

    SubArgs a{};
    a.corpus = reinterpret_cast<const _Float16*>(idx->corpus);
    a.inv_norm = idx->inv_norm;
    a.bucket_off = idx->bucket_off;
    a.sub_pos = sub_pos;
    a.sub_off = sub_off;
    a.d_pad = idx->d_pad;
    a.sub_rows = f.sub_rows;
    a.max_slices = f.max_slices;
    a.R = R;
    a.qbuf = reinterpret_cast<const _Float16*>(ws + f.base.qbuf);
    a.invq = (const float*)(ws + f.base.invq);
    a.pair_q = pair_q;
    a.tab = (const int32_t*)(ws + f.tab);
    a.work = (int32_t*)(ws + f.work);
    a.thr_g = (unsigned long long*)(ws + f.thr_g);
    a.partial = (uint64_t*)(ws + f.partial);
    LMI_TRY(f.kl == 10 ? launch_scan_subset<10>(a, s) : launch_scan_subset<16>(a, s));

    return launch_few_merge(f.kl, a.partial, f.max_slices, f.sub_rows, pair_q, pair_bucket, sub_off, idx->gpos,
                            idx->n_rows, P, k, out_d, out_pos, status, s);
}
