// The few-query scan (include/lmi_hip.h, lmi_bucket_topk_few): K2 for a call of
// at most LMI_FEW_MAX_PAIRS (query, probe) pairs, the latency shape.  Every
// other scan cuts a call into (bucket, chunk, <= 256 pairs) tiles, so one query
// with R probes keeps at most R * chunks-per-bucket workgroups busy; this one
// cuts each probed bucket into row slices sized per call, so that one query
// spreads over every CU.
//
//   item       (bucket c, a group of <= 32 of the pairs probing c, a slice of
//              few_rows rows of c); few_plan_kernel lists the (bucket, group)s
//              of the existing plan's grouped pairs with their first item, the
//              items of a group being its slices in row order.  A persistent
//              grid of one workgroup per CU takes items in that order, so a
//              workgroup that stays inside a group stages its queries once.
//   queries    the group's <= 32 queries are the B operand of
//              v_mfma_f32_32x32x16_f16, in LDS for every d_pad <= 992: 32 rows
//              at a pitch of 2 d_pad + 16 B (16 rows 16 B apart mod 256: the
//              ds_read_b128 of a fragment is conflict-free); dead slots hold
//              zeros and a bound of 0, which rejects everything.
//   rows       each of the 4 waves owns whole 32-row blocks of the slice
//              (block b: wave b mod 4) and streams them through a ring of its
//              own: 3 stages of 32 rows x 128 k (8 KiB, eight 1-KiB
//              buffer_load ... lds DMAs) + the block's 32 norms (one 4-byte
//              DMA).  Two stages are in flight while one is multiplied: 64 KiB
//              of loads per CU, and no workgroup barrier until the slice ends.
//              (Two whole blocks a wave, 4 d_pad KiB, do not fit beside the
//              query image above d_pad 384; the ring holds the same bytes in
//              flight at every width.)  LDS image of a stage: row r, 16-B
//              chunk c at chunk c ^ (r & 15) of the row's 256 B -- the XOR is
//              applied to the DMA's source address, LDS stays lane-linear.
//              Every DMA address is clamped into the slice (the last row, the
//              row's first chunk), so nothing is read past the bucket, and the
//              epilogue takes rows below valid_rows alone.
//   epilogue   tile_epilogue's distance, fmaf(-acc, invq * inv_norm, 1), on the
//              accumulators; survivors of the bound go into the lane's
//              register list.  At the slice's end the 8 lists of a column are
//              merged in LDS (over the drained rings) into the (pair, slice)
//              list and the pair's bound is lowered by atomicMin.
//   few_merge_kernel  one wave per pair: its slices' lists (hundreds) -> k by
//              (distance, position), positions -> global positions.
// The LDS reads inside the stage loop are inline asm: a C++ LDS access there
// makes the compiler wait for every DMA in flight first.
#include "lmi_few_lds.hpp"
#include "lmi_scan_internal.hpp"

#include <algorithm>

namespace lmi {
namespace {

struct FewArgs {
    const _Float16* corpus;
    const float* inv_norm;
    const int64_t* bucket_off;
    int32_t d_pad, few_rows, max_slices, R;
    const _Float16* qbuf;   // [nq][d_pad]
    const float* invq;      // [nq]
    const int32_t* pair_q;  // [P] pair ids grouped by bucket (the scan's plan)
    const int32_t* tab;     // few_plan_kernel's groups: (c, pp0, np, item0, slices)
    int32_t* work;          // the item counter
    unsigned long long* thr_g;  // [P] the pairs' bounds (grouped position)
    uint64_t* partial;      // [P][max_slices][KL]
};

size_t few_lds_bytes(int d_pad) {
    return (size_t)32 * (d_pad + few::QPAD) * 2 + (size_t)kWaves * few::NSLOT * (few::STAGE + few::NORMB);
}

// The (bucket, group)s of a call and each one's first item.  The plan grouped
// the P <= 256 pairs by bucket (pair_bucket ascending over the valid positions,
// -1 behind them); position pp heads a group when it is the 32 i-th pair of its
// bucket.  One workgroup; it also clears the item counter and the bounds.
__global__ __launch_bounds__(LMI_FEW_MAX_PAIRS) void few_plan_kernel(const int32_t* __restrict__ pair_bucket,
                                                                     const int32_t* __restrict__ counts,
                                                                     const int64_t* __restrict__ bucket_off,
                                                                     int32_t P, int32_t few_rows,
                                                                     int32_t* __restrict__ tab,
                                                                     int32_t* __restrict__ work,
                                                                     unsigned long long* __restrict__ thr_g) {
    __shared__ int sb[LMI_FEW_MAX_PAIRS], sns[LMI_FEW_MAX_PAIRS];
    const int pp = threadIdx.x;
    const int b = pp < P ? pair_bucket[pp] : -1;
    sb[pp] = b;
    if (pp < P) thr_g[pp] = kEmptyKey;
    if (pp == 0) work[0] = 0;
    __syncthreads();
    int ns = 0, np = 0;
    if (b >= 0) {
        int start = pp;
        while (start > 0 && sb[start - 1] == b) --start;
        if ((pp - start) % 32 == 0) {
            np = std::min(32, start + counts[b] - pp);
            const int64_t rows = bucket_off[b + 1] - bucket_off[b];
            ns = (int)((rows + few_rows - 1) / few_rows);  // (an empty bucket has no item)
        }
    }
    sns[pp] = ns;
    __syncthreads();
    int g = 0, item0 = 0;
    for (int i = 0; i < pp; ++i) {
        g += sns[i] > 0 ? 1 : 0;
        item0 += sns[i];
    }
    if (ns > 0) {
        int32_t* e = tab + few::TAB_HDR + few::TAB_ENT * g;
        e[0] = b;
        e[1] = pp;
        e[2] = np;
        e[3] = item0;
        e[4] = ns;
    }
    if (pp == LMI_FEW_MAX_PAIRS - 1) {
        tab[0] = g + (ns > 0 ? 1 : 0);
        tab[1] = item0 + ns;
    }
}

template <int KL>
__global__ __launch_bounds__(kThreads, 1) void scan_few_kernel(FewArgs a) {
    using namespace few;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int d_pad = a.d_pad;
    const int ldq = d_pad + QPAD;
    const uint32_t qs_bytes = 32u * (uint32_t)ldq * 2u;
    _Float16* Qs = reinterpret_cast<_Float16*>(smem);
    // (the item and its group wait in the last query row's pad: the widest
    // image and the rings fill the LDS, and the fragment reads stop at the
    // row's last k.  A short last segment's row fragments past nm are read
    // from the wave's own stage -- stale bytes of the ring -- and feed no MFMA)
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
        const int64_t row0 = a.bucket_off[c] + (int64_t)slice * a.few_rows;
        const int nrows =
            __builtin_amdgcn_readfirstlane((int)std::min<int64_t>(a.few_rows, a.bucket_off[c + 1] - row0));

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

        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.corpus + row0 * d_pad), (short)0, nrows * d_pad * 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t rn =
            __builtin_amdgcn_make_buffer_rsrc((void*)(a.inv_norm + row0), (short)0, nrows * 4, 0x00020000);
        const int nblk = (nrows + 31) / 32;
        const int nmy = nblk > wave ? (nblk - wave + kWaves - 1) / kWaves : 0;  // blocks wave, wave + 4, ..
        const int nst = nmy * nseg;

        // stage t = (the wave's block t / nseg, segment t % nseg) into slot t % 3
        auto issue = [&](int t) {
            const int bi = t / nseg, j = t - bi * nseg;
            const int b = wave + kWaves * bi;
            const int slot = t % NSLOT;
            const int cv = std::min(16, (d_pad - j * KSEG) / 8);  // the segment's chunks of a row
#pragma unroll
            for (int u = 0; u < STAGE / 1024; ++u) {
                const int rb = 4 * u + (lane >> 4);
                const int r = std::min(b * 32 + rb, nrows - 1);
                int cs = (lane & 15) ^ (rb & 15);
                cs = cs < cv ? cs : 0;
                const uint32_t vo = (uint32_t)r * (uint32_t)(d_pad * 2) + (uint32_t)(j * ROWB + cs * 16);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(ring + slot * STAGE + u * 1024), 16, vo, 0, 0,
                                                         0);
            }
            // (every stage brings its block's norms to its own slot: one DMA
            // count per stage, whatever the width)
            if (lane < 32) {
                const int r = std::min(b * 32 + lane, nrows - 1);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rn, (lds_t)(norms + slot * NORMB), 4, (uint32_t)r * 4u, 0, 0,
                                                         0);
            }
        };
        if (nst > 0) issue(0);
        if (nst > 1) issue(1);

        f32x16 acc;
        for (int t = 0; t < nst; ++t) {
            const int bi = t / nseg, j = t - bi * nseg;
            if (t + 2 < nst) {
                issue(t + 2);
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
            const uint32_t row_base = (uint32_t)(row0 + b * 32);
            const int valid_rows = nrows - b * 32;
            f32x4 n4[4];
            lds_read_norms(n4, norm_a + (uint32_t)(slot * NORMB));
            const float bound = key_dist_bound(thr);
            // (the filter first, as one mask a lane: the walk below then
            // branches on a register, not on sixteen live compare results)
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
                        const uint64_t key = make_key(dv[reg], row_base + (uint32_t)i);
                        if (ok && key < L[KL - 1]) list_insert<KL>(L, key);
                    }
                }
            }
            thr = std::min(thr, L[KL - 1]);
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

// One wave per grouped pair: lane l merges the pair's slice lists l, l + 64, ..
// into a register list, a butterfly of shuffles merges the lanes' lists (every
// lane ends with the union's KL smallest), and lanes 0 .. k - 1 write the
// entries.  Keys hold corpus rows, which ascend with the global position inside
// a bucket, so the order is the reference's (distance, position).
template <int KL>
__global__ __launch_bounds__(64) void few_merge_kernel(const uint64_t* __restrict__ partial, int32_t max_slices,
                                                       int32_t few_rows, const int32_t* __restrict__ pair_q,
                                                       const int32_t* __restrict__ pair_bucket,
                                                       const int64_t* __restrict__ bucket_off,
                                                       const int32_t* __restrict__ gpos, int64_t n_rows, int32_t k,
                                                       float* __restrict__ out_d, int32_t* __restrict__ out_pos,
                                                       int32_t* __restrict__ status) {
    const int pp = blockIdx.x, lane = threadIdx.x;
    const int c = pair_bucket[pp];
    if (c < 0) return;  // (a class out of range: the prefilled (+inf, -1) stay)
    const int nsl = (int)((bucket_off[c + 1] - bucket_off[c] + few_rows - 1) / few_rows);
    uint64_t L[KL];
    list_clear<KL>(L);
    for (int s = lane; s < nsl; s += 64) {
        const uint64_t* src = partial + ((size_t)pp * max_slices + s) * KL;
        uint64_t K[KL];
#pragma unroll
        for (int i = 0; i < KL; ++i) K[i] = src[i];
#pragma unroll
        for (int i = 0; i < KL; ++i)
            if (K[i] < L[KL - 1]) list_insert<KL>(L, K[i]);
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        uint64_t O[KL];
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)L[i], off);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(L[i] >> 32), off);
            O[i] = ((uint64_t)hi << 32) | lo;
        }
#pragma unroll
        for (int i = 0; i < KL; ++i)
            if (O[i] < L[KL - 1]) list_insert<KL>(L, O[i]);
    }
    uint64_t key = kEmptyKey;
#pragma unroll
    for (int i = 0; i < KL; ++i) key = i == lane ? L[i] : key;
    if (lane < k) {
        const uint32_t row = (uint32_t)key;
        bool empty = key == kEmptyKey;
        if (!empty && row >= (uint32_t)n_rows) {
            atomicOr(status, LMI_STATUS_INTERNAL);  // never for a sound scan
            empty = true;
        }
        const size_t o = (size_t)pair_q[pp] * k + lane;
        out_d[o] = empty ? __builtin_inff() : ord2f((uint32_t)(key >> 32));
        out_pos[o] = empty ? -1 : gpos[row];
    }
}

// ---- host ---------------------------------------------------------------------
// The call's layout: the scan's own plan (whose plan phase rounds the queries,
// fills the outputs and groups the pairs) and, behind it, this path's arrays.
struct FewPlan {
    ScanPlan base;
    int32_t kl, few_rows, max_slices;
    size_t tab, work, thr_g, partial, total;
};

// few_rows = 0: slices such that the call cuts into about six items per CU,
// taking the probed buckets for distinct and of the mean size; floor 256 rows,
// cap the largest bucket (and what a 32-bit DMA offset addresses).
int32_t few_rows_of(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t few_rows) {
    const int64_t bucket_cap = std::max<int64_t>(32, (int64_t)std::max(idx->max_chunks, 1) * idx->chunk_rows);
    const int64_t dma_cap = ((int64_t)1 << 30) / (idx->d_pad * 2) / 32 * 32;
    const int64_t cap = std::min(bucket_cap, dma_cap);
    if (few_rows > 0) return (int32_t)std::min<int64_t>(few_rows, cap);
    const int64_t P = (int64_t)nq * R, C = idx->n_buckets;
    const int64_t rows = std::min(P, C) * ((idx->n_rows + C - 1) / C);
    const int64_t per = rows / (6 * (int64_t)num_cus());
    return (int32_t)std::min<int64_t>(std::max<int64_t>(256, (per + 31) / 32 * 32), cap);
}

int few_gate(const char* fn, const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k, int32_t few_rows) {
    LMI_CHECK_ARG(idx != nullptr, "%s: null index", fn);
    LMI_CHECK_ARG(nq >= 0 && R >= 1, "%s: bad nq/R (%d, %d)", fn, nq, R);
    LMI_CHECK_ARG(few_rows >= 0 && few_rows % 32 == 0,
                  "%s: few_rows=%d is not a positive multiple of 32 (0: the call chooses)", fn, few_rows);
    LMI_CHECK_ARG(k >= 1, "%s: k=%d < 1", fn, k);
    LMI_CHECK_ARG(idx->d >= 1 && idx->d_pad >= idx->d && idx->d_pad % 32 == 0, "%s: bad d/d_pad", fn);
    LMI_CHECK_ARG(idx->n_buckets >= 1, "%s: n_buckets < 1", fn);
    LMI_CHECK_ARG(idx->chunk_rows >= 32 && idx->chunk_rows % 32 == 0, "%s: chunk_rows must be a multiple of 32", fn);
    LMI_CHECK_ARG(join_wgs() == 0, "%s: the few-query scan takes no join workgroups (lmi_scan_set_join_workgroups)",
                  fn);
    auto unsupported = [&](bool bad, const char* what) {
        if (bad) set_error("%s: the few-query scan takes %s", fn, what);
        return bad;
    };
    if (unsupported((int64_t)nq * R > LMI_FEW_MAX_PAIRS, "at most LMI_FEW_MAX_PAIRS = 256 pairs (nq * R)") ||
        unsupported(k > LMI_MAX_K, "k <= 16") ||
        unsupported(idx->dtype != LMI_F16, "the fp16 storage alone (LMI_F16)") ||
        unsupported(idx->d_pad > kFewMaxDPad, "d_pad <= 992") ||
        unsupported(idx->corpus32 || idx->corpus64, "no split mode and no float64 rows (corpus32 / corpus64)") ||
        unsupported(idx->chunk_centroid != nullptr, "no sub-cluster layout (chunk_centroid)"))
        return LMI_E_UNSUPPORTED;
    return LMI_OK;
}

FewPlan few_plan(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k, int32_t few_rows) {
    FewPlan f{};
    f.base = scan_plan(idx, nq, R, k, LMI_Q_F16);
    f.kl = k <= 10 ? 10 : 16;
    f.few_rows = few_rows_of(idx, nq, R, few_rows);
    const int64_t bucket_cap = (int64_t)std::max(idx->max_chunks, 1) * idx->chunk_rows;
    f.max_slices = (int32_t)((bucket_cap + f.few_rows - 1) / f.few_rows);
    const size_t P = (size_t)nq * R;
    size_t off = f.base.total;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 256);
        return at;
    };
    f.tab = take((few::TAB_HDR + few::TAB_ENT * LMI_FEW_MAX_PAIRS) * 4);
    f.work = take(4);
    f.thr_g = take(P * 8);
    f.partial = take(P * (size_t)f.max_slices * f.kl * 8);
    f.total = off;
    return f;
}

template <int KL>
int launch_scan_few(const FewArgs& a, hipStream_t s) {
    const size_t lds = few_lds_bytes(a.d_pad);
    return launch_dyn_lds<scan_few_kernel<KL>>("scan_few_kernel", dim3(num_cus()), dim3(kThreads), lds, s, a);
}

}  // namespace

int launch_few_merge(int kl, const uint64_t* partial, int32_t max_slices, int32_t few_rows, const int32_t* pair_q,
                     const int32_t* pair_bucket, const int64_t* off, const int32_t* gpos, int64_t n_rows, int32_t P,
                     int32_t k, float* out_d, int32_t* out_pos, int32_t* status, hipStream_t s) {
#define LMI_FM(KLV)                                                                                             \
    hipLaunchKernelGGL((few_merge_kernel<KLV>), dim3(P), dim3(64), 0, s, partial, max_slices, few_rows, pair_q, \
                       pair_bucket, off, gpos, n_rows, k, out_d, out_pos, status)
    if (kl == 10) LMI_FM(10); else LMI_FM(16);
#undef LMI_FM
    LMI_LAUNCH_CHECK("few_merge_kernel");
    return LMI_OK;
}

static_assert(32 * (kFewMaxDPad + few::QPAD) * 2 + kWaves * few::NSLOT * (few::STAGE + few::NORMB) <= 160 * 1024,
              "LDS budget");

}  // namespace lmi

extern "C" size_t lmi_scan_few_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t k,
                                               int32_t few_rows) {
    using namespace lmi;
    if (few_gate("lmi_scan_few_workspace_bytes", idx, nq, R, k, few_rows) != LMI_OK) return 0;
    return few_plan(idx, nq, R, k, few_rows).total;
}

extern "C" int lmi_bucket_topk_few(const lmi_index_desc* idx, const float* q, int32_t nq, int32_t ldq,
                                   const int32_t* classes, int32_t R, int32_t k, int32_t few_rows, void* workspace,
                                   size_t ws_bytes, float* out_d, int32_t* out_pos, int32_t* status, void* stream) {
    using namespace lmi;
    // (every refusal comes before any launch and needs no device)
    LMI_TRY(few_gate("lmi_bucket_topk_few", idx, nq, R, k, few_rows));
    LMI_CHECK_ARG(idx->n_rows >= 0 && idx->n_rows < (int64_t)UINT32_MAX, "lmi_bucket_topk_few: n_rows out of range");
    LMI_CHECK_ARG(ldq >= idx->d, "lmi_bucket_topk_few: ldq < d");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(q && classes && out_d && out_pos && status && workspace, "lmi_bucket_topk_few: null pointer");
    const FewPlan f = few_plan(idx, nq, R, k, few_rows);
    if (ws_bytes < f.total) {
        set_error("lmi_bucket_topk_few: workspace %zu B < required %zu B", ws_bytes, f.total);
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
    if (idx->n_rows == 0) return LMI_OK;

    auto* ws = reinterpret_cast<unsigned char*>(workspace);
    const int P = nq * R;
    const int32_t* pair_q = (const int32_t*)(ws + f.base.pair_q);
    const int32_t* pair_bucket = (const int32_t*)(ws + f.base.pair_bucket);
    hipLaunchKernelGGL(few_plan_kernel, dim3(1), dim3(LMI_FEW_MAX_PAIRS), 0, s, pair_bucket,
                       (const int32_t*)(ws + f.base.counts), idx->bucket_off, P, f.few_rows, (int32_t*)(ws + f.tab),
                       (int32_t*)(ws + f.work), (unsigned long long*)(ws + f.thr_g));
    LMI_LAUNCH_CHECK("few_plan_kernel");

    FewArgs a{};
    a.corpus = reinterpret_cast<const _Float16*>(idx->corpus);
    a.inv_norm = idx->inv_norm;
    a.bucket_off = idx->bucket_off;
    a.d_pad = idx->d_pad;
    a.few_rows = f.few_rows;
    a.max_slices = f.max_slices;
    a.R = R;
    a.qbuf = reinterpret_cast<const _Float16*>(ws + f.base.qbuf);
    a.invq = (const float*)(ws + f.base.invq);
    a.pair_q = pair_q;
    a.tab = (const int32_t*)(ws + f.tab);
    a.work = (int32_t*)(ws + f.work);
    a.thr_g = (unsigned long long*)(ws + f.thr_g);
    a.partial = (uint64_t*)(ws + f.partial);
    LMI_TRY(f.kl == 10 ? launch_scan_few<10>(a, s) : launch_scan_few<16>(a, s));

    return launch_few_merge(f.kl, a.partial, f.max_slices, f.few_rows, pair_q, pair_bucket, idx->bucket_off, idx->gpos,
                            idx->n_rows, P, k, out_d, out_pos, status, s);
}
