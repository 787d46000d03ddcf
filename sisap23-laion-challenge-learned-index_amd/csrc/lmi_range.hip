// K11 — range search: every row of the probed buckets within a per-query
// radius (gfx950).
//
//   lmi_bucket_range   the collect scan: per (query, probe) pair every row with
//                      d <= bound[q] as a key make_key(d, row) in the pair's
//                      candidate buffer, and the pair's exact hit count
//                        - fp16 corpus, fp16-exact queries, d_pad 768, no tags:
//                          the 8-wave ring's collect scan (scan3_kernel MODE 2,
//                          as the wide path runs it), whose grouped-pair
//                          outputs range_ungroup_kernel re-indexes by pair id
//                        - everything else: range_scan_kernel below, the
//                          collect form of the general kernel
//   lmi_range_pack     the pairs' candidates -> one segment per query of
//                      (distance, global position, query) entries, unsorted
//                      (the caller sorts; with float64 distances from
//                      lmi_range_rescore_f64, lmi_refine.hip, only d64 <= r)
// The distance of a hit is the list scans' own: the value a top-k list of the
// same kernel family holds for that (query, row).
#include "lmi_scan_internal.hpp"

#include <algorithm>
#include <mutex>
#include <type_traits>

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// the general kernel's collect form
// ---------------------------------------------------------------------------
// scan_kernel's tile (lmi_scan_v12.hip): the tile's queries staged in LDS, each
// wave streams 32-row blocks straight into MFMA A fragments.  The staging and
// the MFMA loop are that kernel's, statement for statement, so a (query, row)
// gets the same accumulator and, through the same fmaf, the same distance bits;
// they are repeated here and not shared so that scan_kernel's code object stays
// what it is.  The epilogue differs: no lists, no running bound.  A lane's 16
// accumulator registers are tested against the query's fixed bound; the two
// lanes of a query column (col, col + 32) add their hit counts (a
// v_permlane32_swap), lane col reserves the slots of both with one atomic on
// the pair's counter, and each lane writes its keys (plain vector stores).
template <bool F16MATH>
struct RangeCfg {
    static constexpr int QB = F16MATH ? 64 : 32;
    static constexpr int NQF = QB / 32;
    static constexpr int QPAD = F16MATH ? 8 : 4;
    using QT = typename std::conditional<F16MATH, _Float16, float>::type;
};

// (per query slot: 1/|q|, the bound, the pair id, the tag value word; 16 bytes
// for the tile counter; then the slots' tag mask words)
template <bool F16MATH>
size_t range_lds_bytes(int d_pad) {
    using Cfg = RangeCfg<F16MATH>;
    return (size_t)Cfg::QB * (d_pad + Cfg::QPAD) * sizeof(typename Cfg::QT) + (size_t)Cfg::QB * 16 + 16 +
           (size_t)Cfg::QB * 4;
}

template <bool F16MATH, typename TC, bool TAG>
__global__ __launch_bounds__(kThreads, 1) void range_scan_kernel(RangeArgs ra) {
    using Cfg = RangeCfg<F16MATH>;
    using QT = typename Cfg::QT;
    constexpr int QB = Cfg::QB, NQF = Cfg::NQF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ScanArgs& a = ra.s;

    const int d_pad = a.d_pad;
    const int ldq = d_pad + Cfg::QPAD;
    QT* Qs = reinterpret_cast<QT*>(smem);
    float* invq_s = reinterpret_cast<float*>(smem + (size_t)QB * ldq * sizeof(QT));
    float* bound_s = invq_s + QB;
    int32_t* pid_s = reinterpret_cast<int32_t*>(bound_s + QB);
    uint32_t* want_s = reinterpret_cast<uint32_t*>(pid_s + QB);
    int& s_tile = *reinterpret_cast<int*>(want_s + QB);
    uint32_t* mask_s = want_s + QB + 4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int h = lane >> 5;
    const int col = lane & 31;

    const TC* __restrict__ corpus = reinterpret_cast<const TC*>(a.corpus);
    const QT* __restrict__ qbuf = reinterpret_cast<const QT*>(a.qbuf);
    const int ntiles = a.meta[2 * kGroups];
    const uint32_t cap = (uint32_t)ra.cap;

    for (;;) {
        if (tid == 0) s_tile = atomicAdd(&a.work[kGroups], 1);
        __syncthreads();
        const int t = s_tile;
        if (t >= ntiles) break;
        const Tile tile = a.tiles[t];
        const int64_t bstart = a.bucket_off[tile.c];
        const int64_t bend = a.bucket_off[tile.c + 1];
        const int64_t row0 = bstart + (int64_t)tile.chunk * a.chunk_rows;
        const int nrows = (int)std::min<int64_t>(a.chunk_rows, bend - row0);

        // ---- stage the tile's queries (16 B per lane per step) ----------
        {
            constexpr int EPV = 16 / sizeof(QT);
            const int vpr = d_pad / EPV;
            for (int e = tid; e < QB * vpr; e += kThreads) {
                const int r = e / vpr, v = e - r * vpr;
                uint4 val = make_uint4(0, 0, 0, 0);
                if (r < tile.np) {
                    const int q = a.pair_q[tile.pp0 + r] / a.R;
                    val = *reinterpret_cast<const uint4*>(qbuf + (size_t)q * d_pad + v * EPV);
                }
                *reinterpret_cast<uint4*>(Qs + r * ldq + v * EPV) = val;
            }
            for (int r = tid; r < QB; r += kThreads) {
                const bool live = r < tile.np;
                const int pid = live ? a.pair_q[tile.pp0 + r] : 0;
                const int q = pid / a.R;
                invq_s[r] = live ? a.invq[q] : 0.0f;
                bound_s[r] = live ? ra.bound[q] : -__builtin_inff();  // dead slots take nothing
                pid_s[r] = pid;
                // (TAG: a.want holds (1/|q|, value, mask) triples)
                want_s[r] = (TAG && live) ? a.want[3 * (size_t)q + 1] : 0u;
                if (TAG) mask_s[r] = live ? a.want[3 * (size_t)q + 2] : 0u;
            }
        }
        __syncthreads();

        const int nsub = (nrows + 31) / 32;
        for (int st = wave; st < nsub; st += kWaves) {
            const int sub0 = st * 32;
            const int myrow = std::min(sub0 + col, nrows - 1);
            const TC* yrow = corpus + (size_t)(row0 + myrow) * d_pad;
            f32x16 acc[NQF];
#pragma unroll
            for (int f = 0; f < NQF; ++f)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[f][i] = 0.0f;

            if constexpr (F16MATH) {
                // 64-wide k block: lane half h covers k = kb + 32h + [0, 32);
                // MFMA step s (0..3), element j  <->  k = kb + 32h + 8s + j
                static_assert(sizeof(TC) == 2, "fp16 math needs an fp16 corpus");
                const half8* ysrc = reinterpret_cast<const half8*>(yrow) + 4 * h;
                half8 acur[4], anext[4];
                const int nkb = d_pad / 64;
                // (d_pad == 32 has no full block: lane half 1's first 64 B
                // would lie past its row, past the corpus for the last row)
                if (nkb > 0) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) acur[s] = ysrc[s];
                }
                for (int kb = 0; kb < nkb; ++kb) {
                    if (kb + 1 < nkb) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) anext[s] = ysrc[(kb + 1) * 8 + s];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
#pragma unroll
                        for (int f = 0; f < NQF; ++f) {
                            const half8 b = *reinterpret_cast<const half8*>(
                                Qs + (32 * f + col) * ldq + kb * 64 + 32 * h + 8 * s);
                            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(acur[s], b, acc[f], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) acur[s] = anext[s];
                }
                // d_pad is a multiple of 32: a trailing 32-wide half block
                if (d_pad % 64) {
                    const int kb = nkb;
                    const half8* ys2 = reinterpret_cast<const half8*>(yrow + kb * 64) + 2 * h;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const half8 av = ys2[s];
#pragma unroll
                        for (int f = 0; f < NQF; ++f) {
                            const half8 b = *reinterpret_cast<const half8*>(
                                Qs + (32 * f + col) * ldq + kb * 64 + 16 * h + 8 * s);
                            acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b, acc[f], 0, 0, 0);
                        }
                    }
                }
            } else {
                // fp32 math, 32-wide k block: lane half h covers kb + 16h + [0,16);
                // group s (0..3) of 4 MFMAs 32x32x2, element j <-> k = kb + 16h + 4s + j
                const int nkb = d_pad / 32;
                for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        f32x4 av;
                        if constexpr (sizeof(TC) == 2) {
                            const half4 hv = *reinterpret_cast<const half4*>(yrow + kb * 32 + 16 * h + 4 * s);
#pragma unroll
                            for (int j = 0; j < 4; ++j) av[j] = (float)hv[j];
                        } else {
                            av = *reinterpret_cast<const f32x4*>(yrow + kb * 32 + 16 * h + 4 * s);
                        }
#pragma unroll
                        for (int f = 0; f < NQF; ++f) {
                            const f32x4 b = *reinterpret_cast<const f32x4*>(
                                Qs + (32 * f + col) * ldq + kb * 32 + 16 * h + 4 * s);
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[j], acc[f], 0, 0, 0);
                        }
                    }
                }
            }

            // ---- collect: lane holds query column col and rows
            // (reg&3) + 8*(reg>>2) + 4*h of the block, reg = 0..15 -----------
            const uint32_t row_base = (uint32_t)(row0 + sub0);
            const int valid_rows = nrows - sub0;
#pragma unroll
            for (int f = 0; f < NQF; ++f) {
                const int qslot = 32 * f + col;
                const float invq = invq_s[qslot], bound = bound_s[qslot];
                const uint32_t want = want_s[qslot], tmask = TAG ? mask_s[qslot] : 0u;
                float dv[16];
                uint32_t mask = 0;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const bool valid = i < valid_rows;
                    const float inv = valid ? a.inv_norm[row_base + i] : 0.0f;
                    dv[reg] = fmaf(-acc[f][reg], invq * inv, 1.0f);
                    const bool tag_ok = !TAG || (valid && (a.tags[row_base + i] & tmask) == want);
                    mask |= (valid && dv[reg] <= bound && tag_ok) ? (1u << reg) : 0u;
                }
                if (!__any(mask != 0)) continue;
                // one atomic per query column: lane col reserves its own and
                // lane col + 32's slots; the count runs on past cap
                const uint32_t mine = (uint32_t)__builtin_popcount(mask);
                const uint32_t theirs = partner_u32(mine, h);
                uint32_t base = 0;
                if (h == 0 && mine + theirs != 0)
                    base = atomicAdd(&ra.ccount[pid_s[qslot]], mine + theirs);
                const uint32_t pbase = partner_u32(base, h);
                uint32_t at = h ? pbase + theirs : base;
                uint64_t* dst = ra.cand + (size_t)pid_s[qslot] * cap;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    if (mask & (1u << reg)) {
                        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        if (at < cap) dst[at] = make_key(dv[reg], row_base + (uint32_t)i);
                        ++at;
                    }
                }
            }
        }
        __syncthreads();  // every wave done with Qs and the slot arrays
    }
}

template <bool F16MATH, typename TC, bool TAG>
int launch_range(const RangeArgs& a, hipStream_t s) {
    const size_t lds = range_lds_bytes<F16MATH>(a.s.d_pad);
    if (lds > 160 * 1024) {
        set_error("lmi_bucket_range: d_pad=%d needs %zu B of LDS per workgroup", a.s.d_pad, lds);
        return LMI_E_UNSUPPORTED;
    }
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)range_scan_kernel<F16MATH, TC, TAG>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    LMI_HIP_TRY(attr_err);
    const bool timed = timing().on;
    std::pair<hipEvent_t, hipEvent_t> ev{};
    if (timed) LMI_TRY(timing_record(s, true, ev));
    hipLaunchKernelGGL((range_scan_kernel<F16MATH, TC, TAG>), dim3(num_cus()), dim3(kThreads), lds, s, a);
    LMI_LAUNCH_CHECK("range_scan_kernel");
    if (timed) return timing_record(s, false, ev);
    return LMI_OK;
}

// ---------------------------------------------------------------------------
// the 8-wave ring's collect scan, re-indexed
// ---------------------------------------------------------------------------
// bound_ord[pair id] of the collect scan (WideScan mode 2): the ordinal of the
// query's bound.  MODE 2 tests d <= ord2f(bound_ord), inclusive as the range
// search is, so the ordinal goes in as it is.  (Ordinal 0, "takes nothing", is
// the image of a NaN with every bit set alone; a -inf bound has ordinal
// 0x007fffff and rejects every finite distance through the comparison.)
__global__ __launch_bounds__(256) void range_bound_kernel(const float* __restrict__ bound, int64_t P, int32_t R,
                                                          uint32_t* __restrict__ bound_ord) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < P) bound_ord[p] = f2ord(bound[p / R]);
}

// one wave per grouped pair: its count and the stored keys to its pair id
__global__ __launch_bounds__(256) void range_ungroup_kernel(const int32_t* __restrict__ pair_q,
                                                            const int32_t* __restrict__ pair_bucket, int64_t P,
                                                            const uint64_t* __restrict__ cand_g,
                                                            const uint32_t* __restrict__ ccount_g, int32_t cap,
                                                            uint64_t* __restrict__ cand, uint32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t pp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pp >= P || pair_bucket[pp] < 0) return;  // (-1: never filled, the pair has no bucket)
    const int64_t p = pair_q[pp];
    if (p < 0 || p >= P) return;
    const uint32_t n = ccount_g[pp];
    if (lane == 0) count[p] = n;
    const uint32_t m = std::min(n, (uint32_t)cap);
    for (uint32_t i = lane; i < m; i += 64) cand[(size_t)p * cap + i] = cand_g[(size_t)pp * cap + i];
}

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------
// One wave per pair: the pair's stored candidates to off[pair] .. of the
// outputs as (distance, global position, query).  A pair whose count exceeds
// cap is skipped (the second scan's call writes it).  With d64 / radius64 (the
// float64 re-score) only candidates with d64 <= radius64[q] are written, d64
// as the distance; off is then the prefix of the kept counts.  The order inside
// a pair is the scan's arrival order: the caller sorts.
__global__ __launch_bounds__(256) void range_pack_kernel(const uint64_t* __restrict__ cand,
                                                         const uint32_t* __restrict__ count, int32_t cap,
                                                         int64_t P, int32_t R, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ gpos,
                                                         const double* __restrict__ d64,
                                                         const double* __restrict__ radius64,
                                                         double* __restrict__ out_d, int32_t* __restrict__ out_pos,
                                                         int32_t* __restrict__ out_q) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const uint32_t n = count[p];
    if (n == 0 || n > (uint32_t)cap) return;
    const int32_t q = (int32_t)(p / R);
    const double r = d64 ? radius64[q] : 0.0;
    int64_t o = off[p];
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        bool keep = i < n;
        uint64_t key = 0;
        double d = 0.0;
        if (keep) {
            key = cand[(size_t)p * cap + i];
            if (d64) {
                d = d64[(size_t)p * cap + i];
                keep = d <= r;
            } else {
                d = (double)ord2f((uint32_t)(key >> 32));
            }
        }
        const uint64_t m = __ballot(keep);
        if (keep) {
            const int64_t at = o + __popcll(m & ((1ull << lane) - 1ull));
            out_d[at] = d;
            out_pos[at] = gpos[(uint32_t)key];
            out_q[at] = q;
        }
        o += __popcll(m);
    }
}

// what lmi_bucket_range takes (every refusal before any launch, no device needed)
int range_check(const lmi_index_desc* idx, bool tags, bool want, int32_t nq, int32_t R, int32_t qmode,
                int32_t pair_cap) {
    LMI_CHECK_ARG(idx != nullptr, "lmi_bucket_range: null index");
    LMI_TRY(i8_refuse("lmi_bucket_range", idx));
    LMI_CHECK_ARG(tags == want, "lmi_bucket_range: tags and want come together");
    LMI_CHECK_ARG(!idx->corpus32 && !idx->corpus64,
                  "lmi_bucket_range: the split mode (corpus32 / corpus64) takes no range search");
    LMI_CHECK_ARG(!idx->chunk_centroid, "lmi_bucket_range: sub-cluster layouts (chunk_centroid) take no range search");
    LMI_CHECK_ARG(idx->dtype == LMI_F16 || idx->dtype == LMI_F32, "lmi_bucket_range: bad corpus dtype");
    LMI_CHECK_ARG(idx->d >= 1 && idx->d_pad >= idx->d && idx->d_pad % 32 == 0, "lmi_bucket_range: bad d/d_pad");
    LMI_CHECK_ARG(idx->n_buckets >= 1, "lmi_bucket_range: n_buckets < 1");
    LMI_CHECK_ARG(idx->chunk_rows >= 32 && idx->chunk_rows % 32 == 0,
                  "lmi_bucket_range: chunk_rows must be a multiple of 32");
    LMI_CHECK_ARG(idx->n_rows >= 0 && idx->n_rows < (int64_t)UINT32_MAX, "lmi_bucket_range: n_rows out of range");
    LMI_CHECK_ARG(qmode == LMI_Q_F16 || qmode == LMI_Q_F32,
                  "lmi_bucket_range: qmode 0x%x: LMI_Q_F16 or LMI_Q_F32 alone (no phase, join or seed flag)", qmode);
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < INT32_MAX, "lmi_bucket_range: bad nq/R");
    LMI_CHECK_ARG(pair_cap >= 1 && pair_cap <= (1 << 24), "lmi_bucket_range: pair_cap=%d outside [1, 2^24]", pair_cap);
    return LMI_OK;
}

// the workspace: the scan's plan region, and on the 8-wave ring the collect
// scan's grouped outputs behind it
struct RangeWs {
    ScanPlan plan;
    bool ring;
    size_t bound_ord, ccount_g, cand_g, total;
};
RangeWs range_ws(const lmi_index_desc* idx, int nq, int R, int qmode, bool tagged, int pair_cap) {
    RangeWs w{};
    w.plan = scan_plan(idx, nq, R, 10, qmode);
    w.ring = !tagged && w.plan.family == ScanKernel::Ring8;
    // (16-entry lists of the tagged plan: the general family for every shape)
    if (!w.ring) w.plan = scan_plan(idx, nq, R, 16, qmode, false, true);
    size_t off = align_up(w.plan.total, 256);
    if (w.ring) {
        const size_t P = (size_t)nq * R;
        w.bound_ord = off;
        off = align_up(off + P * 4, 256);
        w.ccount_g = off;
        off = align_up(off + P * 4, 256);
        w.cand_g = off;
        off = align_up(off + P * (size_t)pair_cap * 8, 256);
    }
    w.total = std::max<size_t>(off, 256);
    return w;
}
// range_scan_kernel stages its tile's queries whole: past this width the tile
// does not fit the LDS of a workgroup (d_pad > 1248 in either arithmetic)
bool range_too_wide(const RangeWs& w, const lmi_index_desc* idx) {
    if (w.ring) return false;
    return (w.plan.f16math ? range_lds_bytes<true>(idx->d_pad) : range_lds_bytes<false>(idx->d_pad)) > 160 * 1024;
}

}  // namespace

int launch_range_scan(const RangeArgs& a, bool f16math, bool corpus_f16, hipStream_t s) {
    const bool tag = a.s.tags != nullptr;
    if (f16math) return tag ? launch_range<true, _Float16, true>(a, s) : launch_range<true, _Float16, false>(a, s);
    if (corpus_f16) return tag ? launch_range<false, _Float16, true>(a, s) : launch_range<false, _Float16, false>(a, s);
    return tag ? launch_range<false, float, true>(a, s) : launch_range<false, float, false>(a, s);
}

}  // namespace lmi

extern "C" size_t lmi_range_workspace_bytes(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t qmode,
                                            int32_t tagged, int32_t pair_cap) {
    using namespace lmi;
    if (range_check(idx, tagged != 0, tagged != 0, nq, R, qmode, pair_cap) != LMI_OK) return 0;
    const RangeWs w = range_ws(idx, nq, R, qmode, tagged != 0, pair_cap);
    return range_too_wide(w, idx) ? 0 : w.total;
}

extern "C" int lmi_bucket_range(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* want,
                                const float* q, int32_t nq, int32_t ldq, const int32_t* classes, int32_t R,
                                int32_t qmode, const float* bound, int32_t pair_cap, uint64_t* cand,
                                uint32_t* count, int32_t* status, void* workspace, size_t ws_bytes,
                                void* stream) {
    return lmi_bucket_range_masked(idx, tags, want, want, nullptr, nullptr, q, nq, ldq, classes, R, qmode, bound,
                                   pair_cap, cand, count, status, workspace, ws_bytes, stream);
}

extern "C" int lmi_bucket_range_masked(const lmi_index_desc* idx, const uint32_t* tags, const uint32_t* want,
                                       const uint32_t* mask, const uint32_t* host_value,
                                       const uint32_t* host_mask, const float* q, int32_t nq, int32_t ldq,
                                       const int32_t* classes, int32_t R, int32_t qmode, const float* bound,
                                       int32_t pair_cap, uint64_t* cand, uint32_t* count, int32_t* status,
                                       void* workspace, size_t ws_bytes, void* stream) {
    using namespace lmi;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    LMI_TRY(range_check(idx, tags != nullptr, want != nullptr, nq, R, qmode, pair_cap));
    LMI_CHECK_ARG((want != nullptr) == (mask != nullptr), "lmi_bucket_range: value and mask come together");
    LMI_TRY(masked_words_check("lmi_bucket_range_masked", host_value, host_mask, nq));
    LMI_CHECK_ARG(ldq >= idx->d, "lmi_bucket_range: ldq < d");
    LMI_CHECK_ARG(join_wgs() == 0, "lmi_bucket_range: the range scan runs in one launch (join workgroups are set)");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(q && classes && bound && cand && count && status && workspace, "lmi_bucket_range: null pointer");
    LMI_CHECK_ARG(idx->n_rows == 0 || (idx->corpus && idx->inv_norm && idx->gpos),
                  "lmi_bucket_range: null corpus arrays");
    LMI_CHECK_ARG(idx->bucket_off && idx->chunk_first, "lmi_bucket_range: null bucket tables");
    const RangeWs w = range_ws(idx, nq, R, qmode, tags != nullptr, pair_cap);
    if (range_too_wide(w, idx)) {
        set_error("lmi_bucket_range: d_pad=%d exceeds the LDS budget of the scan's query tile", idx->d_pad);
        return LMI_E_UNSUPPORTED;
    }
    if (ws_bytes < w.total) {
        set_error("lmi_bucket_range: workspace %zu B < required %zu B", ws_bytes, w.total);
        return LMI_E_WORKSPACE;
    }
    auto* ws = reinterpret_cast<unsigned char*>(workspace);
    const int64_t P = (int64_t)nq * R;
    // (no lists are written: the list outputs are placeholders inside the
    // plan's region, which prep -- prefill off -- never touches)
    ScanCall c{.idx = idx, .q = q, .nq = nq, .ldq = ldq, .classes = classes, .R = R, .k = w.ring ? 10 : 16,
               .qmode = qmode, .out_d = reinterpret_cast<float*>(ws), .out_pos = reinterpret_cast<int32_t*>(ws),
               .status = status, .workspace = workspace, .ws_bytes = ws_bytes, .stream = s};
    c.prefill = false;
    c.phases = kPhasePlan | kPhaseScan;
    c.plan = &w.plan;
    if (!w.ring) {
        const RangeScan rs{bound, cand, count, pair_cap};
        c.tags = tags;
        c.want = want;
        c.mask = mask;
        c.range = &rs;
        return bucket_topk_impl(c);
    }
    uint32_t* bound_ord = reinterpret_cast<uint32_t*>(ws + w.bound_ord);
    uint32_t* ccount_g = reinterpret_cast<uint32_t*>(ws + w.ccount_g);
    uint64_t* cand_g = reinterpret_cast<uint64_t*>(ws + w.cand_g);
    hipLaunchKernelGGL(range_bound_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, bound, P, R, bound_ord);
    LMI_LAUNCH_CHECK("range_bound_kernel");
    LMI_TRY(fill_u32(count, 0u, (size_t)P, s));  // (pairs without a bucket: never grouped)
    const WideScan m2{2, bound_ord, cand_g, ccount_g, pair_cap, nullptr, 0, nullptr, nullptr};
    c.wide = &m2;
    LMI_TRY(bucket_topk_impl(c));
    if (idx->n_rows == 0) return LMI_OK;
    hipLaunchKernelGGL(range_ungroup_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s,
                       (const int32_t*)(ws + w.plan.pair_q), (const int32_t*)(ws + w.plan.pair_bucket), P, cand_g,
                       ccount_g, pair_cap, cand, count);
    LMI_LAUNCH_CHECK("range_ungroup_kernel");
    return LMI_OK;
}

extern "C" int lmi_range_pack(const lmi_index_desc* idx, int32_t nq, int32_t R, int32_t pair_cap,
                              const uint64_t* cand, const uint32_t* count, const int64_t* off,
                              const double* d64, const double* radius64, double* out_d, int32_t* out_pos,
                              int32_t* out_q, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(idx != nullptr, "lmi_range_pack: null index");
    LMI_TRY(i8_refuse("lmi_range_pack", idx));
    LMI_CHECK_ARG(nq >= 0 && R >= 1 && (int64_t)nq * R < INT32_MAX, "lmi_range_pack: bad nq/R");
    LMI_CHECK_ARG(pair_cap >= 1, "lmi_range_pack: pair_cap=%d < 1", pair_cap);
    LMI_CHECK_ARG((d64 != nullptr) == (radius64 != nullptr), "lmi_range_pack: d64 and radius64 come together");
    if (nq == 0) return LMI_OK;
    LMI_CHECK_ARG(cand && count && off && out_d && out_pos && out_q && idx->gpos, "lmi_range_pack: null pointer");
    const int64_t P = (int64_t)nq * R;
    hipLaunchKernelGGL(range_pack_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), cand, count, pair_cap, P, R, off, idx->gpos, d64,
                       radius64, out_d, out_pos, out_q);
    LMI_LAUNCH_CHECK("range_pack_kernel");
    return LMI_OK;
}
