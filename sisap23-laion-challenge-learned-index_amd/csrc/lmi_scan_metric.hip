// The metric scans (include/lmi_hip.h, lmi_bucket_topk_metric): the 8-wave
// ring and the general kernel with the distance of LMI_METRIC_L2 or
// LMI_METRIC_IP in place of the cosine, and the query prep that writes the
// words they read.
//   scan3_kernel MODE 5 / 6 (lmi_scan3.hpp)  d_pad == 768, fp16 rows, fp16-exact
//                queries, k <= 10: the ring's plain 10-entry lists, instantiated
//                here (the 15-entry form spilled a query fragment into the
//                MFMA stream under l2, which tests/test_codeobj.py refuses)
//   scan_kernel_metric  every other d_pad <= 992: scan_kernel's tile queue,
//                query staging and MFMA loops (lmi_scan_v12.hip) with the
//                metric's epilogue; plain lists alone, so none of its lower
//                bounds or tag words
// This unit holds the metric instantiations alone, so the cosine units compile
// exactly as they did.  New to this project: the reference scores by cosine
// alone (utils.py:10-11).
#include "lmi_scan3.hpp"
#include "lmi_quant.hpp"

#include <algorithm>
#include <type_traits>

namespace lmi {
namespace {

// ---------------------------------------------------------------------------
// the general kernel by another metric
// ---------------------------------------------------------------------------
// (scan_kernel's tile shape: lmi_scan_v12.hip)
template <int KL, bool F16MATH>
struct ScanCfg {
    static constexpr int QB = F16MATH ? 64 : 32;  // queries per tile
    static constexpr int NQF = QB / 32;            // 32-query MFMA fragments per wave
    static constexpr int QPAD = F16MATH ? 8 : 4;   // LDS row pad (elements): 16 B
    using QT = typename std::conditional<F16MATH, _Float16, float>::type;
};

template <int KL, bool F16MATH>
size_t scan_lds_bytes(int d_pad) {
    using Cfg = ScanCfg<KL, F16MATH>;
    const size_t qs = (size_t)Cfg::QB * (d_pad + Cfg::QPAD) * sizeof(typename Cfg::QT);
    const size_t merge = (size_t)Cfg::QB * 2 * kWaves * KL * sizeof(uint64_t);
    const size_t queue = (size_t)kWaves * kQCap * 64 * sizeof(uint64_t);
    return std::max(qs, merge) + queue + Cfg::QB * (sizeof(uint64_t) + sizeof(float)) + 16;
}

// The epilogue of one 32x32 accumulator tile (lane: query column lane & 31,
// rows (reg&3) + 8*(reg>>2) + 4*(lane>>5)): tile_epilogue's filter, queue and
// insertion with d = metric_dist -- l2: inv_norm holds |y|^2 and wq the
// query's |q|^2; ip: neither word is read.  Distances may be negative: the
// keys' image of a float (f2ord) orders them, and a dead slot's bound (thr =
// 0) is -inf.
template <int KL, int METRIC>
__device__ inline void metric_epilogue(const f32x16& acc, uint64_t (&L)[KL], uint64_t* thr_slot, float wq,
                                       const float* __restrict__ inv_norm, uint32_t row_base, int valid_rows,
                                       uint64_t* queue, int lane) {
    const int h = lane >> 5;
    const uint64_t thr = *thr_slot;
    const float bound = key_dist_bound(thr);
    int cnt = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const bool valid = i < valid_rows;
        const float wy = (METRIC != LMI_METRIC_IP && valid) ? inv_norm[row_base + i] : 0.0f;
        const float d = metric_dist<METRIC>(acc[reg], wq, wy);
        if (valid && d <= bound) {
            const uint64_t key = make_key(d, row_base + (uint32_t)i);
            if (key < thr) {
                queue[cnt * 64] = key;
                ++cnt;
            }
        }
    }
    for (int i = 0; __any(i < cnt); ++i) {
        if (i < cnt) {
            const uint64_t key = queue[i * 64];
            if (key < L[KL - 1]) list_insert<KL>(L, key);
        }
    }
    // publish this partial list's k-th key (the query's bound is the min over
    // its partial lists)
    if (L[KL - 1] < thr) atomicMin(reinterpret_cast<unsigned long long*>(thr_slot), (unsigned long long)L[KL - 1]);
}

// Kept in lock-step with scan_kernel (lmi_scan_v12.hip): its tile queue, query
// staging, MFMA loops, list merge and `partial` layout, word for word; the
// epilogue alone differs.
template <int KL, bool F16MATH, typename TC, int METRIC>
__global__ __launch_bounds__(kThreads, 1) void scan_kernel_metric(ScanArgs a) {
    using Cfg = ScanCfg<KL, F16MATH>;
    using QT = typename Cfg::QT;
    constexpr int QB = Cfg::QB, NQF = Cfg::NQF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int d_pad = a.d_pad;
    const int ldq = d_pad + Cfg::QPAD;
    const size_t qs_bytes = std::max((size_t)QB * ldq * sizeof(QT),
                                     (size_t)QB * 2 * kWaves * KL * sizeof(uint64_t));
    QT* Qs = reinterpret_cast<QT*>(smem);
    uint64_t* mergebuf = reinterpret_cast<uint64_t*>(smem);  // aliases Qs after the scan
    uint64_t* queue_all = reinterpret_cast<uint64_t*>(smem + qs_bytes);
    uint64_t* thr_s = queue_all + kWaves * kQCap * 64;
    float* invq_s = reinterpret_cast<float*>(thr_s + QB);
    // no static __shared__ in this kernel: it would shift the dynamic base
    // off 16-B alignment and every ds_read_b128 would replay (guide G17)
    int& s_tile = *reinterpret_cast<int*>(invq_s + QB);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int h = lane >> 5;
    const int col = lane & 31;
    uint64_t* queue = queue_all + wave * kQCap * 64 + lane;

    const TC* __restrict__ corpus = reinterpret_cast<const TC*>(a.corpus);
    const QT* __restrict__ qbuf = reinterpret_cast<const QT*>(a.qbuf);
    const int ntiles = a.meta[2 * kGroups];

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
                // (l2: |q|^2; ip: no word, the prep writes none)
                invq_s[r] = (METRIC != LMI_METRIC_IP && live) ? a.invq[a.pair_q[tile.pp0 + r] / a.R] : 0.0f;
                thr_s[r] = live ? kEmptyKey : 0ull;  // dead slots reject everything
            }
        }
        __syncthreads();

        uint64_t L[NQF][KL];
#pragma unroll
        for (int f = 0; f < NQF; ++f) list_clear<KL>(L[f]);

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
                // MFMA step s (0..3), element j  <->  k = kb + 32h + 8s + j.
                // A and B use the same permutation of k, so the dot is exact.
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
                    // only lane-half h covers k = kb*64 + 16h + [0,16) here
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
                // group s (0..3) of 4 MFMAs 32x32x2, element j <-> k = kb + 16h + 4s + j.
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

            const uint32_t row_base = (uint32_t)(row0 + sub0);
            const int valid_rows = nrows - sub0;
#pragma unroll
            for (int f = 0; f < NQF; ++f) {
                const int qslot = 32 * f + col;
                metric_epilogue<KL, METRIC>(acc[f], L[f], &thr_s[qslot], invq_s[qslot], a.inv_norm, row_base,
                                            valid_rows, queue, lane);
            }
        }
        __syncthreads();  // all waves done with Qs -> reuse as merge buffer

        // ---- merge the 2*kWaves partial lists of every query --------------
        // list index of (wave, half) = 2*wave + h; layout [qslot][list][KL]
#pragma unroll
        for (int f = 0; f < NQF; ++f) {
            uint64_t* dst = mergebuf + ((size_t)(32 * f + col) * (2 * kWaves) + 2 * wave + h) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) dst[i] = L[f][i];
        }
        __syncthreads();
        if (tid < tile.np) {
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
            uint64_t* out = a.partial + ((size_t)(tile.pp0 + tid) * a.max_chunks + tile.chunk) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) out[i] = M[i];
        }
        __syncthreads();
    }
}

// prep_kernel for a metric scan (LMI_METRIC_L2 / _IP): the queries as they are
// -- not normalised -- rounded to qbuf like prep_kernel's, and for l2 invq =
// |q|^2 by the rows' own device function (row_sqnorm: float64 accumulation,
// one rounding); ip writes no word.  The output prefill and the word fills as
// prep_kernel's.  VEC: float4 loads of the query rows (16-byte aligned, ldq % 4 == 0).
template <bool F16, bool VEC>
__global__ __launch_bounds__(kThreads) void prep_metric_kernel(const float* __restrict__ q, int32_t nq,
                                                               int32_t ldq, int32_t d, int32_t d_pad,
                                                               int32_t metric, void* __restrict__ qbuf,
                                                               float* __restrict__ invq,
                                                               int32_t* __restrict__ status,
                                                               float* __restrict__ out_d,
                                                               int32_t* __restrict__ out_pos,
                                                               int32_t* __restrict__ out_row,
                                                               int32_t out_per_q, WordFills fills) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;  // (wave-uniform; no block-wide barrier below)
    const float* src = q + (size_t)row * ldq;
    bool inexact = false;
    for (int c0 = 4 * lane; c0 < d_pad; c0 += 256) {  // d_pad is a multiple of 32
        float v[4];
        quant_load4<VEC>(src, c0, d, v);
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
    if constexpr (F16) {
        if (__any(inexact) && lane == 0) atomicOr(status, LMI_STATUS_QUERY_NOT_F16);
    }
    if (metric == LMI_METRIC_L2) {  // (the second read of the row hits the cache)
        const float qq = row_sqnorm<float, VEC>(src, d, lane);
        if (lane == 0) invq[row] = qq;
    }
    prep_fill_tail(row, lane, out_d, out_pos, out_row, out_per_q, fills);
}

}  // namespace

int launch_prep_metric(bool f16, const float* q, int32_t nq, int32_t ldq, int32_t d, int32_t d_pad, int32_t metric,
                       void* qbuf, float* invq, int32_t* status, float* out_d, int32_t* out_pos, int32_t* out_row,
                       int32_t out_per_q, const WordFills& fills, hipStream_t s) {
    const dim3 pg((nq + kThreads / 64 - 1) / (kThreads / 64));
    const bool vec = ((uintptr_t)q % 16 == 0) && (ldq % 4 == 0);
    auto* kp = f16 ? (vec ? prep_metric_kernel<true, true> : prep_metric_kernel<true, false>)
                   : (vec ? prep_metric_kernel<false, true> : prep_metric_kernel<false, false>);
    hipLaunchKernelGGL(kp, pg, dim3(kThreads), 0, s, q, nq, ldq, d, d_pad, metric, qbuf, invq, status, out_d,
                       out_pos, out_row, out_per_q, fills);
    LMI_LAUNCH_CHECK("prep_metric_kernel");
    return LMI_OK;
}

// the 8-wave ring's plain 10-entry lists (k <= 10)
template <int KL, int METRIC>
int launch_scan3_metric(const Scan2Args& b, hipStream_t s) {
    return launch_scan3_v<KL, 0, false, METRIC == LMI_METRIC_L2 ? 5 : 6>(b, s);
}

template <int KL, bool F16MATH, typename TC, int METRIC>
int launch_scan_metric(const ScanArgs& a, int d_pad, hipStream_t s) {
    const size_t lds = scan_lds_bytes<KL, F16MATH>(d_pad);
    if (d_pad > kMetricMaxDPad || lds > 160 * 1024) {
        set_error("metric scan: d_pad=%d above %d", d_pad, kMetricMaxDPad);
        return LMI_E_UNSUPPORTED;
    }
    return launch_dyn_lds<scan_kernel_metric<KL, F16MATH, TC, METRIC>>("scan_kernel_metric", dim3(num_cus()),
                                                                       dim3(kThreads), lds, s, a);
}

#define LMI_METRIC_INST(M)                                                                        \
    template int launch_scan_metric<10, true, _Float16, M>(const ScanArgs&, int, hipStream_t);    \
    template int launch_scan_metric<16, true, _Float16, M>(const ScanArgs&, int, hipStream_t);    \
    template int launch_scan_metric<10, false, _Float16, M>(const ScanArgs&, int, hipStream_t);   \
    template int launch_scan_metric<16, false, _Float16, M>(const ScanArgs&, int, hipStream_t);   \
    template int launch_scan_metric<10, false, float, M>(const ScanArgs&, int, hipStream_t);      \
    template int launch_scan_metric<16, false, float, M>(const ScanArgs&, int, hipStream_t);      \
    template int launch_scan3_metric<10, M>(const Scan2Args&, hipStream_t);
LMI_METRIC_INST(LMI_METRIC_L2)
LMI_METRIC_INST(LMI_METRIC_IP)
#undef LMI_METRIC_INST

}  // namespace lmi
