// The reference's float64 distance of one (query, stored row), a wave per
// row: d = 1 - <q/|q|, y/|y|> in sklearn.normalize + GEMM order (the header
// comment of lmi_refine.hip).  Shared by the float64 refine, the range
// rescore (lmi_refine.hip) and the re-rank of 8-bit lists (lmi_rerank.hip):
// one definition, so every entry point gives a (query, row) the same bits.
// Not an ABI.
#pragma once
#include "lmi_common.hpp"

namespace lmi {

constexpr double kEps64 = 2.220446049250313e-16;

__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the 4-element pieces of a row a lane owns: piece l + 64 i (i < nps)
template <typename TC>
__device__ inline void load_piece(const TC* row, int piece, int d, double (&v)[4]) {
    const int e0 = 4 * piece;
    if constexpr (sizeof(TC) == 2) {
        if (e0 + 4 <= d) {
            const uint2 raw = *reinterpret_cast<const uint2*>(row + e0);
            _Float16 h[4];
            __builtin_memcpy(h, &raw, 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (double)h[j];
            return;
        }
    } else if constexpr (sizeof(TC) == 8) {
        if (e0 + 4 <= d) {
            const double2 a = *reinterpret_cast<const double2*>(row + e0);
            const double2 b = *reinterpret_cast<const double2*>(row + e0 + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
            return;
        }
    } else {
        if (e0 + 4 <= d) {
            const float4 f = *reinterpret_cast<const float4*>(row + e0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (e0 + j < d) ? (double)row[e0 + j] : 0.0;
}

constexpr int kMaxPieces = 4;  // d <= 1024 (4 pieces of 4 per lane)

// q^ for this lane's pieces (sklearn normalize of the query row, float64)
template <typename TQ, int NP = kMaxPieces>
__device__ inline void query_hat(const TQ* qrow, int d, int nps, double (&qh)[NP][4]) {
    const int lane = threadIdx.x & 63;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * (lane + 64 * i) + j;
            const double v = (i < nps && e < d) ? (double)qrow[e] : 0.0;
            qh[i][j] = v;
            ss = fma(v, v, ss);
        }
    }
    double n = sqrt(wave_sum_d(ss));
    if (n < 10.0 * kEps64) n = 1.0;  // sklearn _handle_zeros_in_scale
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) qh[i][j] = qh[i][j] / n;
}

// 1 - <q^, y/|y|> of one stored row, float64 (every lane gets the value)
template <typename TC, int NP = kMaxPieces>
__device__ inline double row_dist64(const TC* row, int d, int nps, const double (&qh)[NP][4]) {
    const int lane = threadIdx.x & 63;
    double dot = 0.0, ss = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (i < nps) {
            double v[4];
            load_piece<TC>(row, lane + 64 * i, d, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dot = fma(qh[i][j], v[j], dot);
                ss = fma(v[j], v[j], ss);
            }
        }
    }
    dot = wave_sum_d(dot);
    double n = sqrt(wave_sum_d(ss));
    if (n < 10.0 * kEps64) n = 1.0;
    return 1.0 - dot / n;
}

// row_dist64 of up to kB fp16 rows at once (d % 4 == 0): every row's pieces
// are loaded before any is used, so a wave waits one memory latency per kB
// rows instead of one per row, and the 2 kB wave reductions interleave; each
// row's value is computed in exactly row_dist64's order (the same bits)
// (NPS: pieces per lane known at compile time, 3 for d in (512, 768])
constexpr int kB = 4;
template <int NPS, int KB = kB>
__device__ inline void rows_dist64_f16(const _Float16* base, size_t d_pad, const int32_t (&r)[KB], int d,
                                       int nps, const double (&qh)[NPS][4], double (&out)[KB]) {
    const int lane = threadIdx.x & 63;
    uint2 raw[KB][NPS];
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
        for (int i = 0; i < NPS; ++i) {
            const int e0 = 4 * (lane + 64 * i);
            raw[b][i] = (r[b] >= 0 && i < nps && e0 + 4 <= d)
                            ? *reinterpret_cast<const uint2*>(base + (size_t)r[b] * d_pad + e0)
                            : make_uint2(0u, 0u);
        }
    double dot[KB], ss[KB];
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        dot[b] = 0.0;
        ss[b] = 0.0;
#pragma unroll
        for (int i = 0; i < NPS; ++i) {
            if (i < nps) {
                _Float16 h[4];
                __builtin_memcpy(h, &raw[b][i], 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double v = (double)h[j];
                    dot[b] = fma(qh[i][j], v, dot[b]);
                    ss[b] = fma(v, v, ss[b]);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            dot[b] += __shfl_xor(dot[b], off);
            ss[b] += __shfl_xor(ss[b], off);
        }
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        double n = sqrt(ss[b]);
        if (n < 10.0 * kEps64) n = 1.0;
        out[b] = 1.0 - dot[b] / n;
    }
}

__device__ inline bool lt_dp(double a, int32_t pa, double b, int32_t pb) {
    return a < b || (a == b && pa < pb);
}

}  // namespace lmi
