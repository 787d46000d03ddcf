// Metrics of the scan (include/lmi_hip.h, LMI_METRIC_*): the distance every
// metric scan computes from the MFMA accumulator, and the one device function
// that turns a vector into its squared norm.  The row kernel (lmi_metric.hip,
// lmi_row_sqnorms) and the query prep of a metric scan (prep_metric_kernel,
// lmi_scan_metric.hip) both call it, so rows and queries cannot drift apart.  New to
// this project: the reference scores by cosine alone (utils.py:10-11).
// Not an ABI.
#pragma once
#include "lmi_common.hpp"

#include <hip/hip_fp16.h>

namespace lmi {

// d of a (query, row) pair: acc = sum_j q_j y_j, wq / wy the pair's per-query
// and per-row words (cosine: 1/|q|, 1/|y|; l2: |q|^2, |y|^2; ip: unused).
// One expression for the filter and for the walk that rebuilds a candidate's
// distance: both must give the same bits.
template <int METRIC>
__device__ __forceinline__ float metric_dist(float acc, float wq, float wy) {
    if constexpr (METRIC == LMI_METRIC_L2) {
        return fmaf(-2.0f, acc, wq + wy);
    } else if constexpr (METRIC == LMI_METRIC_IP) {
        return -acc;
    } else {
        return fmaf(-acc, wq * wy, 1.0f);
    }
}

__device__ __forceinline__ float sq_f32(float v) { return v; }
__device__ __forceinline__ float sq_f32(__half v) { return __half2float(v); }

// One wave, one vector: sum_j src[j]^2 over j < d, accumulated in float64 and
// rounded once to float32, on every lane.  Each lane takes runs of 16 bytes
// (VEC: the vector is 16-byte aligned, one load a run; the run that straddles
// d and unaligned vectors go element by element), squares in float64 (exact:
// a float32 square has 48 bits), adds with fma, and a 6-level butterfly sums
// the lanes: at most d float64 roundings, far inside the one float32 rounding.
template <typename T, bool VEC>
__device__ inline float row_sqnorm(const T* __restrict__ src, int d, int lane) {
    constexpr int EPV = 16 / (int)sizeof(T);
    double ss = 0.0;
    for (int c0 = EPV * lane; c0 < d; c0 += 64 * EPV) {
        float v[EPV];
        if (VEC && c0 + EPV <= d) {
            union { uint4 u; T t[EPV]; } p;
            p.u = *reinterpret_cast<const uint4*>(src + c0);
#pragma unroll
            for (int e = 0; e < EPV; ++e) v[e] = sq_f32(p.t[e]);
        } else {
#pragma unroll
            for (int e = 0; e < EPV; ++e) v[e] = (c0 + e < d) ? sq_f32(src[c0 + e]) : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < EPV; ++e) ss = fma((double)v[e], (double)v[e], ss);
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    return (float)ss;
}

}  // namespace lmi
