// 8-bit storage: the one device function that turns a vector into int8 codes
// (include/lmi_hip.h, lmi_quantize_rows_i8).  The row quantiser (lmi_quant.hip)
// and the query prep of an LMI_I8 scan (prep_i8_kernel, lmi_scan.hip) both call
// it, so rows and queries cannot drift apart.  Not an ABI.
#pragma once
#include "lmi_common.hpp"

#include <hip/hip_fp16.h>

namespace lmi {

// four consecutive values of a row as float32, zeros past d; VEC: the row is
// aligned for one vector load of four elements
template <bool VEC>
__device__ __forceinline__ void quant_load4(const float* __restrict__ src, int c0, int d, float (&v)[4]) {
    if (VEC && c0 + 3 < d) {
        const float4 f = *reinterpret_cast<const float4*>(src + c0);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (c0 + e < d) ? src[c0 + e] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void quant_load4(const __half* __restrict__ src, int c0, int d, float (&v)[4]) {
    if (VEC && c0 + 3 < d) {
        union { uint2 u; __half h[4]; } p;
        p.u = *reinterpret_cast<const uint2*>(src + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __half2float(p.h[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (c0 + e < d) ? __half2float(src[c0 + e]) : 0.0f;
    }
}

// One wave quantises one vector: src[0..d) -> dst[0..d_pad) (4-byte aligned,
// d_pad a multiple of 32), returns 1/||codes|| on every lane.
//   m = max |v_j| (a NaN anywhere makes it NaN); !(m >= 2^-100): all codes 0
//   s = m / 127.0f; c_j = clamp(rintf(v_j / s), -127, 127)   (IEEE divisions)
//   ss = sum c_j^2 in int32 (<= d_pad * 127^2: exact for d_pad < 133 000)
//   inv = ss == 0 ? 1 : (float)(1.0 / sqrt((double)ss))
// The row is read twice (the second pass hits the cache); each lane owns runs
// of four consecutive columns and writes them as one 32-bit word.
template <typename T, bool VEC>
__device__ inline float quantize_row_i8(const T* __restrict__ src, int d, int d_pad, int lane,
                                        int8_t* __restrict__ dst) {
    float m = 0.0f;
    bool nan = false;
    for (int c0 = 4 * lane; c0 < d; c0 += 256) {
        float v[4];
        quant_load4<VEC>(src, c0, d, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            nan |= v[e] != v[e];
            m = fmaxf(m, fabsf(v[e]));
        }
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    const bool zero = __any(nan) || !(m >= 0x1p-100f);
    const float s = __fdiv_rn(m, 127.0f);
    int ss = 0;
    for (int c0 = 4 * lane; c0 < d_pad; c0 += 256) {
        uint32_t word = 0u;
        if (!zero && c0 < d) {
            float v[4];
            quant_load4<VEC>(src, c0, d, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float r = fminf(fmaxf(rintf(__fdiv_rn(v[e], s)), -127.0f), 127.0f);
                const int c = (int)r;
                ss += c * c;
                word |= ((uint32_t)c & 0xffu) << (8 * e);
            }
        }
        *reinterpret_cast<uint32_t*>(dst + c0) = word;
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    return ss == 0 ? 1.0f : (float)(1.0 / sqrt((double)ss));
}

}  // namespace lmi
