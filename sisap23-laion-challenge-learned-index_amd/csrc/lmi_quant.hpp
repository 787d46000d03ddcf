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

// 4-bit storage: the one device function that turns a vector into MXFP4 codes
// (include/lmi_hip.h, "the MXFP4 format"); the row quantiser (lmi_quant.hip) and
// the query prep of an LMI_MX4 scan (prep_mx4_kernel, lmi_scan_ring_mx.hip)
// both call it.
// One wave quantises one vector: src[0..d) -> codes[0..d_pad/2) (4-byte
// aligned) and scales[0..d_pad/32), d_pad a multiple of 64; returns the codes'
// 1/n on every lane.  A pass takes 512 columns: lane l owns the eight
// consecutive columns 8l.. (one 32-bit word of codes), four lanes own a block.
//   block b:  m = max |v_j| (a NaN anywhere makes the block zero)
//             !(m >= 2^-100): codes +0, scale byte 127
//             else byte = exponent field of m - 2 (e_b + 127), t_j = v_j 2^-e_b
//             (one exact multiplication), code = E2M1 nearest |t_j|, ties to the
//             even mantissa, saturating at 6; a zero code carries no sign
//   scales :  byte of block b at (b & 1) * d_pad/64 + (b >> 1)
//   n^2    :  sum_b S_b 2^(2 e_b - 2), S_b = sum_j (2 c_j)^2 an integer, summed
//             in float64 in block order (lane shuffles in a fixed order)
template <typename T, bool VEC>
__device__ inline float quantize_row_mx4(const T* __restrict__ src, int d, int d_pad, int lane,
                                         uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
    const int half_blocks = d_pad >> 6;
    double n2 = 0.0;
    for (int base = 0; base < d_pad; base += 512) {
        const int c0 = base + 8 * lane;
        float v[2][4] = {};
        if (c0 < d) {
            quant_load4<VEC>(src, c0, d, v[0]);
            quant_load4<VEC>(src, c0 + 4, d, v[1]);
        }
        float m = 0.0f;
        int nan = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = v[e >> 2][e & 3];
            nan |= (x != x) ? 1 : 0;
            m = fmaxf(m, fabsf(x));
        }
#pragma unroll
        for (int off = 1; off < 4; off <<= 1) {
            m = fmaxf(m, __shfl_xor(m, off));
            nan |= __shfl_xor(nan, off);
        }
        const bool zero = nan != 0 || !(m >= 0x1p-100f);
        const uint32_t ef = zero ? 129u : (__float_as_uint(m) >> 23) & 0xffu;  // e_b = ef - 129
        const float mul = __uint_as_float((256u - ef) << 23);                  // 2^-e_b
        uint32_t word = 0u;
        int ss = 0;
        if (!zero) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = v[e >> 2][e & 3] * mul;
                const float a = fabsf(t);
                const uint32_t idx = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                                     (a >= 3.5f) + (a > 5.0f);
                const int c2 = (int)((0xC8643210u >> (4 * idx)) & 15u);  // 2 |c|
                ss += c2 * c2;
                word |= (idx | ((t < 0.0f && idx != 0u) ? 8u : 0u)) << (4 * e);
            }
        }
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        if (c0 < d_pad) {
            *reinterpret_cast<uint32_t*>(codes + (c0 >> 1)) = word;
            const int b = c0 >> 5;
            if ((lane & 3) == 0) scales[(b & 1) * half_blocks + (b >> 1)] = (uint8_t)(ef - 2u);
        }
        // S_b 2^(2 e_b - 2): exact in float64 (S_b <= 4608)
        const double term = (double)ss * __hiloint2double((int)((1023u + 2u * ef - 260u) << 20), 0);
#pragma unroll
        for (int j = 0; j < 16; ++j) n2 += __shfl(term, 4 * j);
    }
    return n2 == 0.0 ? 1.0f : (float)(1.0 / sqrt(n2));
}

// 6-bit storage: the one device function that turns a vector into MXFP6 codes
// (include/lmi_hip.h, "the MXFP6 format"); the row quantiser (lmi_quant.hip) and
// the query prep of an LMI_MX6 scan (prep_mx6_kernel, lmi_scan_ring_mx.hip)
// both call it.
// One wave quantises one vector: src[0..d) -> codes[0..d_pad*3/4) (4-byte
// aligned) and scales[0..d_pad/32), d_pad a multiple of 64; returns the codes'
// 1/n on every lane.  A pass takes 512 columns: lane l owns the eight
// consecutive columns 8l.. (48 bits of codes), four lanes own a block's 24-byte
// fragment and write it as six 32-bit words (the even lane of a pair two, the
// odd lane one).
//   block b:  scale byte and t_j as quantize_row_mx4
//             code = E2M3 nearest |t_j|: index i = 8 * exponent field + mantissa
//             is monotone in the magnitude -- |t| < 2: rint(8 |t|); < 4: 16 +
//             rint(4 (|t| - 2)); else 24 + rint(2 (|t| - 4)), at most 31 (7.5).
//             Every product and difference there is exact and rint rounds ties
//             to the even integer, which is the even mantissa (16 and 24 are
//             even); bit 5 is the sign, never set on a zero code
//   fragment: the code of column j of the block in bits [6j, 6j + 6) of the
//             block's 192-bit little-endian string
//   scales :  byte of block b at (b & 1) * d_pad/64 + (b >> 1)
//   n^2    :  sum_b S_b 2^(2 e_b - 6), S_b = sum_j (8 c_j)^2 an integer, summed
//             in float64 in block order (lane shuffles in a fixed order)
template <typename T, bool VEC>
__device__ inline float quantize_row_mx6(const T* __restrict__ src, int d, int d_pad, int lane,
                                         uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
    const int half_blocks = d_pad >> 6;
    double n2 = 0.0;
    for (int base = 0; base < d_pad; base += 512) {
        const int c0 = base + 8 * lane;
        float v[2][4] = {};
        if (c0 < d) {
            quant_load4<VEC>(src, c0, d, v[0]);
            quant_load4<VEC>(src, c0 + 4, d, v[1]);
        }
        float m = 0.0f;
        int nan = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = v[e >> 2][e & 3];
            nan |= (x != x) ? 1 : 0;
            m = fmaxf(m, fabsf(x));
        }
#pragma unroll
        for (int off = 1; off < 4; off <<= 1) {
            m = fmaxf(m, __shfl_xor(m, off));
            nan |= __shfl_xor(nan, off);
        }
        const bool zero = nan != 0 || !(m >= 0x1p-100f);
        const uint32_t ef = zero ? 129u : (__float_as_uint(m) >> 23) & 0xffu;  // e_b = ef - 129
        const float mul = __uint_as_float((256u - ef) << 23);                  // 2^-e_b
        uint32_t lo = 0u, hi = 0u;  // the lane's 48 bits: codes 0..4 and the low 2 bits of 5 | the rest
        int ss = 0;
        if (!zero) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = v[e >> 2][e & 3] * mul;
                const float a = fabsf(t);
                const float r = a < 2.0f ? rintf(a * 8.0f)
                                : a < 4.0f ? 16.0f + rintf((a - 2.0f) * 4.0f) : 24.0f + rintf((a - 4.0f) * 2.0f);
                const uint32_t idx = min((uint32_t)r, 31u);
                const int c8 = (int)(idx < 16u ? idx : idx < 24u ? 2u * idx - 16u : 4u * idx - 64u);  // 8 |c|
                ss += c8 * c8;
                const uint64_t code = idx | ((t < 0.0f && idx != 0u) ? 32u : 0u);
                const uint64_t sh = code << (6 * e);
                lo |= (uint32_t)sh;
                hi |= (uint32_t)(sh >> 32);
            }
        }
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        // the pair's 96 bits: the even lane's 48, then the odd lane's
        const uint32_t plo = __shfl_xor(lo, 1);
        if (c0 < d_pad) {
            uint32_t* w = reinterpret_cast<uint32_t*>(codes + (c0 >> 3) * 6 - (lane & 1) * 6);  // the pair's 12 bytes
            if ((lane & 1) == 0) {
                w[0] = lo;
                w[1] = hi | (plo << 16);
            } else {
                w[2] = (lo >> 16) | (hi << 16);
            }
            const int b = c0 >> 5;
            if ((lane & 3) == 0) scales[(b & 1) * half_blocks + (b >> 1)] = (uint8_t)(ef - 2u);
        }
        // S_b 2^(2 e_b - 6): exact in float64 (S_b <= 115 200)
        const double term = (double)ss * __hiloint2double((int)((1023u + 2u * ef - 264u) << 20), 0);
#pragma unroll
        for (int j = 0; j < 16; ++j) n2 += __shfl(term, 4 * j);
    }
    return n2 == 0.0 ? 1.0f : (float)(1.0 / sqrt(n2));
}

}  // namespace lmi
