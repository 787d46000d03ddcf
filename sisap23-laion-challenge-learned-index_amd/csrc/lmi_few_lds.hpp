// What the few-query scan (lmi_scan_few.hip) and its gathered sibling
// (lmi_scan_subset.hip) share: the ring's shape and the LDS reads of the stage
// loop -- inline asm: a C++ LDS access inside a ring of LDS DMAs makes the
// compiler wait for every DMA in flight first.  (The stage loop's body, the
// epilogue and the slice-end merge stay written out in both kernels: called
// through shared device functions, scan_few_kernel no longer compiles to the
// code it had -- 232 -> 236 VGPRs at 10 entries, 244 -> 276 and 48 AGPRs at 16.)
#pragma once
#include "lmi_scan_internal.hpp"

#include <algorithm>

namespace lmi {

namespace few {
constexpr int KSEG = 128;                 // k elements of a stage
constexpr int ROWB = KSEG * 2;            // bytes of one row in one stage
constexpr int STAGE = 32 * ROWB;          // 8 KiB
constexpr int NSLOT = 3;                  // per wave: one read, two in flight
constexpr int NORMB = 32 * 4;             // a stage's norms
constexpr int QPAD = 8;                   // elements: the query rows' pitch is 2 d_pad + 16 B
constexpr int DMAS = STAGE / 1024 + 1;    // DMA instructions of a stage
constexpr int TAB_HDR = 4, TAB_ENT = 5;   // the group table: (n groups, n items, -, -), then entries
}  // namespace few

// four / eight 16-byte LDS reads in flight and their wait, out of the compiler's sight
__device__ __forceinline__ void lds_read4(half8 (&v)[8], int o, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    asm volatile(
        "ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(v[o]), "=&v"(v[o + 1]), "=&v"(v[o + 2]), "=&v"(v[o + 3])
        : "v"(a0), "v"(a1), "v"(a2), "v"(a3)
        : "memory");
}
__device__ __forceinline__ void lds_read8_affine(half8 (&v)[8], uint32_t a) {
    asm volatile(
        "ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:32\n\tds_read_b128 %2, %8 offset:64\n\t"
        "ds_read_b128 %3, %8 offset:96\n\tds_read_b128 %4, %8 offset:128\n\tds_read_b128 %5, %8 offset:160\n\t"
        "ds_read_b128 %6, %8 offset:192\n\tds_read_b128 %7, %8 offset:224\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
        : "v"(a)
        : "memory");
}
// (a short last segment: two fragments at a time, so that no read leaves the query row)
template <int O>
__device__ __forceinline__ void lds_read2_affine(half8 (&v)[8], uint32_t a) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[O]), "=&v"(v[O + 1])
                 : "v"(a), "i"(32 * O), "i"(32 * O + 32)
                 : "memory");
}
__device__ __forceinline__ void lds_read_norms(f32x4 (&n)[4], uint32_t a) {
    asm volatile(
        "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:32\n\tds_read_b128 %2, %4 offset:64\n\t"
        "ds_read_b128 %3, %4 offset:96\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(n[0]), "=&v"(n[1]), "=&v"(n[2]), "=&v"(n[3])
        : "v"(a)
        : "memory");
}

}  // namespace lmi
