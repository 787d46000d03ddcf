// Parts that the 8-wave rings on quantised storage share (scan3_i8_kernel,
// lmi_scan_ring_i8.hip; scan3_mx4_kernel / scan3_mx6_kernel,
// lmi_scan_ring_mx.hip): the list clear at the head of a tile and the end of a
// tile.  They take scalars by value: the same text behind a reference to a
// struct of the tile's values compiled to another schedule.  The wave -> slot
// numbering, the tile head and the block epilogue are the same text in the i8
// ring and in ring_mx_body and are NOT here: as functions they moved the
// kernels' register allocation and the rings measured 0.5 to 2 % slower
// (DESIGN.md "Where a ring's parts live").
#pragma once
#include "lmi_scan3.hpp"

namespace lmi {
namespace {

// Every lane's list to EMPTY, then the barrier that ends the tile's set-up (the
// wave's loads and first DMA waited for)
template <int KL>
__device__ __forceinline__ void ring_lists_clear(uint32_t lbase) {
    {
        uint64_t E[KL];
        list_clear<KL>(E);
        list_store<KL>(opaque_u(lbase), E);
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
    __syncthreads();
}

// The end of a tile: the lists still in append mode sorted, the barrier behind
// which every wave's DMA has drained (the loop's tail waited vmcnt(0)), the two
// partial lists of each query (lanes col, col + 32) merged into `partial`, and
// the pair's global bound lowered to the merged list's last key.
template <int KL>
__device__ __forceinline__ void ring_finish(uint64_t* partial, int max_chunks, unsigned long long* thr_g, int pp,
                                            int chunk, int h, bool live, uint32_t lbase, int cnt) {
    // lanes still in append mode hold an unsorted (EMPTY-padded) buffer
    if (__any(cnt < KL)) {
        if (cnt < KL) {
            uint64_t L[KL];
            list_load<KL>(lbase, L);
            list_sort<KL>(L);
            list_store<KL>(lbase, L);
        }
    }
    __syncthreads();
    if (h == 0 && live) {
        uint64_t L[KL], P[KL];
        list_load<KL, 0>(lbase, L);
        list_load<KL, 32 * 8>(lbase, P);
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            if (P[i] >= L[KL - 1]) break;
            list_insert<KL>(L, P[i]);
        }
        uint64_t* out = partial + ((size_t)pp * max_chunks + chunk) * KL;
#pragma unroll
        for (int i = 0; i < KL; ++i) out[i] = L[i];
        if (L[KL - 1] != kEmptyKey) atomicMin(&thr_g[pp], (unsigned long long)L[KL - 1]);
    }
}

}  // namespace
}  // namespace lmi
