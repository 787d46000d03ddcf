// 8-bit storage: lmi_quantize_rows_i8 (include/lmi_hip.h) -- rows of an fp16 or
// float32 block to int8 codes and the codes' 1/||c||, one wave per row, straight
// into their slots of the store (dst_rows: the bucket-sorted scatter of an index
// build).  New to this project: the reference keeps its rows as the data set
// gives them (search.py:79-84) and has no quantised form.
#include "lmi_quant.hpp"

#include <algorithm>

namespace lmi {
namespace {

constexpr int kQuantThreads = 256;   // 4 waves: 4 rows per workgroup pass
constexpr int kQuantMaxGrid = 8192;  // grid-strided beyond

template <typename T, bool VEC>
__global__ __launch_bounds__(kQuantThreads) void quantize_rows_kernel(
    const T* __restrict__ rows, int64_t m, int64_t ld, int32_t d, int32_t d_pad,
    const int64_t* __restrict__ dst_rows, int8_t* __restrict__ codes, float* __restrict__ inv_norm) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kQuantThreads / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kQuantThreads / 64);
    for (int64_t i = wave; i < m; i += nwaves) {  // (wave-uniform: no barrier below)
        const int64_t to = dst_rows ? dst_rows[i] : i;
        const float inv = quantize_row_i8<T, VEC>(rows + i * ld, d, d_pad, lane, codes + to * d_pad);
        if (lane == 0) inv_norm[to] = inv;
    }
}

}  // namespace
}  // namespace lmi

extern "C" int lmi_quantize_rows_i8(const void* rows, int32_t dtype, int64_t m, int64_t ld, int32_t d,
                                    int32_t d_pad, const int64_t* dst_rows, int8_t* codes, float* inv_norm,
                                    void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(dtype == LMI_F16 || dtype == LMI_F32, "quantize rows: dtype=%d (LMI_F16 or LMI_F32)", dtype);
    LMI_CHECK_ARG(m >= 0, "quantize rows: m=%lld", (long long)m);
    LMI_CHECK_ARG(d > 0 && d_pad >= d && d_pad % 32 == 0 && d_pad - d < 32,
                  "quantize rows: d=%d d_pad=%d (d rounded up to a multiple of 32)", d, d_pad);
    LMI_CHECK_ARG(ld >= d, "quantize rows: ld=%lld < d=%d", (long long)ld, d);
    if (m == 0) return LMI_OK;
    LMI_CHECK_ARG(rows && codes && inv_norm, "quantize rows: null pointer");
    LMI_CHECK_ARG((reinterpret_cast<uintptr_t>(codes) & 3) == 0, "quantize rows: codes not 4-byte aligned");
    // one vector load of four elements: 16 B (float32) / 8 B (fp16) alignment of every run
    const int64_t el = dtype == LMI_F16 ? 2 : 4;
    const bool vec = (reinterpret_cast<uintptr_t>(rows) % (4 * el)) == 0 && ld % 4 == 0;
    const unsigned grid = (unsigned)std::min<int64_t>((m + kQuantThreads / 64 - 1) / (kQuantThreads / 64),
                                                      kQuantMaxGrid);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define LMI_QUANT(T, V)                                                                              \
    hipLaunchKernelGGL((quantize_rows_kernel<T, V>), dim3(grid), dim3(kQuantThreads), 0, s,          \
                       static_cast<const T*>(rows), m, ld, d, d_pad, dst_rows, codes, inv_norm)
    if (dtype == LMI_F16) {
        if (vec) LMI_QUANT(__half, true); else LMI_QUANT(__half, false);
    } else {
        if (vec) LMI_QUANT(float, true); else LMI_QUANT(float, false);
    }
#undef LMI_QUANT
    LMI_LAUNCH_CHECK("quantize_rows_kernel");
    return LMI_OK;
}
