// Metric scans: lmi_row_sqnorms (include/lmi_hip.h) -- the per-row word of an
// index searched by squared Euclidean distance, |y|^2 of every row of an fp16
// or float32 block, one wave per row, straight into the rows' slots of the
// store (dst_rows: the bucket-sorted scatter of an index build).  The scan
// variants that read it are scan3_kernel MODE 5 (lmi_scan3.hpp) and
// scan_kernel_metric (lmi_scan_metric.hip); the queries' |q|^2 comes from the
// same device function (lmi_metric.hpp), in prep_metric_kernel.
#include "lmi_metric.hpp"

#include <algorithm>

namespace lmi {
namespace {

constexpr int kSqThreads = 256;   // 4 waves: 4 rows per workgroup pass
constexpr int kSqMaxGrid = 8192;  // grid-strided beyond

template <typename T, bool VEC>
__global__ __launch_bounds__(kSqThreads) void row_sqnorms_kernel(const T* __restrict__ rows, int64_t m,
                                                                 int64_t ld, int32_t d,
                                                                 const int64_t* __restrict__ dst_rows,
                                                                 float* __restrict__ sqnorm) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kSqThreads / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kSqThreads / 64);
    for (int64_t i = wave; i < m; i += nwaves) {  // (wave-uniform: no barrier below)
        const float ss = row_sqnorm<T, VEC>(rows + i * ld, d, lane);
        if (lane == 0) sqnorm[dst_rows ? dst_rows[i] : i] = ss;
    }
}

}  // namespace
}  // namespace lmi

extern "C" int lmi_row_sqnorms(const void* rows, int32_t dtype, int64_t m, int64_t ld, int32_t d,
                               const int64_t* dst_rows, float* sqnorm, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(dtype == LMI_F16 || dtype == LMI_F32, "row sqnorms: dtype=%d (LMI_F16 or LMI_F32)", dtype);
    LMI_CHECK_ARG(m >= 0, "row sqnorms: m=%lld", (long long)m);
    LMI_CHECK_ARG(d > 0 && ld >= d, "row sqnorms: d=%d ld=%lld", d, (long long)ld);
    if (m == 0) return LMI_OK;
    LMI_CHECK_ARG(rows && sqnorm, "row sqnorms: null pointer");
    // one 16-byte load a run: every row starts on a 16-byte boundary
    const int64_t el = dtype == LMI_F16 ? 2 : 4;
    const bool vec = reinterpret_cast<uintptr_t>(rows) % 16 == 0 && (ld * el) % 16 == 0;
    const unsigned grid = (unsigned)std::min<int64_t>((m + kSqThreads / 64 - 1) / (kSqThreads / 64), kSqMaxGrid);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define LMI_SQ(T, V)                                                                                  \
    hipLaunchKernelGGL((row_sqnorms_kernel<T, V>), dim3(grid), dim3(kSqThreads), 0, s,               \
                       static_cast<const T*>(rows), m, ld, d, dst_rows, sqnorm)
    if (dtype == LMI_F16) {
        if (vec) LMI_SQ(__half, true); else LMI_SQ(__half, false);
    } else {
        if (vec) LMI_SQ(float, true); else LMI_SQ(float, false);
    }
#undef LMI_SQ
    LMI_LAUNCH_CHECK("row_sqnorms_kernel");
    return LMI_OK;
}
