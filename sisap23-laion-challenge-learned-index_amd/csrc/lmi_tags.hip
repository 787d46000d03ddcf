// Tag edits in place: lmi_index_edit_tags rewrites the tag words of chosen rows
// of a tagged index, tags[rows[i]] = (tags[rows[i]] & ~clear[i]) | set[i].
//
// One launch, one entry per thread in a grid-stride loop: a 4-byte gather, two
// bit operations, a 4-byte scatter.  The caller guarantees that the rows of a
// call are distinct, so no two threads touch one word and nothing is atomic.
// A row outside [0, n_rows) is skipped and LMI_STATUS_INTERNAL raised: every
// thread that meets one stores the same word (the status word as the kernel
// found it, with the bit set), so these plain stores do not race on a value.
#include <algorithm>

#include "lmi_common.hpp"

namespace lmi {
namespace {

constexpr int kEditBlock = 256;
constexpr int kEditMaxGrid = 4096;

__global__ __launch_bounds__(kEditBlock) void edit_tags_kernel(uint32_t* __restrict__ tags, int64_t n_rows,
                                                              const int64_t* __restrict__ rows,
                                                              const uint32_t* __restrict__ clear,
                                                              const uint32_t* __restrict__ set, int64_t n,
                                                              int32_t* __restrict__ status) {
    const int32_t status_in = *status;
    const int64_t step = (int64_t)gridDim.x * kEditBlock;
    for (int64_t i = (int64_t)blockIdx.x * kEditBlock + threadIdx.x; i < n; i += step) {
        const int64_t r = rows[i];
        if (r < 0 || r >= n_rows) {
            *status = status_in | LMI_STATUS_INTERNAL;
            continue;
        }
        tags[r] = (tags[r] & ~clear[i]) | set[i];
    }
}

}  // namespace
}  // namespace lmi

extern "C" int lmi_index_edit_tags(uint32_t* tags, int64_t n_rows, const int64_t* rows, const uint32_t* clear,
                                   const uint32_t* set, int64_t n, int32_t* status, void* stream) {
    using namespace lmi;
    LMI_CHECK_ARG(n >= 0 && n_rows >= 0, "lmi_index_edit_tags: n=%lld or n_rows=%lld < 0", (long long)n,
                  (long long)n_rows);
    if (n == 0) return LMI_OK;
    LMI_CHECK_ARG(tags && rows && clear && set && status, "lmi_index_edit_tags: null pointer");
    const int grid = (int)std::min<int64_t>((n + kEditBlock - 1) / kEditBlock, kEditMaxGrid);
    hipLaunchKernelGGL(edit_tags_kernel, dim3(grid), dim3(kEditBlock), 0, reinterpret_cast<hipStream_t>(stream), tags,
                       n_rows, rows, clear, set, n, status);
    LMI_LAUNCH_CHECK("edit_tags_kernel");
    return LMI_OK;
}
