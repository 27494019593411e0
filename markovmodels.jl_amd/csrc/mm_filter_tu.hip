// mm_filter_tu.hip -- translation unit of the forward filtering posteriors (mm_kernel_filter.hip): one kernel, the forward step
// with the per-pdf sums of the finished frame and the carried state.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_filter.hip"

namespace mm {

size_t mm_filter_lds_bytes(int S1p, int P1p) { return size_t(filter_lds_plan(S1p, P1p).total) * 4; }

int mm_launch_filter(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const FilterParams &fp, hipStream_t stream) {
    return item_instance("filter posteriors", NI, bigv, [&](auto I) {
        return mm_launch(mm_filter_kernel<decltype(I)::NI, decltype(I)::BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, fp);
    });
}

}  // namespace mm
