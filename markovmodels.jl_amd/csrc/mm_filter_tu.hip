// mm_filter_tu.hip -- translation unit of the forward filtering posteriors (mm_kernel_filter.hip): one kernel, the forward step
// with the per-pdf sums of the finished frame and the carried state.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_filter.hip"

namespace mm {

size_t mm_filter_lds_bytes(int S1p, int P1p) { return size_t(filter_lds_plan(S1p, P1p).total) * 4; }

int mm_launch_filter(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const FilterParams &fp, hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    if (NI == 8 && !bigv) return mm_launch(mm_filter_kernel<8, false>, grid, block, lds, stream, p, fp);
    if (NI == 8) return mm_launch(mm_filter_kernel<8, true>, grid, block, lds, stream, p, fp);
    if (NI == 0 && bigv) return mm_launch(mm_filter_kernel<0, true>, grid, block, lds, stream, p, fp);
    return mm_fail(MM_ERR_UNSUPPORTED, "filter posteriors: no instance for this geometry");
}

}  // namespace mm
