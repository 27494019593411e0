// mm_arcs_tu.hip -- translation unit of the arc posteriors (mm_kernel_arcs.hip): the forward half of the item kernel, the
// backward kernel that accumulates the arcs, the scatter into the caller's entry order.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_arcs.hip"

namespace mm {

int mm_launch_arcs(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const ArcParams &ap, hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    const int rc = item_instance("arc posteriors", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_log_kernel<MODE_FB, NI_, 1, false, BIGV>, grid, block, lds, stream, p);
        return rc ? rc : mm_launch(mm_arc_kernel<NI_, BIGV>, grid, block, lds + MM_ARC_LDS_EXTRA, stream, p, ap);
    });
    return rc ? rc : mm_launch(mm_arc_scatter_kernel, dim3(unsigned(B), 4), dim3(256), 0, stream, p, ap);
}

}  // namespace mm
