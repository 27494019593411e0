// mm_arcclass_tu.hip -- translation unit of the per-frame arc-class posteriors (mm_kernel_arcclass.hip): the forward half of the
// item kernel, then the backward kernel that writes a row of class sums per frame.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_arcclass.hip"

namespace mm {

int mm_launch_arcclass(int64_t B, int NW, int NI, bool bigv, size_t lds, size_t term_lds, const RunParams &p, const ArcClassParams &cp,
                       hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("arc-class posteriors", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_log_kernel<MODE_FB, NI_, 1, false, BIGV>, grid, block, lds, stream, p);
        return rc ? rc : mm_launch(mm_arcclass_kernel<NI_, BIGV>, grid, block, lds + MM_ARC_LDS_EXTRA + term_lds, stream, p, cp);
    });
}

}  // namespace mm
