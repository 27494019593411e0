// mm_scored_tu.hip -- translation unit of the posteriors with per-frame arc-class scores (mm_kernel_scored.hip): the scored forward
// kernel, then the backward kernel that writes gamma and a row of class sums per frame.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_scored.hip"

namespace mm {

int mm_launch_scored(int64_t B, int NW, int NI, bool bigv, size_t lds, size_t term_lds, const RunParams &p, const ScoredParams &sp,
                     hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("scored posteriors", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_scored_fwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, sp);
        return rc ? rc : mm_launch(mm_scored_bwd_kernel<NI_, BIGV>, grid, block, lds + term_lds, stream, p, sp);
    });
}

}  // namespace mm
