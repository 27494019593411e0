// mm_classcost_tu.hip -- translation unit of the expected arc-class cost (mm_kernel_classcost.hip): the forward kernel that carries r
// beside alpha~, the backward kernel that carries s beside beta~ and writes risk, grad, gamma and ttl, every arc with its class's cost.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_classcost.hip"

namespace mm {

int mm_launch_classcost(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const ClassCostParams &cp, hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("expected class cost", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_classcost_fwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, cp);
        return rc ? rc : mm_launch(mm_classcost_bwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, cp);
    });
}

}  // namespace mm
