// mm_cost_tu.hip -- translation unit of the expected path cost (mm_kernel_cost.hip): the forward kernel that carries r beside
// alpha~, the backward kernel that carries s beside beta~ and writes risk, grad, gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_cost.hip"

namespace mm {

size_t mm_cost_lds_bytes(int S1p, int P1p) { return size_t(cost_lds_plan(S1p, P1p).total) * 4; }

int mm_launch_cost(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const CostParams &cp, hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("expected cost", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_cost_fwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, cp);
        return rc ? rc : mm_launch(mm_cost_bwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, cp);
    });
}

}  // namespace mm
