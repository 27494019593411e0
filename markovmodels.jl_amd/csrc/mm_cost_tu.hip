// mm_cost_tu.hip -- translation unit of the expected path cost (mm_kernel_cost.hip): the forward kernel that carries r beside
// alpha~, the backward kernel that carries s beside beta~ and writes risk, grad, gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_cost.hip"

namespace mm {

size_t mm_cost_lds_bytes(int S1p, int P1p) { return size_t(cost_lds_plan(S1p, P1p).total) * 4; }

template <int NI, bool BIGV>
static int launch_cost_ni(int64_t B, int NW, size_t lds, const RunParams &p, const CostParams &cp, hipStream_t stream) {
    const int rc = mm_launch(mm_cost_fwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, cp);
    return rc ? rc : mm_launch(mm_cost_bwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, cp);
}

int mm_launch_cost(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const CostParams &cp, hipStream_t stream) {
    if (NI == 8) return bigv ? launch_cost_ni<8, true>(B, NW, lds, p, cp, stream) : launch_cost_ni<8, false>(B, NW, lds, p, cp, stream);
    if (NI == 0 && bigv) return launch_cost_ni<0, true>(B, NW, lds, p, cp, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "expected cost: no instance for this geometry");
}

}  // namespace mm
