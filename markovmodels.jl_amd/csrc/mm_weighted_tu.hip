// mm_weighted_tu.hip -- translation unit of the posteriors with call-time arc weights (mm_kernel_weighted.hip): the prologue that
// builds the call's weight planes and descriptors, the forward half of the item kernel on them, the backward kernel that sums the
// arcs and writes gamma, the scatter into the caller's entry order.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_weighted.hip"

namespace mm {

size_t mm_weighted_lds_bytes(int S1p, int P1p) { return size_t(lds_plan(S1p, P1p, true).total + 2 * MM_MAX_WAVES + S1p) * 4; }

int mm_launch_weighted(int64_t B, int NW, int NI, bool bigv, size_t lds_fwd, size_t lds_bwd, const RunParams &p0, const WeightedParams &wp,
                       hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    RunParams p = p0;
    const int rc = item_instance("weighted posteriors", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        int rc = MM_OK;
        if (wp.utts_call) {
            rc = mm_launch(mm_weights_kernel, dim3(unsigned(B), 16), dim3(256), 0, stream, p, wp);
            if (rc) return rc;
            p.utts = wp.utts_call;
        }
        rc = mm_launch(mm_log_kernel<MODE_FB, NI_, 1, false, BIGV>, grid, block, lds_fwd, stream, p);
        return rc ? rc : mm_launch(mm_weighted_bwd_kernel<NI_, BIGV>, grid, block, lds_bwd, stream, p, wp);
    });
    if (rc || !(wp.counts || wp.init_counts || wp.ttl)) return rc;
    return mm_launch(mm_weighted_scatter_kernel, dim3(unsigned(B), 4), dim3(256), 0, stream, p, wp);
}

}  // namespace mm
