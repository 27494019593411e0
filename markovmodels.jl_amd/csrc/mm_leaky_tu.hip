// mm_leaky_tu.hip -- translation unit of the leaky-HMM pdf posteriors (mm_kernel_leaky.hip): the forward kernel with the leak
// term in the row epilogue, the backward kernel that fixes beta up with eps c_n and writes gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_leaky.hip"

namespace mm {

size_t mm_leaky_lds_bytes(int S1p, int P1p) { return size_t(leaky_lds_plan(S1p, P1p).total) * 4; }

int mm_launch_leaky(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const LeakParams &lp, hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("leaky posteriors", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_leaky_fwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, lp);
        return rc ? rc : mm_launch(mm_leaky_bwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, lp);
    });
}

}  // namespace mm
