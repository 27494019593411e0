// mm_entropy_tu.hip -- translation unit of the posterior path entropy (mm_kernel_entropy.hip): the forward kernel that carries
// Hf beside alpha~ and writes entropy and ttl, the backward kernel that carries Hb beside beta~ and writes grad and gamma.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_entropy.hip"

namespace mm {

size_t mm_entropy_lds_bytes(int S1p, int P1p) { return size_t(entropy_lds_plan(S1p, P1p).total) * 4; }

int mm_launch_entropy(int64_t B, int NW, int NI, bool bigv, size_t lds, bool backward, const RunParams &p, const EntropyParams &ep,
                      hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    return item_instance("path entropy", NI, bigv, [&](auto I) {
        constexpr int NI_ = decltype(I)::NI;
        constexpr bool BIGV = decltype(I)::BIGV;
        const int rc = mm_launch(mm_entropy_fwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, ep);
        return rc || !backward ? rc : mm_launch(mm_entropy_bwd_kernel<NI_, BIGV>, grid, block, lds, stream, p, ep);
    });
}

}  // namespace mm
