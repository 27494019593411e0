// mm_entropy_tu.hip -- translation unit of the posterior path entropy (mm_kernel_entropy.hip): the forward kernel that carries
// Hf beside alpha~ and writes entropy and ttl, the backward kernel that carries Hb beside beta~ and writes grad and gamma.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_entropy.hip"

namespace mm {

size_t mm_entropy_lds_bytes(int S1p, int P1p) { return size_t(entropy_lds_plan(S1p, P1p).total) * 4; }

template <int NI, bool BIGV>
static int launch_entropy_ni(int64_t B, int NW, size_t lds, bool backward, const RunParams &p, const EntropyParams &ep, hipStream_t stream) {
    const int rc = mm_launch(mm_entropy_fwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, ep);
    return rc || !backward ? rc : mm_launch(mm_entropy_bwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, ep);
}

int mm_launch_entropy(int64_t B, int NW, int NI, bool bigv, size_t lds, bool backward, const RunParams &p, const EntropyParams &ep,
                      hipStream_t stream) {
    if (NI == 8)
        return bigv ? launch_entropy_ni<8, true>(B, NW, lds, backward, p, ep, stream) : launch_entropy_ni<8, false>(B, NW, lds, backward, p, ep, stream);
    if (NI == 0 && bigv) return launch_entropy_ni<0, true>(B, NW, lds, backward, p, ep, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "path entropy: no instance for this geometry");
}

}  // namespace mm
