// mm_leaky_tu.hip -- translation unit of the leaky-HMM pdf posteriors (mm_kernel_leaky.hip): the forward kernel with the leak
// term in the row epilogue, the backward kernel that fixes beta up with eps c_n and writes gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_leaky.hip"

namespace mm {

size_t mm_leaky_lds_bytes(int S1p, int P1p) { return size_t(leaky_lds_plan(S1p, P1p).total) * 4; }

template <int NI, bool BIGV>
static int launch_leaky_ni(int64_t B, int NW, size_t lds, const RunParams &p, const LeakParams &lp, hipStream_t stream) {
    const int rc = mm_launch(mm_leaky_fwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, lp);
    return rc ? rc : mm_launch(mm_leaky_bwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, lp);
}

int mm_launch_leaky(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const LeakParams &lp, hipStream_t stream) {
    if (NI == 8) return bigv ? launch_leaky_ni<8, true>(B, NW, lds, p, lp, stream) : launch_leaky_ni<8, false>(B, NW, lds, p, lp, stream);
    if (NI == 0 && bigv) return launch_leaky_ni<0, true>(B, NW, lds, p, lp, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "leaky posteriors: no instance for this geometry");
}

}  // namespace mm
