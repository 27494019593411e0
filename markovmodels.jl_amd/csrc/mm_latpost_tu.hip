// mm_latpost_tu.hip -- translation unit of the lattice posteriors (mm_kernel_latpost.hip): the forward-backward over the records of
// a lattice, one workgroup per utterance, and the per-pdf sums of its posteriors, one workgroup per utterance and frame.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_latpost.hip"

namespace mm {

size_t mm_latpost_lds_bytes(int S1p) { return MM_LP_HEAD + size_t(S1p) * (2 * sizeof(unsigned) + sizeof(unsigned long long)); }
size_t mm_latpost_gamma_lds_bytes(int P1) { return size_t(P1) * sizeof(unsigned long long); }

template <int NT>
static int launch_latpost(int64_t B, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, hipStream_t stream) {
    const int rc = mm_launch(mm_latpost_fb_kernel<NT>, dim3(unsigned(B)), dim3(NT), mm_latpost_lds_bytes(max_S1p), stream, p, lp);
    if (rc || !lp.gamma) return rc;
    return mm_launch(mm_latpost_gamma_kernel<MM_LATPOST_GAMMA_NT>, dim3(unsigned(B * int64_t(p.N))), dim3(MM_LATPOST_GAMMA_NT), mm_latpost_gamma_lds_bytes(max_P1),
                     stream, p, lp);
}

int mm_launch_latpost(int64_t B, int nt, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, hipStream_t stream) {
    if (nt == 256) return launch_latpost<256>(B, max_S1p, max_P1, p, lp, stream);
    if (nt == 512) return launch_latpost<512>(B, max_S1p, max_P1, p, lp, stream);
    if (nt == 1024) return launch_latpost<1024>(B, max_S1p, max_P1, p, lp, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "mm_latticeposteriors_f32: no instance of " + std::to_string(nt) + " threads");
}

}  // namespace mm
