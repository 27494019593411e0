// mm_latcost_tu.hip -- translation unit of the lattice expected cost (mm_kernel_latpost.hip in its instance with costs): the
// forward-backward over the records of a lattice with the cost recursions beside it, one workgroup per utterance, and the per-pdf
// sums of diff and of the posteriors, one workgroup per utterance and frame.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_latpost.hip"

namespace mm {

size_t mm_latcost_lds_bytes(int S1p) { return MM_LC_HEAD + size_t(S1p) * (2 * sizeof(unsigned) + 2 * sizeof(unsigned long long) + sizeof(float)); }
size_t mm_latcost_grad_lds_bytes(int P1) { return 16 + size_t(P1) * 2 * sizeof(unsigned long long); }

template <int NT>
static int launch_latcost(int64_t B, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, const LatCostParams &lc, hipStream_t stream) {
    const int rc = mm_launch(mm_latcost_fb_kernel<NT>, dim3(unsigned(B)), dim3(NT), mm_latcost_lds_bytes(max_S1p), stream, p, lp, lc);
    if (rc || (!lp.gamma && !lc.grad)) return rc;
    return mm_launch(mm_latcost_grad_kernel<MM_LATPOST_GAMMA_NT>, dim3(unsigned(B * int64_t(p.N))), dim3(MM_LATPOST_GAMMA_NT), mm_latcost_grad_lds_bytes(max_P1),
                     stream, p, lp, lc);
}

int mm_launch_latcost(int64_t B, int nt, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, const LatCostParams &lc, hipStream_t stream) {
    if (nt == 256) return launch_latcost<256>(B, max_S1p, max_P1, p, lp, lc, stream);
    if (nt == 512) return launch_latcost<512>(B, max_S1p, max_P1, p, lp, lc, stream);
    if (nt == 1024) return launch_latcost<1024>(B, max_S1p, max_P1, p, lp, lc, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "mm_latticecost_f32: no instance of " + std::to_string(nt) + " threads");
}

}  // namespace mm
