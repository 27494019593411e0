// mm_latsample_tu.hip -- translation unit of the lattice path sampling (mm_kernel_latsample.hip): the forward pass over the records of
// a lattice, one workgroup per utterance, and the Gumbel-max backward draw, one workgroup per utterance and 64 samples.
#define MM_SECONDARY_TU
#include <algorithm>

#include "mm_internal.h"
#include "mm_kernel_latsample.hip"

namespace mm {

// the forward pass's LDS (mm_latpost_fb_kernel's layout) and the sampler's (the key slots, a 64-bit mask per state)
static size_t fwd_lds_bytes(int S1p) { return MM_LP_HEAD + size_t(S1p) * (2 * sizeof(unsigned) + sizeof(unsigned long long)); }
static size_t draw_lds_bytes(int S1p) { return MM_LS_HEAD + size_t(S1p) * sizeof(unsigned long long); }
size_t mm_latsample_lds_bytes(int S1p) { return std::max(fwd_lds_bytes(S1p), draw_lds_bytes(S1p)); }

template <int NT>
static int launch_latsample(int64_t B, int max_S1p, const RunParams &p, const LatPostParams &lp, const LatSampleParams &ls, hipStream_t stream) {
    const int rc = mm_launch(mm_latsample_fwd_kernel<NT>, dim3(unsigned(B)), dim3(NT), fwd_lds_bytes(max_S1p), stream, p, lp);
    if (rc) return rc;
    const unsigned chunks = unsigned((ls.nsamples + MM_LS_CHUNK - 1) / MM_LS_CHUNK);
    return mm_launch(mm_latsample_kernel<NT>, dim3(unsigned(B), chunks), dim3(NT), draw_lds_bytes(max_S1p), stream, p, lp, ls);
}

int mm_launch_latsample(int64_t B, int nt, int max_S1p, const RunParams &p, const LatPostParams &lp, const LatSampleParams &ls, hipStream_t stream) {
    if (nt == 256) return launch_latsample<256>(B, max_S1p, p, lp, ls, stream);
    if (nt == 512) return launch_latsample<512>(B, max_S1p, p, lp, ls, stream);
    if (nt == 1024) return launch_latsample<1024>(B, max_S1p, p, lp, ls, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "mm_latticesample_f32: no instance of " + std::to_string(nt) + " threads");
}

}  // namespace mm
