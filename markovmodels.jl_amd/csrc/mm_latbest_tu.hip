// mm_latbest_tu.hip -- translation unit of the lattice best paths (mm_kernel_latbest.hip): the tropical forward-backward over the
// records of a lattice with the trace of the best path, one workgroup per utterance.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_latbest.hip"

namespace mm {

size_t mm_latbest_lds_bytes(int S1p) { return MM_LB_HEAD + size_t(S1p) * 3 * sizeof(unsigned); }

int mm_launch_latbest(int64_t B, int nt, int max_S1p, const RunParams &p, const LatPostParams &lp, const LatBestParams &lb, hipStream_t stream) {
    const size_t lds = mm_latbest_lds_bytes(max_S1p);
    if (nt == 256) return mm_launch(mm_latbest_kernel<256>, dim3(unsigned(B)), dim3(256), lds, stream, p, lp, lb);
    if (nt == 512) return mm_launch(mm_latbest_kernel<512>, dim3(unsigned(B)), dim3(512), lds, stream, p, lp, lb);
    if (nt == 1024) return mm_launch(mm_latbest_kernel<1024>, dim3(unsigned(B)), dim3(1024), lds, stream, p, lp, lb);
    return mm_fail(MM_ERR_UNSUPPORTED, "mm_latticebest_f32: no instance of " + std::to_string(nt) + " threads");
}

}  // namespace mm
