// mm_window_tu.hip -- translation unit of the fixed-lag smoothing posteriors (mm_kernel_window.hip): the forward kernel from a
// carried start vector with the alpha~ store, the backward kernel from an open or a closed end that writes gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_window.hip"

namespace mm {

size_t mm_window_lds_bytes(int S1p, int P1p) { return size_t(window_lds_plan(S1p, P1p).total) * 4; }

// the forward kernel alone: the first half of mm_launch_window, and of the segment entry (mm_segment_tu.hip), whose backward kernel
// is its own
int mm_launch_window_fwd(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    return item_instance("window posteriors", NI, bigv, [&](auto I) {
        return mm_launch(mm_window_fwd_kernel<decltype(I)::NI, decltype(I)::BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, wp);
    });
}

int mm_launch_window(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    const int rc = mm_launch_window_fwd(B, NW, NI, bigv, lds, p, wp, stream);
    if (rc) return rc;
    return item_instance("window posteriors", NI, bigv, [&](auto I) {
        return mm_launch(mm_window_bwd_kernel<decltype(I)::NI, decltype(I)::BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, wp);
    });
}

}  // namespace mm
