// mm_window_tu.hip -- translation unit of the fixed-lag smoothing posteriors (mm_kernel_window.hip): the forward kernel from a
// carried start vector with the alpha~ store, the backward kernel from an open or a closed end that writes gamma and ttl.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_window.hip"

namespace mm {

size_t mm_window_lds_bytes(int S1p, int P1p) { return size_t(window_lds_plan(S1p, P1p).total) * 4; }

template <int NI, bool BIGV>
static int launch_window_ni(int64_t B, int NW, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    const int rc = mm_launch(mm_window_fwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, wp);
    return rc ? rc : mm_launch(mm_window_bwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, wp);
}

int mm_launch_window(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    if (NI == 8) return bigv ? launch_window_ni<8, true>(B, NW, lds, p, wp, stream) : launch_window_ni<8, false>(B, NW, lds, p, wp, stream);
    if (NI == 0 && bigv) return launch_window_ni<0, true>(B, NW, lds, p, wp, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "window posteriors: no instance for this geometry");
}

// (behind mm_launch_window: the kernels' instantiation order, and with it the translation unit's device code, stays as it was)
template <int NI, bool BIGV>
static int launch_window_fwd_ni(int64_t B, int NW, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    return mm_launch(mm_window_fwd_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, wp);
}

// the forward kernel alone, for the segment entry (mm_segment_tu.hip), whose backward kernel is its own
int mm_launch_window_fwd(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const WindowParams &wp, hipStream_t stream) {
    if (NI == 8) return bigv ? launch_window_fwd_ni<8, true>(B, NW, lds, p, wp, stream) : launch_window_fwd_ni<8, false>(B, NW, lds, p, wp, stream);
    if (NI == 0 && bigv) return launch_window_fwd_ni<0, true>(B, NW, lds, p, wp, stream);
    return mm_fail(MM_ERR_UNSUPPORTED, "window posteriors: no instance for this geometry");
}

}  // namespace mm
