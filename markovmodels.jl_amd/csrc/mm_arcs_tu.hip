// mm_arcs_tu.hip -- translation unit of the arc posteriors (mm_kernel_arcs.hip): the forward half of the item kernel, the
// backward kernel that accumulates the arcs, the scatter into the caller's entry order.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_arcs.hip"

namespace mm {

template <int NI, bool BIGV>
static int launch_arcs_ni(int64_t B, int NW, size_t lds, const RunParams &p, const ArcParams &ap, hipStream_t stream) {
    const int rc = mm_launch(mm_log_kernel<MODE_FB, NI, 1, false, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p);
    return rc ? rc : mm_launch(mm_arc_kernel<NI, BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds + MM_ARC_LDS_EXTRA, stream, p, ap);
}

int mm_launch_arcs(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const ArcParams &ap, hipStream_t stream) {
    int rc;
    if (NI == 8) rc = bigv ? launch_arcs_ni<8, true>(B, NW, lds, p, ap, stream) : launch_arcs_ni<8, false>(B, NW, lds, p, ap, stream);
    else if (NI == 0 && bigv) rc = launch_arcs_ni<0, true>(B, NW, lds, p, ap, stream);
    else return mm_fail(MM_ERR_UNSUPPORTED, "arc posteriors: no instance for this geometry");
    return rc ? rc : mm_launch(mm_arc_scatter_kernel, dim3(unsigned(B), 4), dim3(256), 0, stream, p, ap);
}

}  // namespace mm
