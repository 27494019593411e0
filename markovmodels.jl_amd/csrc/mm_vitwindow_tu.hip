// mm_vitwindow_tu.hip -- translation unit of the windowed best paths (mm_kernel_vitwindow.hip): the tropical forward kernel from a
// carried start vector that keeps the back-pointer rows, the pre-emission maxima and the frames' maxima, and the trace kernel that
// follows the best path and the surviving set back to the convergence point and writes state_out at the commit frame.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_vitwindow.hip"

namespace mm {

size_t mm_vitwindow_lds_bytes(int S1p, int P1p) { return size_t(vitwindow_lds_floats(S1p, P1p)) * 4; }
bool mm_vitwindow_flags_global(int S1p) { return vitwindow_trace_lds_bytes(S1p, false) + 256 > MM_LDS_MAX; }

int mm_launch_vitwindow(int64_t B, int NW, int NI, bool bigv, size_t lds, int max_S1p, const RunParams &p, const VitWindowParams &wp,
                        hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    int rc;
    if (NI == 8)
        rc = bigv ? mm_launch(mm_vitwindow_fwd_kernel<8, true>, grid, block, lds, stream, p, wp)
                  : mm_launch(mm_vitwindow_fwd_kernel<8, false>, grid, block, lds, stream, p, wp);
    else if (NI == 0)
        rc = bigv ? mm_launch(mm_vitwindow_fwd_kernel<0, true>, grid, block, lds, stream, p, wp)
                  : mm_launch(mm_vitwindow_fwd_kernel<0, false>, grid, block, lds, stream, p, wp);
    else
        return mm_fail(MM_ERR_UNSUPPORTED, "windowed best paths: no instance for this geometry");
    if (rc) return rc;
    const bool gflags = mm_vitwindow_flags_global(max_S1p);
    if (gflags && !p.ws_big) return mm_fail(MM_ERR_UNSUPPORTED, "windowed best paths: FSM too large for the LDS and no global-memory vectors were allocated");
    if (gflags) return mm_launch(mm_vitwindow_trace_kernel<true>, grid, dim3(256), 0, stream, p, wp);
    return mm_launch(mm_vitwindow_trace_kernel<false>, grid, dim3(256), vitwindow_trace_lds_bytes(max_S1p, false), stream, p, wp);
}

}  // namespace mm
