// mm_classpath_tu.hip -- translation unit of the best paths with arc classes (mm_kernel_classpath.hip): the tropical forward kernel
// that scores every arc by its class and keeps the back-pointer and the class rows, and the trace kernel that follows the best path
// from the phony final state and writes path and classes.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_classpath.hip"

namespace mm {

size_t mm_classpath_lds_bytes(int S1p, int P1p) { return size_t(classpath_lds_floats(S1p, P1p)) * 4; }

template <int MODE>
static int launch_classpath_fwd(int NI, bool bigv, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const RunParams &p, const ClassPathParams &cp) {
    if (NI == 8)
        return bigv ? mm_launch(mm_classpath_fwd_kernel<8, true, MODE>, grid, block, lds, stream, p, cp)
                    : mm_launch(mm_classpath_fwd_kernel<8, false, MODE>, grid, block, lds, stream, p, cp);
    if (NI == 0)
        return bigv ? mm_launch(mm_classpath_fwd_kernel<0, true, MODE>, grid, block, lds, stream, p, cp)
                    : mm_launch(mm_classpath_fwd_kernel<0, false, MODE>, grid, block, lds, stream, p, cp);
    return mm_fail(MM_ERR_UNSUPPORTED, "best paths with arc classes: no instance for this geometry");
}

int mm_launch_classpath(int64_t B, int NW, int NI, bool bigv, int mode, size_t lds, const RunParams &p, const ClassPathParams &cp,
                        hipStream_t stream) {
    const dim3 grid{unsigned(B)}, block{unsigned(64 * NW)};
    const int rc = mode == 2   ? launch_classpath_fwd<2>(NI, bigv, grid, block, lds, stream, p, cp)
                   : mode == 1 ? launch_classpath_fwd<1>(NI, bigv, grid, block, lds, stream, p, cp)
                               : launch_classpath_fwd<0>(NI, bigv, grid, block, lds, stream, p, cp);
    return rc ? rc : mm_launch(mm_classpath_trace_kernel, grid, dim3(256), 0, stream, p, cp);
}

}  // namespace mm
