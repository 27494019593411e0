// mm_segment_tu.hip -- translation unit of the segment posteriors (mm_kernel_segment.hip): the window entry's forward kernel from a
// carried start vector (launched through mm_window_tu.hip, where it lives), then the backward kernel from an open, a closed or a
// carried end that writes gamma, ttl and the end vector of the segment before.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_segment.hip"

namespace mm {

int mm_launch_segment(int64_t B, int NW, int NI, bool bigv, size_t lds, const RunParams &p, const SegmentParams &sp, hipStream_t stream) {
    return item_instance("segment posteriors", NI, bigv, [&](auto I) {
        // the forward half: no commit frame, no state_out; its total in ws_c[0] is the open one (end_mode 0) or the closed one (the
        // backward kernel takes a carried end's total itself)
        WindowParams wp{};
        wp.state_in = sp.state_in;
        wp.closed = sp.end_mode;
        const int rc = mm_launch_window_fwd(B, NW, NI, bigv, lds, p, wp, stream);
        return rc ? rc : mm_launch(mm_segment_bwd_kernel<decltype(I)::NI, decltype(I)::BIGV>, dim3(unsigned(B)), dim3(64 * NW), lds, stream, p, sp);
    });
}

}  // namespace mm
