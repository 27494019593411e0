// mm_lattice_tu.hip -- translation unit of the beam-pruned best-path lattices (mm_kernel_lattice.hip): the pass over the arcs that
// counts and writes the entries within the beam, and the scan of the counts between its two modes.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_lattice.hip"

namespace mm {

size_t mm_lattice_lds_bytes(int S1p) { return MM_LAT_HEAD + size_t(2) * size_t(S1p) * sizeof(float); }

template <bool WRITE>
static int launch_prune(bool global, size_t lds, dim3 grid, hipStream_t stream, const RunParams &p, const LatticeParams &lp) {
    return global ? mm_launch(mm_lattice_prune_kernel<false, WRITE>, grid, dim3(MM_LAT_NT), lds, stream, p, lp)
                  : mm_launch(mm_lattice_prune_kernel<true, WRITE>, grid, dim3(MM_LAT_NT), lds, stream, p, lp);
}

int mm_launch_lattice(int64_t B, bool global, int max_S1p, const RunParams &p, const LatticeParams &lp, long long *total, hipStream_t stream) {
    const dim3 grid{unsigned(B * int64_t(p.N))};
    const size_t lds = global ? size_t(MM_LAT_HEAD) : mm_lattice_lds_bytes(max_S1p);
    int rc = launch_prune<false>(global, lds, grid, stream, p, lp);
    if (rc) return rc;
    rc = mm_launch(mm_lattice_scan_kernel, dim3(1), dim3(MM_LAT_NT), 0, stream, (const int *)lp.counts, lp.csb, int(B), p.N, lp.offs, total);
    if (rc || !lp.arc) return rc;
    return launch_prune<true>(global, lds, grid, stream, p, lp);
}

}  // namespace mm
