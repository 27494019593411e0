// mm_wpair_tu.hip -- translation unit of the wide-exponent pair kernels (mm_kernel_wpair.hip): their instances and launches.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_wpair.hip"

namespace mm {

// Two utterances per workgroup like mm_fbp_kernel, one grid per phase: the forward agents are the first half of the grid, the
// backward agents the second.  (NJ: 64-lane passes over the pdfs in the service wave, 2 for P + 1 <= 128, 4 up to 250)
template <int NJ, int PHASE>
__global__ void __launch_bounds__(1024) mm_fbw_kernel(RunParams p) {
    const int npairs = (p.B + 1) / 2, dir = (int)blockIdx.x >= npairs;
    wpair_agent<MM_PAIR_KA, MM_ROW_RS, PHASE, NJ>(p, (int)blockIdx.x - (dir ? npairs : 0), dir);
}
template <int NJ, int PHASE>
static int launch_wpair_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbw_kernel<NJ, PHASE>, "wide pair kernel", wpair_lds_bytes(MM_ROW_RS, PHASE, pl.slotrows, pair_pc(NJ)),
                             2 * pair_count(pl), pl.nwc + 1, st, p);
}
template <int NJ>
static int launch_wpairs_nj(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_wpair_phase<NJ, 0>, launch_wpair_phase<NJ, 1>, mm_dpair_finish_kernel, pl, p, s0);
}
// ---- teams of H workgroups per utterance pair and direction (the split kernels' graphs: mm_split_tu.hip)
template <int NJ, int PHASE, int H>
__global__ void __launch_bounds__(1024) mm_fbws_kernel(RunParams p) {
    const int half = (int)gridDim.x / 2, dir = (int)blockIdx.x >= half;
    const TeamPos t = team_pos<H>((int)blockIdx.x - (dir ? half : 0));
    if (t.idx >= (p.B + 1) / 2) return;
    if ((p.x_sleep & 0x400) && t.hset == 1) return;  // (test aid: a team mate that never shows up)
    wpair_agent<mm_split_ka(H), mm_split_rs(H), PHASE, NJ, H, mm_split_rsh(H)>(p, t.idx, dir, t.hset);
}
template <int NJ, int PHASE, int H>
static int launch_wsplit_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbws_kernel<NJ, PHASE, H>, "wide split kernel",
                             wpair_lds_bytes(mm_split_rs(H), PHASE, pl.slotrows, wpair_pc(NJ, H), mm_split_rsh(H)),
                             2 * team_grid(pair_count(pl), H), MM_SPLIT_NWC + 2, st, p);
}
template <int NJ, int H>
static int launch_wsplit_nj(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_wsplit_phase<NJ, 0, H>, launch_wsplit_phase<NJ, 1, H>, mm_dpair_finish_kernel, pl, p, s0);
}
// does the batch fit the wide pair kernels?  (up to 250 pdfs; the LDS of phase B with per-pdf sums of two doubles; one workgroup or a team of 2)
bool mm_wpair_fits(const PairLaunch &pl) {
    if (pl.max_P1 > 250) return false;
    const int nj = mm_pair_nj(pl.max_P1);
    if (pl.H == 1) return pl.pair_ka <= MM_PAIR_KA && wpair_lds_bytes(MM_ROW_RS, 1, pl.slotrows, pair_pc(nj)) <= MM_LDS_MAX;
    if (pl.H != 2) return false;  // (teams of 4: the kernels compile with 30 .. 45 spilled registers -- the float64 team kernels keep those graphs)
    return pl.pair_ka <= mm_split_ka(pl.H) && wpair_lds_bytes(mm_split_rs(pl.H), 1, pl.slotrows, wpair_pc(nj, pl.H), mm_split_rsh(pl.H)) <= MM_LDS_MAX;
}
int mm_launch_wpairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    if (!mm_wpair_fits(pl)) return MM_ERR_UNSUPPORTED;
    const bool two = pl.max_P1 <= 128;
    if (pl.H == 1) return two ? launch_wpairs_nj<2>(pl, p, s0) : launch_wpairs_nj<4>(pl, p, s0);
    return two ? launch_wsplit_nj<2, 2>(pl, p, s0) : launch_wsplit_nj<4, 2>(pl, p, s0);
}

}  // namespace mm
