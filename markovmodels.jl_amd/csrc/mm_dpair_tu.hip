// mm_dpair_tu.hip -- translation unit of the float64 exact pair kernels (mm_kernel_dpair.hip): their instances and launches.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_dpair.hip"

namespace mm {

// One utterance per workgroup; one launch per phase: the forward agents are the first B workgroups (by rank in the
// longest-first order), the backward agents the second B (mm_pairs_tu.hip).
// (NJ: 64-lane passes over the pdfs in the service wave, 2 for P + 1 <= 128, else 4)
template <int NJ, int PHASE>
__global__ void __launch_bounds__(1024) mm_fbd_kernel(RunParams p) {
    const int dir = (int)blockIdx.x >= p.B;
    dpair_agent<MM_PAIR_KA, MM_ROW_RS, PHASE, NJ>(p, (int)blockIdx.x - (dir ? p.B : 0), dir);
}
template <int NJ, int PHASE>
static int launch_dpair_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbd_kernel<NJ, PHASE>, "exact pair kernel", pair_lds_bytes(MM_ROW_RS, PHASE, pl.slotrows, 0, pair_pc(NJ)),
                             2 * unsigned(pl.B), pl.nwc + 1, st, p);
}
template <int NJ>
static int launch_dpairs_nj(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_dpair_phase<NJ, 0>, launch_dpair_phase<NJ, 1>, mm_dpair_finish_kernel, pl, p, s0);
}
// ---- teams of H workgroups per utterance and direction (the split kernels' graphs: mm_split_tu.hip)
template <int NJ, int PHASE, int H>
__global__ void __launch_bounds__(1024) mm_fbds_kernel(RunParams p) {
    const int half = (int)gridDim.x / 2, dir = (int)blockIdx.x >= half;
    const TeamPos t = team_pos<H>((int)blockIdx.x - (dir ? half : 0));
    if (t.idx >= p.B) return;
    if ((p.x_sleep & 0x400) && t.hset == 1) return;  // (test aid: a team mate that never shows up)
    dpair_agent<mm_split_ka(H), mm_split_rs(H), PHASE, NJ, H, mm_split_rsh(H)>(p, t.idx, dir, t.hset);
}
template <int NJ, int PHASE, int H>
static int launch_dsplit_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbds_kernel<NJ, PHASE, H>, "exact split kernel",
                             pair_lds_bytes(mm_split_rs(H), PHASE, pl.slotrows, mm_split_rsh(H), pair_pc(NJ)), 2 * team_grid(unsigned(pl.B), H),
                             MM_SPLIT_NWC + 2, st, p);
}
template <int NJ, int H>
static int launch_dsplit_nj(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_dsplit_phase<NJ, 0, H>, launch_dsplit_phase<NJ, 1, H>, mm_dpair_finish_kernel, pl, p, s0);
}
int mm_launch_dpairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    const int nj = mm_pair_nj(pl.max_P1, pl.H);
    if (nj == 0) return MM_ERR_UNSUPPORTED;
    if (pl.H == 1) {
        if (pl.pair_ka > MM_PAIR_KA) return MM_ERR_UNSUPPORTED;
        return nj == 2 ? launch_dpairs_nj<2>(pl, p, s0) : (nj == 4 ? launch_dpairs_nj<4>(pl, p, s0) : launch_dpairs_nj<8>(pl, p, s0));
    }
    if (pl.pair_ka > mm_split_ka(pl.H)) return MM_ERR_UNSUPPORTED;
    if (pl.H == 8) return nj == 2 ? launch_dsplit_nj<2, 8>(pl, p, s0) : (nj == 4 ? launch_dsplit_nj<4, 8>(pl, p, s0) : launch_dsplit_nj<5, 8>(pl, p, s0));
    if (pl.H == 4) return nj == 2 ? launch_dsplit_nj<2, 4>(pl, p, s0) : (nj == 4 ? launch_dsplit_nj<4, 4>(pl, p, s0) : launch_dsplit_nj<8, 4>(pl, p, s0));
    if (pl.H != 2) return mm_fail(MM_ERR_UNSUPPORTED, "exact split kernel: teams of 2, 4 or 8");
    return nj == 2 ? launch_dsplit_nj<2, 2>(pl, p, s0) : (nj == 4 ? launch_dsplit_nj<4, 2>(pl, p, s0) : launch_dsplit_nj<8, 2>(pl, p, s0));
}

}  // namespace mm
