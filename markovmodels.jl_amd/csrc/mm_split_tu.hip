// mm_split_tu.hip -- translation unit of the SPLIT pair kernels: pair_agent (mm_kernel_pairs.hip) with teams of H = 2 or 4
// workgroups per utterance pair and direction, for FSMs beyond the registers / LDS of one compute unit (the reference's
// WSJ denominator graph, misc/benchmark/den_fsm_wsj.txt; the reference itself has no size limit, src/linalg.jl:170-181).
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_pairs.hip"

namespace mm {

// (teams of 2: a vector of 24 KB, up to 3070 states; teams of 4: 32 KB, up to 4094 states, a quarter of the rows each; the
// geometry of a team: mm_split_rs, mm_split_rsh, mm_split_ka; its place in the grid: team_pos, team_grid)
// One launch per phase: the teams of the forward agents are the first half of the grid, those of the backward agents the
// second (mm_pairs_tu.hip).
template <int NJ, int PHASE, int H>
__global__ void __launch_bounds__(1024) mm_fbs_kernel(RunParams p) {
    const int half = (int)gridDim.x / 2, dir = (int)blockIdx.x >= half;
    const TeamPos t = team_pos<H>((int)blockIdx.x - (dir ? half : 0));
    if (t.idx >= (p.B + 1) / 2) return;
    if ((p.x_sleep & 0x400) && t.hset == 1) return;  // (test aid, MM_SPLIT_SLEEP bit 0x400: a team mate that never shows up)
    pair_agent<mm_split_ka(H), mm_split_rs(H), PHASE, -1, NJ, H, mm_split_rsh(H)>(p, t.idx, t.hset, dir);
}
template <int NJ, int PHASE, int H>
static int launch_split_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbs_kernel<NJ, PHASE, H>, "split kernel", pair_lds_bytes(mm_split_rs(H), PHASE, pl.slotrows, mm_split_rsh(H), pair_pc(NJ)),
                             2 * team_grid(pair_count(pl), H), MM_SPLIT_NWC + 2, st, p);
}
template <int NJ, int H>
static int launch_split_nj(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_split_phase<NJ, 0, H>, launch_split_phase<NJ, 1, H>, mm_pair_finish_kernel, pl, p, s0);
}
int mm_launch_split(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    if (pl.pair_ka > mm_split_ka(pl.H)) return MM_ERR_UNSUPPORTED;
    const int nj = mm_pair_nj(pl.max_P1, pl.H);
    if (nj == 0) return MM_ERR_UNSUPPORTED;
    if (pl.H == 8) return nj == 2 ? launch_split_nj<2, 8>(pl, p, s0) : (nj == 4 ? launch_split_nj<4, 8>(pl, p, s0) : launch_split_nj<5, 8>(pl, p, s0));
    if (pl.H == 4) return nj == 2 ? launch_split_nj<2, 4>(pl, p, s0) : (nj == 4 ? launch_split_nj<4, 4>(pl, p, s0) : launch_split_nj<8, 4>(pl, p, s0));
    if (pl.H != 2) return mm_fail(MM_ERR_UNSUPPORTED, "split kernel: teams of 2, 4 or 8");
    return nj == 2 ? launch_split_nj<2, 2>(pl, p, s0) : (nj == 4 ? launch_split_nj<4, 2>(pl, p, s0) : launch_split_nj<8, 2>(pl, p, s0));
}
// ---- alpha-recursion / beta-recursion export on the team kernels (mm_pairs_tu.hip, mm_fbx_kernel): phase A of ONE direction over all
// N + 1 frames by teams of H workgroups, then mm_pair_export_kernel.  Teams of 2 and 4, up to 128 pdfs (the reference's WSJ denominator).
template <int NJ, int H>
__global__ void __launch_bounds__(1024) mm_fbsx_kernel(RunParams p, int dir) {
    const TeamPos t = team_pos<H>((int)blockIdx.x);
    if (t.idx >= (p.B + 1) / 2) return;
    pair_agent<mm_split_ka(H), mm_split_rs(H), 0, -1, NJ, H, mm_split_rsh(H), false, true>(p, t.idx, t.hset, dir);
}
template <int NJ, int H>
static int launch_split_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t st) {
    const int rc = pair_launch_phase(mm_fbsx_kernel<NJ, H>, "split kernel", pair_lds_bytes(mm_split_rs(H), 0, pl.slotrows, mm_split_rsh(H), pair_pc(NJ)),
                                     team_grid(pair_count(pl), H), MM_SPLIT_NWC + 2, st, p, dir);
    return rc ? rc : pair_launch_export_layout(pl, p, dir, st);
}
bool mm_split_export_fits(const PairLaunch &pl) {
    return (pl.H == 2 || pl.H == 4) && pl.pair_ka <= mm_split_ka(pl.H) && mm_pair_nj(pl.max_P1, pl.H) == 2;
}
int mm_launch_split_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t s0) {
    if (!mm_split_export_fits(pl)) return MM_ERR_UNSUPPORTED;
    return pl.H == 4 ? launch_split_export<2, 4>(pl, p, dir, s0) : launch_split_export<2, 2>(pl, p, dir, s0);
}
size_t mm_split_lds_bytes(int H, int phase, int nslotrows, int max_P1) {
    const int nj = mm_pair_nj(max_P1, H);
    return nj ? pair_lds_bytes(mm_split_rs(H), phase, nslotrows, mm_split_rsh(H), pair_pc(nj)) : 0;
}

}  // namespace mm
