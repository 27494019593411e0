// mm_pairs_tu.hip -- translation unit of the pair kernels (mm_kernel_pairs.hip): their instances and launches.
#define MM_SECONDARY_TU
#include "mm_internal.h"
#include "mm_kernel_pairs.hip"

namespace mm {

// The pair kernels (mm_kernel_pairs.hip): phase A, then phase B, each ONE launch that holds the forward agents (the first
// half of the grid) and the backward agents (the second half) of all pairs -- the two agents of a pair run at the same time
// because they are workgroups of one grid, not because two streams happen to share no hardware queue.  (Rounds 2 and 3
// launched the two directions as two kernels on a pair of library streams, forked from and joined into the caller's stream
// by events: every fork, join and cross-stream wait cost 10-25 us of idle device -- ~80 us of a 2.9 ms call, rocprofv3
// timeline --, needed a pool of stream pairs probed for real concurrency, and a special case inside stream captures.)
// (NJ: 64-lane passes over the pdfs in the service wave, 2 for P + 1 <= 128, 4 up to 250, 8 up to 506 -- the last with per-pdf
// arrays of twice the size and a partner-row ring of two vectors instead of three: PairLay)
// (SMALL: graphs of up to 127 states, whose service wave does a sixteenth of the copying and scanning)
template <int NJ, int PHASE, bool SMALL>
__global__ void __launch_bounds__(1024) mm_fbp_kernel(RunParams p) {
    const int npairs = (p.B + 1) / 2, dir = (int)blockIdx.x >= npairs;
    pair_agent<MM_PAIR_KA, MM_ROW_RS, PHASE, -1, NJ, 1, 2 * MM_ROW_RS, SMALL>(p, (int)blockIdx.x - (dir ? npairs : 0), 0, dir);
}
template <int NJ, int PHASE, bool SMALL>
static int launch_pair_phase(const PairLaunch &pl, const RunParams &p, hipStream_t st) {
    return pair_launch_phase(mm_fbp_kernel<NJ, PHASE, SMALL>, "pair kernel", pair_lds_bytes(MM_ROW_RS, PHASE, pl.slotrows, 0, pair_pc(NJ)),
                             2 * pair_count(pl), pl.nwc + 1, st, p);
}
template <int NJ, bool SMALL>
static int launch_pairs_ka(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    return pair_launch_phases(launch_pair_phase<NJ, 0, SMALL>, launch_pair_phase<NJ, 1, SMALL>, mm_pair_finish_kernel, pl, p, s0);
}
int mm_launch_pairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0) {
    if (pl.pair_ka > MM_PAIR_KA) return MM_ERR_UNSUPPORTED;
    if (pl.max_P1 <= 128) return pair_small_instances(pl) ? launch_pairs_ka<2, true>(pl, p, s0) : launch_pairs_ka<2, false>(pl, p, s0);
    if (pl.max_P1 <= 250) return launch_pairs_ka<4, false>(pl, p, s0);
    if (pl.max_P1 > MM_PAIR_P1MAX) return MM_ERR_UNSUPPORTED;
    return launch_pairs_ka<8, false>(pl, p, s0);
}
// ---- alpha-recursion / beta-recursion export on the pair kernels (src/inference.jl:62-74, 99-110): phase A of ONE direction over all
// N + 1 frames (pair_agent, XPT), then mm_pair_export_kernel -- instead of the item kernel's one workgroup per utterance with the
// vectors in the log domain (config 3: 26 ms).  The instances of the linear finishes only (up to 250 pdfs).
template <int NJ, bool SMALL>
__global__ void __launch_bounds__(1024) mm_fbx_kernel(RunParams p, int dir) {
    pair_agent<MM_PAIR_KA, MM_ROW_RS, 0, -1, NJ, 1, 2 * MM_ROW_RS, SMALL, true>(p, (int)blockIdx.x, 0, dir);
}
template <int NJ, bool SMALL>
static int launch_pair_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t st) {
    const int rc = pair_launch_phase(mm_fbx_kernel<NJ, SMALL>, "pair kernel", pair_lds_bytes(MM_ROW_RS, 0, pl.slotrows, 0, pair_pc(NJ)), pair_count(pl),
                                     pl.nwc + 1, st, p, dir);
    return rc ? rc : pair_launch_export_layout(pl, p, dir, st);
}
bool mm_pair_export_fits(const PairLaunch &pl) { return pl.H == 1 && pl.pair_ka <= MM_PAIR_KA && pl.max_P1 <= 250; }
int mm_launch_pair_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t s0) {
    if (!mm_pair_export_fits(pl)) return MM_ERR_UNSUPPORTED;
    if (pl.max_P1 <= 128) return pair_small_instances(pl) ? launch_pair_export<2, true>(pl, p, dir, s0) : launch_pair_export<2, false>(pl, p, dir, s0);
    return launch_pair_export<4, false>(pl, p, dir, s0);
}
size_t mm_pair_lds_bytes(int phase, int nslotrows, int max_P1) {
    return pair_lds_bytes(MM_ROW_RS, phase, nslotrows, 0, pair_pc(mm_pair_nj(max_P1)));
}
size_t mm_pair_hand_bytes() { return sizeof(PairHand); }

}  // namespace mm
