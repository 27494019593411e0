// mm_kernel_latsample.hip -- lattice path sampling (mm_latticesample_f32: record sequences drawn from the posterior of a lattice of
// mm_lattice_f32, under the call's V and an optional score per record).  Included by mm_latsample_tu.hip only.
//
// mm_latsample_fwd_kernel<NT>  lp_fb<NT, false, true>: the forward half of mm_latpost_fb_kernel, to the letter -- it ends behind logz
//                              and the -inf fill, so fwd[r] keeps x_r = a_t(i(r)) + wz_r relative to the offset in front of step t
//                              (one constant per cell), -inf for a dead record, a record with no path into its source, the cells at
//                              or behind len and every record of an utterance without a path.
// mm_latsample_kernel<NT>      workgroup (b, c) draws the samples k = 64 c .. 64 c + 63 of utterance b, serial over the transitions
//                              backwards.  A sample sits in one state (f behind the last transition); its record of cell t is the
//                              Gumbel-max draw among the records into that state: the greatest x_r + g_r, g_r = -log(-log u) with
//                              u = unit_open(philox_4x32_10(seed; b, k, t, place of r in its cell).x).  x_r - a_{t+1}(j(r)) is the log
//                              of the record's probability given its destination and a_{t+1}(j) is common to the candidates, so the
//                              argmax is a draw from that conditional; the cell's offset cancels the same way.  A maximum is
//                              order-free: the trace of mm_latbest_kernel with perturbed keys, and the same bits whatever the
//                              thread count.
//                              LDS: a 64-bit occupancy mask per state (bit q: sample 64 c + q sits there) and two sets of 64 key
//                              slots of 64 bits, (code of the key, 2^32 - 1 - place), 0: empty -- step t takes set t & 1.  A step:
//                                scan   every thread takes records lo + tid + q NT of the cell: arc[r] -> destination -> mask.  Most
//                                       records stop at an empty mask.  For every set bit, with fwd[r] finite: one Philox call, two
//                                       logf, one 64-bit LDS atomicMax into the sample's slot.  A place at or behind 2^32 - 1 (a
//                                       doctored cell of that many records) is passed over: never drawn.
//                                barrier
//                                move   lane q of wave 0 reads its slot: the winner's place, its source and wz through lp_gather;
//                                       rec / path stored, wz added to the chain's float64 weight, its bit moved from the old state's
//                                       mask to the source's (atomicAnd / atomicOr: the lanes' bits differ, so the updates of one
//                                       word commute), its slot emptied.
//                                barrier
//                              The second barrier publishes the masks to the next scan; the emptied set is used again two steps on.
//                              The work of a step is the records of the cell, plus the records into at most 64 states.  The first
//                              record of every thread is gathered AHEAD (LpAhead of mm_kernel_latpost.hip, its first two stages:
//                              arc[r] and fwd[r] two steps early, the entry's ends one step early).
//                              A chain of an utterance with a path never dies: the chosen record has a finite x_r, so its source
//                              has a finite a_t, which is the log-sum of finite x of the cell before.  (Only a doctored cell's
//                              passed-over places can empty a slot: the chain's remaining entries are -1 and its logprob -inf.)
// Memory safety: mm_latpost_fb_kernel's -- lp_entry checks a record's entry index, lp_cell clamps the cells, lens are clamped into
// [0, N]; a winner's place is below the cell's size because only scanned records write keys; states come from the batch's tables.
#pragma once
#include "mm_kernel_latbest.hip"  // lb_key (and, through it, mm_kernel_latpost.hip)
#include "mm_philox.h"

namespace mm {

#define MM_LS_HEAD (2 * MM_LS_CHUNK * 8)  // bytes of LDS in front of the masks: the two sets of key slots

template <int NT>
__global__ void __launch_bounds__(NT) mm_latsample_fwd_kernel(RunParams p, LatPostParams lp) {
    extern __shared__ __attribute__((aligned(16))) char lp_smem[];
    lp_fb<NT, false, true>(lp_smem, p, lp, LatCostParams{});
}

// the Gumbel variate of the uniform u in (0, 1): 2^23 values in about [-2.81, 16.64]
__device__ __forceinline__ float ls_gumbel(float u) { return -logf(-logf(u)); }

template <int NT>
__global__ void __launch_bounds__(NT) mm_latsample_kernel(RunParams p, LatPostParams lp, LatSampleParams ls) {
    extern __shared__ __attribute__((aligned(16))) char ls_smem[];
    unsigned long long *const slot = reinterpret_cast<unsigned long long *>(ls_smem);  // [2][64] the samples' keys, 0: empty
    unsigned long long *const mask = slot + 2 * MM_LS_CHUNK;                            // [S1p] who sits in the state
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long k0 = (long long)blockIdx.y * MM_LS_CHUNK;
    const int nk = ls.nsamples - k0 < MM_LS_CHUNK ? int(ls.nsamples - k0) : MM_LS_CHUNK;
    const UttDesc &ud = p.utts[b];
    const int S1 = ud.S1, fin = S1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    LpUtt u;
    u.ld = lp.arcs + b;
    u.s2p = ud.s2p;
    u.Vb = p.V + (long long)b * p.vsb;
    u.vsn = p.vsn;
    u.len = len;
    u.P = ud.P1 - 1;
    const long long cell0 = (long long)b * p.N;
    const float *const fwd = lp.post;
    const float logz = lp.logz[b];  // the forward pass's
    const bool alive = logz > MM_NINF;
    long long *const recb = ls.rec ? ls.rec + (long long)b * ls.rsb + k0 * ls.rsk : nullptr;
    int *const pathb = ls.path ? ls.path + (long long)b * ls.psb + k0 * ls.psk : nullptr;

    // behind len, and everywhere without a path: -1
    {
        const int t0 = alive ? len : 0, w = p.N - t0;
        for (long long e = tid; e < (long long)nk * w; e += NT) {
            const int q = int(e / w), t = t0 + int(e - (long long)q * w);
            if (recb) recb[q * ls.rsk + t] = -1ll;
            if (pathb) pathb[q * ls.psk + t] = -1;
        }
    }
    if (!alive) {
        if (ls.logprob && tid < nk) ls.logprob[(long long)b * ls.lsb + k0 + tid] = MM_NINF;
        return;
    }

    for (int s = tid; s < S1; s += NT) mask[s] = 0ull;
    if (tid < 2 * MM_LS_CHUNK) slot[tid] = 0ull;
    __syncthreads();
    if (tid == 0) mask[fin] = nk == MM_LS_CHUNK ? ~0ull : (1ull << nk) - 1ull;
    __syncthreads();

    // the chain of lane q of wave 0: its state behind the step's transition (-1: dead), its weight so far
    const bool chain = tid < nk;
    int cur = fin;
    double W = 0.0;
    LatPostParams lps = lp;  // the scan needs no extra
    lps.extra = nullptr;
    LpAhead ca, na;  // the step's cell with the thread's first record (two stages of it), and the cell in front of it on its way
    lp_ahead0(lps, nullptr, nullptr, u, cell0, len - 1, true, ca);
    lp_ahead1(u, ca);
    lp_ahead0(lps, nullptr, nullptr, u, cell0, len - 2, true, na);
    for (int t = len - 1; t >= 0; --t) {
        const long long lo = ca.lo, hi = ca.hi;
        unsigned long long *const set = slot + (t & 1) * MM_LS_CHUNK;
        lp_ahead1(u, na);
        // scan
        int q = 0;
        for (long long r = lo + tid; r < hi; r += NT, ++q) {
            const int dst = q == 0 ? (ca.src >= 0 ? ca.dst : -1) : lp_target(lp, u, r, true);
            if (dst < 0) continue;
            unsigned long long m = mask[dst];
            if (!m) continue;
            const float x = q == 0 ? ca.f : fwd[r];
            const long long place = r - lo;
            if (!(x > MM_NINF) || place >= 0xffffffffll) continue;
            do {
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                const float g = ls_gumbel(unit_open(philox_4x32_10(ls.key0, ls.key1, (unsigned)b, (unsigned)(k0 + bit), (unsigned)t, (unsigned)place).x));
                atomicMax(&set[bit], lb_key(lp_enc(x + g), place));
            } while (m);
        }
        __syncthreads();
        // move
        if (chain) {
            const unsigned long long win = set[tid];
            long long r = -1;
            LpRec g{-1, -1, MM_NINF};
            if (win && cur >= 0) {
                r = lo + (long long)(0xffffffffu - unsigned(win));
                g = lp_gather(lp, u, r, t);
            }
            if (g.src < 0) r = -1;
            if (recb) recb[tid * ls.rsk + t] = r;
            if (pathb) pathb[tid * ls.psk + t] = g.src;
            if (cur >= 0) {
                const unsigned long long me = 1ull << tid;
                atomicAnd(&mask[cur], ~me);
                if (g.src >= 0) {
                    atomicOr(&mask[g.src], me);
                    W += double(g.wz);
                }
                cur = g.src;
            }
            set[tid] = 0ull;
        }
        __syncthreads();
        ca = na;
        lp_ahead0(lps, nullptr, nullptr, u, cell0, t - 2, true, na);
    }
    if (chain && ls.logprob) {
        float lpv = MM_NINF;
        if (cur >= 0) {
            W += double(ud.init[cur] + lp_emit(u.Vb, u.vsn, 1, len, u.s2p[cur], u.P));
            lpv = float(W - double(logz));
        }
        ls.logprob[(long long)b * ls.lsb + k0 + tid] = lpv;
    }
}

}  // namespace mm
