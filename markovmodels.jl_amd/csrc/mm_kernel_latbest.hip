// mm_kernel_latbest.hip -- lattice best paths (mm_latticebest_f32: the tropical forward-backward over the records of a lattice of
// mm_lattice_f32, under the call's V and an optional score per record: the best path's weight, every record's through-score below it,
// and the best path itself as records and states).  Included by mm_latbest_tu.hip, and by mm_kernel_latsample.hip for lb_key.
//
// mm_latbest_kernel<NT>   mm_latpost_fb_kernel's organisation -- one workgroup of NT threads per utterance, serial over its transitions,
//                         the work of a step the records of its cell, state vectors in LDS as order-preserving codes of floats, an
//                         integer atomicMax per target state -- with ONE pass and ONE barrier per step: a maximum needs no sum and no
//                         finish.  The values are plain float32, no running offset: adds, one subtraction and a max, so a float32
//                         restatement is bit-exact (the order of the codes puts -0 below +0; that is the max and the equality here).
//                         LDS per state: three 32-bit words.  The vectors rotate: a step reads R, accumulates the next vector into A
//                         and empties E, the vector the step before it read (by the targets of that step's cell, so the work stays
//                         the records'); the barrier at the end of a step separates its reads of R from the next step's emptying of
//                         it, and its emptying of E from the next step's atomics on it.
//                         Forward: f_r = a_t(i(r)) + wz_r into score[r], max into a_{t+1}(j(r)).  best = a_len(f).
//                         Backward: score[r] = (f_r + b_{t+1}(j(r))) - best, max of wz_r + b_{t+1}(j(r)) into b_t(i(r)).  The trace
//                         rides in the same loop: among the records of the cell with j(r) = cur the 64-bit key (code of f_r, 2^32 - 1
//                         minus the record's place in its cell) is maximised -- a wave reduction and one 64-bit LDS atomicMax on one of
//                         three rotating slots -- which is the greatest f_r, a_{t+1}(cur) itself, and among its ties the LOWEST r.
//                         Behind the barrier every thread reads the slot and the winner's source (cur of the next step).  No
//                         back-pointers are stored.  A place at or behind 2^32 - 1 (a doctored cell of that many records) has the
//                         key's low word 0: if such a key wins, the lowest record is found by a 64-bit atomicMin behind two more
//                         barriers.
//                         The first record of every thread is gathered AHEAD (LpAhead of mm_kernel_latpost.hip): its four dependent
//                         loads are issued four, three, two and one step early, one stage per step.
// Memory safety: mm_latpost_fb_kernel's -- lp_gather checks a record's entry index, lp_cell clamps the cells, lens are clamped into
// [0, N]; every other index comes from the batch's own tables.
#pragma once
#include "mm_kernel_latpost.hip"

namespace mm {

#define MM_LB_HEAD 64  // bytes of LDS in front of the vectors: three 64-bit key slots and the 64-bit slot of the exact minimum

__device__ __forceinline__ unsigned long long lb_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long lb_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o);
        v = w < v ? w : v;
    }
    return v;
}
// the trace's key of a record whose forward value has the code c at place d of its cell: greater f first, then the lower place
__device__ __forceinline__ unsigned long long lb_key(unsigned c, long long d) {
    return ((unsigned long long)c << 32) | (d < 0xffffffffll ? 0xffffffffu - unsigned(d) : 0u);
}

// the pipeline of first records: c[0] the step's cell, complete; c[1] .. c[4] the cells one to four steps ahead, one stage short each
struct LbPipe {
    LpAhead c[5];
};
__device__ __forceinline__ void lb_pipe_start(const LatPostParams &lp, const LpUtt &u, long long cell0, int t, int dt, bool want_f, LbPipe &pp) {
    lp_ahead_all(lp, nullptr, nullptr, u, cell0, t, want_f, pp.c[0]);
    lp_ahead0(lp, nullptr, nullptr, u, cell0, t + dt, want_f, pp.c[1]);
    lp_ahead1(u, pp.c[1]);
    lp_ahead2(u, pp.c[1]);
    lp_ahead0(lp, nullptr, nullptr, u, cell0, t + 2 * dt, want_f, pp.c[2]);
    lp_ahead1(u, pp.c[2]);
    lp_ahead0(lp, nullptr, nullptr, u, cell0, t + 3 * dt, want_f, pp.c[3]);
}
// at the head of step t: every cell on its way takes its next stage
__device__ __forceinline__ void lb_pipe_issue(const LatPostParams &lp, const LpUtt &u, long long cell0, int t, int dt, bool want_f, LbPipe &pp) {
    lp_ahead3(u, pp.c[1]);
    lp_ahead2(u, pp.c[2]);
    lp_ahead1(u, pp.c[3]);
    lp_ahead0(lp, nullptr, nullptr, u, cell0, t + 4 * dt, want_f, pp.c[4]);
}
__device__ __forceinline__ void lb_pipe_shift(LbPipe &pp) {
#pragma unroll
    for (int q = 0; q < 4; ++q) pp.c[q] = pp.c[q + 1];
}

template <int NT>
__global__ void __launch_bounds__(NT) mm_latbest_kernel(RunParams p, LatPostParams lp, LatBestParams lb) {
    extern __shared__ __attribute__((aligned(16))) char lb_smem[];
    unsigned long long *const slot = reinterpret_cast<unsigned long long *>(lb_smem);  // [3] the trace's keys, 0: empty
    unsigned long long *const slot_x = slot + 3;                                       // the exact minimum (doctored cells only)
    const int b = blockIdx.x, tid = threadIdx.x;
    const UttDesc &ud = p.utts[b];
    const int S1 = ud.S1, fin = S1 - 1;
    unsigned *R = reinterpret_cast<unsigned *>(lb_smem + MM_LB_HEAD), *A = R + ud.S1p, *E = A + ud.S1p;
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
    float *const score = lp.post;
    const bool trace = lb.rec || lb.path;

    // a_0 = alpha_hat + the first frame's emissions; two empty vectors
    for (int s = tid; s < S1; s += NT) {
        const float a = len > 0 ? ud.init[s] + lp_emit(u.Vb, u.vsn, 1, len, u.s2p[s], u.P) : MM_NINF;
        R[s] = a > MM_NINF ? lp_enc(a) : MM_LP_EMPTY;
        A[s] = E[s] = MM_LP_EMPTY;
    }
    if (tid < 3) slot[tid] = 0ull;
    __syncthreads();

    // ---- forward: a step reads a_t in R, accumulates a_{t+1} in A and empties a_{t-1} in E
    long long plo = 0, phi = 0, pplo = 0, pphi = 0;  // the cells one and two steps back, with the target of the thread's first record
    int ptgt = -1, pptgt = -1;
    LbPipe pp;
    lb_pipe_start(lp, u, cell0, 0, 1, false, pp);
    for (int t = 0; t < len; ++t) {
        const long long lo = pp.c[0].lo, hi = pp.c[0].hi;
        lb_pipe_issue(lp, u, cell0, t, 1, false, pp);
        int tgt0 = -1, q = 0;
        for (long long r = lo + tid; r < hi; r += NT, ++q) {
            const LpRec g = q == 0 ? pp.c[0].rec : lp_gather(lp, u, r, t);
            float f = MM_NINF;
            if (g.src >= 0) {
                f = lp_dec(R[g.src]) + g.wz;
                if (f > MM_NINF)
                    atomicMax(&A[g.dst], lp_enc(f));
                else
                    f = MM_NINF;  // (also what a NaN input becomes)
                if (q == 0) tgt0 = g.dst;
            }
            score[r] = f;
        }
        if (t == 1) {
            for (int s = tid; s < S1; s += NT) E[s] = MM_LP_EMPTY;
        } else if (t > 1) {
            q = 0;
            for (long long r = pplo + tid; r < pphi; r += NT, ++q) {
                const int s = q == 0 ? pptgt : lp_target(lp, u, r, true);
                if (s >= 0) E[s] = MM_LP_EMPTY;
            }
        }
        __syncthreads();
        unsigned *const sw = R;
        R = A;
        A = E;
        E = sw;
        pplo = plo;
        pphi = phi;
        pptgt = ptgt;
        plo = lo;
        phi = hi;
        ptgt = tgt0;
        lb_pipe_shift(pp);
    }
    // (the last step's emission is 0 for the phony final state alone: a_len(f) is the best path's weight)
    const float best = lp_dec(R[fin]);
    const bool alive = best > MM_NINF;
    if (tid == 0) lp.logz[b] = alive ? best : MM_NINF;

    // the records of cells at or behind len, and every record of an utterance without a path: no path through them
    for (int t = alive ? len : 0; t < p.N; ++t) {
        long long lo, hi;
        lp_cell(lp, cell0 + t, lo, hi);
        for (long long r = lo + tid; r < hi; r += NT) score[r] = MM_NINF;
    }
    for (int t = (alive ? len : 0) + tid; t < p.N; t += NT) {
        if (lb.rec) lb.rec[(long long)b * lb.rsb + t] = -1ll;
        if (lb.path) lb.path[(long long)b * lb.psb + t] = -1;
    }
    if (!alive) return;

    // ---- backward: b_len = one at f; a step reads b_{t+1} in R, accumulates b_t in A and empties b_{t+2} in E
    __syncthreads();  // (every thread has read best)
    for (int s = tid; s < S1; s += NT) {
        R[s] = s == fin ? lp_enc(0.f) : MM_LP_EMPTY;
        A[s] = E[s] = MM_LP_EMPTY;
    }
    __syncthreads();
    int cur = fin;                   // the state the best path is in behind the step's transition
    int si = 0;                      // the step's key slot of the three; a step empties the slot of the step behind it
    ptgt = pptgt = -1;
    lb_pipe_start(lp, u, cell0, len - 1, -1, true, pp);
    for (int t = len - 1; t >= 0; --t) {
        const long long lo = pp.c[0].lo, hi = pp.c[0].hi;
        lb_pipe_issue(lp, u, cell0, t, -1, true, pp);
        int tgt0 = -1, q = 0;
        unsigned kc = 0u;  // the thread's own maximum among the records into cur: the code of f_r (0: none) and the record
        long long kr = -1;
        for (long long r = lo + tid; r < hi; r += NT, ++q) {
            const float f = q == 0 ? pp.c[0].f : score[r];
            float sc = MM_NINF;
            const LpRec g = q == 0 ? pp.c[0].rec : lp_gather(lp, u, r, t);
            if (g.src >= 0) {
                const float bj = lp_dec(R[g.dst]);
                const float z = g.wz + bj, y = f + bj;
                if (z > MM_NINF) atomicMax(&A[g.src], lp_enc(z));
                if (y > MM_NINF) sc = y - best;
                if (q == 0) tgt0 = g.src;
                if (trace && g.dst == cur && f > MM_NINF) {  // (r ascends: the first of the thread's own ties stays)
                    const unsigned c = lp_enc(f);
                    if (c > kc) {
                        kc = c;
                        kr = r;
                    }
                }
            }
            score[r] = sc;
        }
        if (t == len - 2) {
            if (tid == 0) E[fin] = MM_LP_EMPTY;
        } else if (t < len - 2) {
            q = 0;
            for (long long r = pplo + tid; r < pphi; r += NT, ++q) {
                const int s = q == 0 ? pptgt : lp_target(lp, u, r, false);
                if (s >= 0) E[s] = MM_LP_EMPTY;
            }
        }
        if (trace) {
            const unsigned long long key = lb_wave_max(kr >= 0 ? lb_key(kc, kr - lo) : 0ull);
            if ((tid & 63) == 0 && key) atomicMax(&slot[si], key);
            // the next step's slot: last read two steps ago, in front of the barrier before this one; the next step's atomics
            // come behind this step's barrier
            if (tid == 0) slot[si == 2 ? 0 : si + 1] = 0ull;
        }
        __syncthreads();
        if (trace) {
            const unsigned long long win = slot[si];
            long long r = -1;
            if (win) {
                const unsigned low = unsigned(win);
                r = lo + (long long)(0xffffffffu - low);
                if (low == 0u) {  // a cell of 2^32 - 1 records or more whose maxima all lie that far in: the exact lowest of them
                    // (uniform: every thread read the same key.  A thread whose own maximum has the winning code holds the lowest
                    // of its own ties, and none of them lies in front of place 2^32 - 1, or the low word were not 0)
                    if (tid == 0) *slot_x = ~0ull;
                    __syncthreads();
                    unsigned long long m = kc == unsigned(win >> 32) ? (unsigned long long)kr : ~0ull;
                    m = lb_wave_min(m);
                    if ((tid & 63) == 0 && m != ~0ull) atomicMin(slot_x, m);
                    __syncthreads();
                    r = *slot_x == ~0ull ? -1 : (long long)*slot_x;
                }
            }
            const int i = r >= 0 ? lp_target(lp, u, r, false) : -1;
            if (tid == 0) {
                if (lb.rec) lb.rec[(long long)b * lb.rsb + t] = i >= 0 ? r : -1ll;
                if (lb.path) lb.path[(long long)b * lb.psb + t] = i;
            }
            cur = i;
            si = si == 2 ? 0 : si + 1;
        }
        unsigned *const sw = R;
        R = A;
        A = E;
        E = sw;
        pplo = plo;
        pphi = phi;
        pptgt = ptgt;
        plo = lo;
        phi = hi;
        ptgt = tgt0;
        lb_pipe_shift(pp);
    }
}

}  // namespace mm
