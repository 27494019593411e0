// mm_kernel_latpost.hip -- lattice posteriors (mm_latticeposteriors_f32: the log-semiring forward-backward over the records of a
// lattice of mm_lattice_f32, under the call's V and an optional score per record).  Included by mm_latpost_tu.hip only.
//
// mm_latpost_fb_kernel<NT>     one workgroup of NT threads per utterance, serial over its transitions; the work of a step is the
//                              records of its cell, never the graph.  LDS per state: two 32-bit words X and Y and a 64-bit sum.  X
//                              holds the current vector (a_t forward, b_{t+1} backward) as order-preserving codes of floats, relative
//                              to the offset accumulated so far; Y and `sum` are the accumulators of the next vector and are empty
//                              between steps.  A step is three passes over the cell, a thread at the records lo + tid + q NT:
//                                A  gather (source, destination, weight) through arc[r], the emission of the destination and extra[r];
//                                   x_r = (X[from] - M) + w + extra + e; integer max of its code into Y[to]
//                                B  sum[to] += rint(exp(x_r - Y[to]) 2^40), a 64-bit integer add
//                                C  the thread whose exchange takes a nonzero sum[to] back to 0 finishes the state:
//                                   Y[to] = Y[to] + log(sum 2^-40); the states the previous step finished are emptied in X; the maximum
//                                   M of the finished values goes into the offset (a double) and is subtracted by the next step's reads
//                              then X and Y change roles.  Integer max and integer add are exact in any order, so nothing depends on
//                              the order the LDS serves the threads in: a repeated call returns the same bits.  The term of the
//                              maximum is exactly 2^40, so a touched state's sum is never 0 -- which is what makes the exchange a
//                              claim -- and the terms lost are below 2^-41 of the largest.
//                              Forward: post[r] = x_r (relative to the offset in front of the step).  Backward (to = the source):
//                              y_r = post[r] + (X[j] - M), post[r] = y_r - LSE_cell(y): the cell's own log-sum normalises, log Z is
//                              never subtracted from anything.  The first record of every thread stays in registers across the
//                              passes; the others are gathered again.  That first record is gathered AHEAD (LpAhead): its four
//                              dependent loads are issued two steps early, one per pass, so a step with at most NT records waits
//                              for no global load of its own.
// mm_latpost_gamma_kernel<NT>  one workgroup per (b, n): exp(post[r]) of the cell summed by the pdf of the source in 64-bit fixed
//                              point in LDS, the row written with its zeros.
// lp_fb<NT, COST, FWD_ONLY>    the body of both forward-backward kernels (FWD_ONLY: of mm_kernel_latsample.hip's forward pass, which ends
//                              behind logz and the -inf fill: post keeps every record's forward value x_r).  COST (mm_latcost_fb_kernel<NT>, mm_latticecost_f32) carries
//                              the expected cost of the paths beside the vectors: a float C per state (ca_t forward, cb_{t+1} backward,
//                              relative to the maximum Cm of the step that finished it -- forward, Cm accumulates in a double, which
//                              ends as the risk) and a signed 64-bit sum.  Pass A also takes the block's maximum vmax of |v_r|,
//                              v_r = (C[from] - Cm) + cost[r]; pass B adds rint(exp(x_r - Y[to]) (v_r / vmax) 2^40) to the cost sum;
//                              the thread that finishes a state in pass C sets C[to] = (cost sum / sum) vmax.  Forward, diff[r]
//                              keeps v_r; backward, u_r = v_r + (C[j] - Cm) is the cost of the paths through r up to a constant of
//                              the cell, and diff[r] = exp(post[r]) (u_r - u_bar) with u_bar the cell's own posterior mean of u, in
//                              the same fixed point: no offset of the forward pass is needed, and a cell's diff sums to 0.  The
//                              maxima and sums share the barriers the posteriors have already; integer sums: any order, same bits.
// mm_latcost_grad_kernel<NT>   one workgroup per (b, n): diff[r] of the cell summed by the pdf of the source, as signed 64-bit
//                              fixed point relative to the cell's largest |diff|, and mm_latpost_gamma_kernel's sums of exp(post).
// Memory safety: a record's entry index is checked against the utterance's entry count, the cells are clamped into [0, nrec] and
// made non-decreasing, lens into [0, N]; every other index comes from the batch's own tables.
#pragma once
#include "mm_internal.h"
#include "mm_kernels.hip"

namespace mm {

#define MM_LP_HEAD 64                // bytes of LDS in front of the per-state arrays: 2 x 2 max slots, 2 64-bit sum slots
#define MM_LP_EMPTY 0x007fffffu      // lp_enc(-inf): an accumulator nobody touched
#define MM_LP_ONE 1099511627776.f    // 2^40: the fixed point of the sums
#define MM_LC_HEAD 80                // ... of the instance with costs: 3 x 2 more max slots (8 bytes unused), 2 signed 64-bit sum slots

// floats as unsigned integers in the floats' order (NaN never gets here: callers pass x > -inf only)
__device__ __forceinline__ unsigned lp_enc(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// exp(d) for d <= 0 in fixed point (d = 0: exactly 2^40), and the log of a sum of such terms (2^40: exactly 0)
__device__ __forceinline__ unsigned long long lp_fix(float d) { return __float2ull_rn(expf(d) * MM_LP_ONE); }
__device__ __forceinline__ float lp_log(unsigned long long s) { return logf(float(__ull2double_rn(s) * (1.0 / 1099511627776.0))); }

// the emission of state j's pdf in the 1-based frame n: the pdf's log-likelihood up to len, the phony pdf's 0 behind it
__device__ __forceinline__ float lp_emit(const float *Vb, long long vsn, int n, int len, int pdf, int P) {
    if (pdf < P) return n <= len ? Vb[(long long)(n - 1) * vsn + pdf] : MM_NINF;
    return n <= len ? MM_NINF : 0.f;
}

// the block's maximum of v: one barrier.  *slot holds MM_LP_EMPTY on entry and the maximum on exit; the CALLER empties it again,
// behind a later barrier (every thread has read it by then) and in front of the barrier before its next use.  The kernel keeps two
// slots per purpose and alternates: a step empties the slots of the step before it.
__device__ __forceinline__ float lp_block_max(unsigned *slot, float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0 && v > MM_NINF) atomicMax(slot, lp_enc(v));
    __syncthreads();
    return lp_dec(*slot);
}
__device__ __forceinline__ unsigned long long lp_block_sum(unsigned long long *slot, unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(slot, v);
    __syncthreads();
    return *slot;
}

// the maximum / the sum of a wave into a slot, without a barrier: the caller's next lp_block_max / lp_block_sum / __syncthreads
// publishes it (the slots alternate and are emptied as lp_block_max says)
__device__ __forceinline__ void lp_wave_max(unsigned *slot, float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0 && v > MM_NINF) atomicMax(slot, lp_enc(v));
}
__device__ __forceinline__ void lp_wave_add(long long *slot, long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(slot), (unsigned long long)v);
}
// exp(d) s for d <= 0 and |s| <= 1 in signed fixed point; the value of a state: its cost sum over its sum, times the scale
__device__ __forceinline__ long long lc_fix(float d, float s) { return __float2ll_rn(expf(d) * MM_LP_ONE * s); }
__device__ __forceinline__ void lc_add(long long *a, long long v) { atomicAdd(reinterpret_cast<unsigned long long *>(a), (unsigned long long)v); }
__device__ __forceinline__ float lc_val(long long cs, unsigned long long s, float scale) {
    return scale > 0.f ? float(__ll2double_rn(cs) / __ull2double_rn(s)) * scale : 0.f;
}
// v over the block's largest |v|: a division, so that the largest term is exactly +-1 (and a cell of one record exact)
__device__ __forceinline__ float lc_ratio(float v, float scale) { return scale > 0.f ? v / scale : 0.f; }

struct LpRec {
    int src, dst;  // src < 0: a dead record (an index outside the utterance's entries, the phony self-loop)
    float wz;      // w + extra + e(dst)
};

// what the kernels know of one utterance
struct LpUtt {
    const LatticeDev *ld;
    const int *s2p;
    const float *Vb;
    long long vsn;
    int len, P;
};

__device__ __forceinline__ int lp_entry(const LatPostParams &lp, const LpUtt &u, long long r) {
    const int k = lp.arc[r];
    return k >= 0 && k < u.ld->nnz ? k : -1;
}
// the end of record r a step sums into (forward: the destination, backward: the source); -1 for a dead record
__device__ __forceinline__ int lp_target(const LatPostParams &lp, const LpUtt &u, long long r, bool fwd) {
    const int k = lp_entry(lp, u, r);
    if (k < 0) return -1;
    const int i = u.ld->src[k];
    return i < 0 ? -1 : (fwd ? u.ld->dst[k] : i);
}
__device__ __forceinline__ LpRec lp_gather(const LatPostParams &lp, const LpUtt &u, long long r, int t) {
    LpRec g{-1, -1, MM_NINF};
    const int k = lp_entry(lp, u, r);
    if (k < 0) return g;
    const int i = u.ld->src[k];
    if (i < 0) return g;
    const int j = u.ld->dst[k];
    const float w = u.ld->w[k], ex = lp.extra ? lp.extra[r] : 0.f;
    const float e = lp_emit(u.Vb, u.vsn, t + 2, u.len, u.s2p[j], u.P);
    g.src = i;
    g.dst = j;
    g.wz = (w + ex) + e;
    return g;
}

// the records of cell (b, t): [lo, hi) inside [0, nrec], whatever the offsets hold
__device__ __forceinline__ void lp_cell(const LatPostParams &lp, long long c, long long &lo, long long &hi) {
    const long long a = lp.offs[c], z = lp.offs[c + 1];
    lo = a < 0 ? 0 : (a > lp.nrec ? lp.nrec : a);
    hi = z < lo ? lo : (z > lp.nrec ? lp.nrec : z);
}

// The first record of a thread in a cell, gathered a stage at a time so that no load waits for the one before it inside a pass: the
// four dependent loads of a record (arc[r]; the three planes at k; the destination's pdf; its emission) do not depend on the
// recursion, so they are issued two steps ahead and one per pass.  lp_ahead3 ends where lp_gather does.
struct LpAhead {
    long long lo, hi;  // the cell
    int t, k;          // its transition; the raw arc[r] (-1: the thread has no record there)
    float ex, f;       // extra[r]; post[r] (the forward value, for the backward pass)
    float cost, fc;    // with costs: cost[r]; diff[r] (the forward cost, for the backward pass)
    int src, dst, pdf;
    float w;
    LpRec rec;
};
__device__ __forceinline__ void lp_ahead0(const LatPostParams &lp, const float *cost, const float *fcost, const LpUtt &u, long long cell0, int t,
                                          bool want_f, LpAhead &a) {
    a.t = t;
    a.cost = a.fc = 0.f;
    a.k = -1;
    a.ex = 0.f;
    a.f = MM_NINF;
    a.src = -1;
    a.lo = a.hi = 0;
    if (t < 0 || t >= u.len) return;
    lp_cell(lp, cell0 + t, a.lo, a.hi);
    const long long r = a.lo + threadIdx.x;
    if (r < a.hi) {
        a.k = lp.arc[r];
        if (lp.extra) a.ex = lp.extra[r];
        if (want_f) a.f = lp.post[r];
        if (cost) a.cost = cost[r];
        if (cost && want_f) a.fc = fcost[r];
    }
}
__device__ __forceinline__ void lp_ahead1(const LpUtt &u, LpAhead &a) {
    a.src = -1;
    a.dst = 0;
    a.w = MM_NINF;
    if (a.k >= 0 && a.k < u.ld->nnz) {
        a.src = u.ld->src[a.k];
        a.dst = u.ld->dst[a.k];
        a.w = u.ld->w[a.k];
    }
}
__device__ __forceinline__ void lp_ahead2(const LpUtt &u, LpAhead &a) { a.pdf = a.src >= 0 ? u.s2p[a.dst] : u.P; }
__device__ __forceinline__ void lp_ahead3(const LpUtt &u, LpAhead &a) {
    a.rec = LpRec{-1, -1, MM_NINF};
    if (a.src >= 0) a.rec = LpRec{a.src, a.dst, (a.w + a.ex) + lp_emit(u.Vb, u.vsn, a.t + 2, u.len, a.pdf, u.P)};
}
__device__ __forceinline__ void lp_ahead_all(const LatPostParams &lp, const float *cost, const float *fcost, const LpUtt &u, long long cell0, int t,
                                             bool want_f, LpAhead &a) {
    lp_ahead0(lp, cost, fcost, u, cell0, t, want_f, a);
    lp_ahead1(u, a);
    lp_ahead2(u, a);
    lp_ahead3(u, a);
}

template <int NT, bool COST, bool FWD_ONLY = false>
__device__ __forceinline__ void lp_fb(char *lp_smem, const RunParams &p, const LatPostParams &lp, const LatCostParams &lc) {
    unsigned *const slot_m = reinterpret_cast<unsigned *>(lp_smem);       // [2] the step's maximum
    unsigned *const slot_y = slot_m + 2;                                   // [2] the cell's maximum (backward)
    unsigned long long *const slot_s = reinterpret_cast<unsigned long long *>(lp_smem + 16);  // [2] the cell's sum (backward)
    const int b = blockIdx.x, tid = threadIdx.x;
    const UttDesc &ud = p.utts[b];
    const int S1 = ud.S1, fin = S1 - 1;
    unsigned *const slot_v = reinterpret_cast<unsigned *>(lp_smem + 32);  // [2] with costs: the cell's largest |v| (backward: |w|)
    unsigned *const slot_c = slot_v + 2;                                   // [2] the step's largest C
    unsigned *const slot_u = slot_v + 4;                                   // [2] the cell's largest |u| (backward)
    long long *const slot_us = reinterpret_cast<long long *>(lp_smem + 64);  // [2] the cell's sum of u (backward)
    unsigned long long *const sum = reinterpret_cast<unsigned long long *>(lp_smem + (COST ? MM_LC_HEAD : MM_LP_HEAD));  // [S1p]
    long long *const csum = reinterpret_cast<long long *>(sum + ud.S1p);  // [S1p] with costs
    unsigned *X = reinterpret_cast<unsigned *>(sum + (COST ? 2 : 1) * ud.S1p), *Y = X + ud.S1p;
    float *const C = reinterpret_cast<float *>(X + 2 * ud.S1p);  // [S1p] with costs
    const float *const costp = COST ? lc.cost : nullptr, *const fcostp = COST ? lc.diff : nullptr;
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

    // a_0 = alpha_hat + the first frame's emissions; empty accumulators
    float lm = MM_NINF;
    for (int s = tid; s < S1; s += NT) {
        const float a = len > 0 ? ud.init[s] + lp_emit(u.Vb, u.vsn, 1, len, u.s2p[s], u.P) : MM_NINF;
        X[s] = a > MM_NINF ? lp_enc(a) : MM_LP_EMPTY;
        Y[s] = MM_LP_EMPTY;
        sum[s] = 0ull;
        if constexpr (COST) {
            csum[s] = 0ll;
            C[s] = 0.f;  // ca_0
        }
        lm = fmaxf(lm, a > MM_NINF ? a : MM_NINF);
    }
    if (tid == 0) {
        slot_m[0] = slot_m[1] = MM_LP_EMPTY;
        slot_y[0] = slot_y[1] = MM_LP_EMPTY;
        slot_s[0] = slot_s[1] = 0ull;
        if constexpr (COST) {
            slot_v[0] = slot_v[1] = slot_c[0] = slot_c[1] = slot_u[0] = slot_u[1] = MM_LP_EMPTY;
            slot_us[0] = slot_us[1] = 0ll;
        }
    }
    __syncthreads();
    float M = lp_block_max(slot_m, lm);  // what the reads of the next step subtract (slot 0; step t takes slot (t + 1) & 1)
    bool alive = M > MM_NINF;
    double acc = alive ? double(M) : 0.0;  // the offset in front of the vector in X: true value = acc + (X - M)
    float Cm = 0.f;                         // with costs: true ca = coff + (C - Cm)
    double coff = 0.0;

    // ---- forward
    long long plo = 0, phi = 0;  // the cell of the previous step, and the target of this thread's first record there
    int ptgt = -1;
    LpAhead cur, nxt;  // this step's cell with the thread's first record, and the cell after it on its way
    lp_ahead_all(lp, costp, fcostp, u, cell0, 0, false, cur);
    lp_ahead0(lp, costp, fcostp, u, cell0, 1, false, nxt);
    for (int t = 0; t < len; ++t) {
        const long long lo = cur.lo, hi = cur.hi;
        const int par = (t + 1) & 1;
        int tgt0 = -1;
        float x0 = MM_NINF, v0 = 0.f, lvm = MM_NINF;
        lp_ahead1(u, nxt);
        // A
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                float x = MM_NINF, v = 0.f;
                int tgt = -1;
                if (alive) {
                    const LpRec g = q == 0 ? cur.rec : lp_gather(lp, u, r, t);
                    if (g.src >= 0) {
                        x = (lp_dec(X[g.src]) - M) + g.wz;
                        if (x > MM_NINF) {
                            tgt = g.dst;
                            if constexpr (COST) v = (C[g.src] - Cm) + (q == 0 ? cur.cost : lc.cost[r]);
                        } else {
                            x = MM_NINF;  // (also what a NaN input becomes)
                        }
                    }
                }
                lp.post[r] = x;
                if (tgt >= 0) atomicMax(&Y[tgt], lp_enc(x));
                if constexpr (COST) {
                    lc.diff[r] = v;
                    if (tgt >= 0) lvm = fmaxf(lvm, fabsf(v));
                }
                if (q == 0) {
                    tgt0 = tgt;
                    x0 = x;
                    v0 = v;
                }
            }
        }
        if constexpr (COST) lp_wave_max(slot_v + par, lvm);
        __syncthreads();
        if (tid == 0) {  // (the step before: read by everyone in front of this barrier)
            slot_m[1 - par] = MM_LP_EMPTY;
            if constexpr (COST) slot_v[1 - par] = slot_c[1 - par] = MM_LP_EMPTY;
        }
        const float vmax = COST ? lp_dec(slot_v[par]) : 0.f;
        lp_ahead2(u, nxt);
        // B
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                const float x = q == 0 ? x0 : lp.post[r];
                const int tgt = q == 0 ? tgt0 : (x > MM_NINF ? lp_target(lp, u, r, true) : -1);
                if (tgt >= 0) {
                    const float d = x - lp_dec(Y[tgt]);
                    atomicAdd(&sum[tgt], lp_fix(d));
                    if constexpr (COST) lc_add(&csum[tgt], lc_fix(d, lc_ratio(q == 0 ? v0 : lc.diff[r], vmax)));
                }
            }
        }
        __syncthreads();
        lp_ahead3(u, nxt);
        // C
        lm = MM_NINF;
        float lcm = MM_NINF;
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                const int tgt = q == 0 ? tgt0 : (lp.post[r] > MM_NINF ? lp_target(lp, u, r, true) : -1);
                if (tgt < 0) continue;
                const unsigned long long s = atomicExch(&sum[tgt], 0ull);
                if (s) {
                    const float v = lp_dec(Y[tgt]) + lp_log(s);
                    Y[tgt] = lp_enc(v);
                    lm = fmaxf(lm, v);
                    if constexpr (COST) {  // (the claim covers the cost sum: nobody else touches it behind pass B)
                        const float c = lc_val(csum[tgt], s, vmax);
                        csum[tgt] = 0ll;
                        C[tgt] = c;
                        lcm = fmaxf(lcm, c);
                    }
                }
            }
            if (t == 0) {
                for (int s = tid; s < S1; s += NT) X[s] = MM_LP_EMPTY;
            } else {
                q = 0;
                for (long long r = plo + tid; r < phi; r += NT, ++q) {
                    const int s = q == 0 ? ptgt : lp_target(lp, u, r, true);
                    if (s >= 0) X[s] = MM_LP_EMPTY;
                }
            }
        }
        if constexpr (COST) lp_wave_max(slot_c + par, lcm);
        const float Mn = lp_block_max(slot_m + par, lm);
        if (Mn > MM_NINF) {
            acc += double(Mn);
            M = Mn;
            if constexpr (COST) {
                Cm = lp_dec(slot_c[par]);
                coff += double(Cm);
            }
        } else {
            alive = false;
        }
        unsigned *const sw = X;
        X = Y;
        Y = sw;
        plo = lo;
        phi = hi;
        ptgt = tgt0;
        cur = nxt;
        lp_ahead0(lp, costp, fcostp, u, cell0, t + 2, false, nxt);
    }
    // (the last step's emission is 0 for the phony final state alone: what is alive here ends in f, and acc is its weight -- and
    // coff, the offset of ca_len(f), the risk)
    if (tid == 0) {
        lp.logz[b] = alive ? float(acc) : MM_NINF;
        if constexpr (COST) lc.risk[b] = alive ? float(coff) : 0.f;
    }

    // the records of cells at or behind len, and every record of an utterance without a path: no path through them
    for (int t = alive ? len : 0; t < p.N; ++t) {
        long long lo, hi;
        lp_cell(lp, cell0 + t, lo, hi);
        for (long long r = lo + tid; r < hi; r += NT) {
            lp.post[r] = MM_NINF;
            if constexpr (COST) lc.diff[r] = 0.f;
        }
    }
    if (FWD_ONLY || !alive) return;

    // ---- backward: b_len = one at f
    for (int s = tid; s < S1; s += NT) {
        X[s] = s == fin ? lp_enc(0.f) : MM_LP_EMPTY;
        Y[s] = MM_LP_EMPTY;
    }
    __syncthreads();
    if (tid == 0) {  // (the forward pass's: every thread is behind its last read)
        slot_m[0] = slot_m[1] = MM_LP_EMPTY;
        if constexpr (COST) {
            slot_v[0] = slot_v[1] = slot_c[0] = slot_c[1] = MM_LP_EMPTY;
            C[fin] = 0.f;  // cb_len(f)
        }
    }
    __syncthreads();
    M = 0.f;
    Cm = 0.f;
    ptgt = -1;
    lp_ahead_all(lp, costp, fcostp, u, cell0, len - 1, true, cur);
    lp_ahead0(lp, costp, fcostp, u, cell0, len - 2, true, nxt);
    for (int t = len - 1; t >= 0; --t) {
        const long long lo = cur.lo, hi = cur.hi;
        const int par = t & 1;
        int tgt0 = -1;
        float y0 = MM_NINF, z0 = MM_NINF, u0 = 0.f, w0 = 0.f, lum = MM_NINF, lwm = MM_NINF;
        lp_ahead1(u, nxt);
        // A: y = forward value + b(j), z = the record's own weight + b(j); the maximum of z by source, of y over the cell
        lm = MM_NINF;
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                const float f = q == 0 ? cur.f : lp.post[r];
                float y = MM_NINF, z = MM_NINF, uu = 0.f, ww = 0.f;
                int tgt = -1;
                if (alive && f > MM_NINF) {
                    const LpRec g = q == 0 ? cur.rec : lp_gather(lp, u, r, t);
                    if (g.src >= 0) {
                        const float bj = lp_dec(X[g.dst]) - M;
                        y = f + bj;
                        z = g.wz + bj;
                        if (y > MM_NINF && z > MM_NINF) {
                            tgt = g.src;
                            if constexpr (COST) {  // u: the cost of the paths through r, up to a constant of the cell; w: cb's term
                                const float cbj = C[g.dst] - Cm;
                                uu = (q == 0 ? cur.fc : lc.diff[r]) + cbj;
                                ww = (q == 0 ? cur.cost : lc.cost[r]) + cbj;
                            }
                        } else {
                            y = z = MM_NINF;
                        }
                    }
                }
                lp.post[r] = y;
                if (tgt >= 0) atomicMax(&Y[tgt], lp_enc(z));
                lm = fmaxf(lm, y);
                if constexpr (COST) {
                    lc.diff[r] = uu;
                    if (tgt >= 0) {
                        lum = fmaxf(lum, fabsf(uu));
                        lwm = fmaxf(lwm, fabsf(ww));
                    }
                }
                if (q == 0) {
                    tgt0 = tgt;
                    y0 = y;
                    z0 = z;
                    u0 = uu;
                    w0 = ww;
                }
            }
        }
        if constexpr (COST) {
            lp_wave_max(slot_u + par, lum);
            lp_wave_max(slot_v + par, lwm);
        }
        const float ym = lp_block_max(slot_y + par, lm);
        if (tid == 0) {  // (the slots of the step before: read by everyone in front of this barrier)
            slot_m[1 - par] = MM_LP_EMPTY;
            slot_y[1 - par] = MM_LP_EMPTY;
            slot_s[1 - par] = 0ull;
            if constexpr (COST) {
                slot_v[1 - par] = slot_c[1 - par] = slot_u[1 - par] = MM_LP_EMPTY;
                slot_us[1 - par] = 0ll;
            }
        }
        const float umax = COST ? lp_dec(slot_u[par]) : 0.f, wmax = COST ? lp_dec(slot_v[par]) : 0.f;
        lp_ahead2(u, nxt);
        // B
        unsigned long long cs = 0ull;
        long long us = 0ll;
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                float y = y0, z = z0, uu = u0, ww = w0;
                int tgt = tgt0;
                if (q) {
                    y = lp.post[r];
                    tgt = -1;
                    if (y > MM_NINF) {
                        const LpRec g = lp_gather(lp, u, r, t);  // (alive, as y says)
                        z = g.wz + (lp_dec(X[g.dst]) - M);
                        tgt = g.src;
                        if constexpr (COST) {
                            uu = lc.diff[r];
                            ww = lc.cost[r] + (C[g.dst] - Cm);
                        }
                    }
                }
                if (tgt >= 0) {
                    const float d = z - lp_dec(Y[tgt]);
                    atomicAdd(&sum[tgt], lp_fix(d));
                    cs += lp_fix(y - ym);
                    if constexpr (COST) {
                        lc_add(&csum[tgt], lc_fix(d, lc_ratio(ww, wmax)));
                        us += lc_fix(y - ym, lc_ratio(uu, umax));
                    }
                }
            }
        }
        if constexpr (COST) lp_wave_add(slot_us + par, us);
        const unsigned long long cst = lp_block_sum(slot_s + par, cs);
        const float lcs = lp_log(cst);
        const float ubar = COST && cst ? lc_val(slot_us[par], cst, umax) : 0.f;  // the cell's posterior mean of u
        lp_ahead3(u, nxt);
        // C
        lm = MM_NINF;
        float lcm = MM_NINF;
        {
            int q = 0;
            for (long long r = lo + tid; r < hi; r += NT, ++q) {
                const float y = q == 0 ? y0 : lp.post[r];
                const int tgt = q == 0 ? tgt0 : (y > MM_NINF ? lp_target(lp, u, r, false) : -1);
                const float pv = tgt >= 0 ? (y - ym) - lcs : MM_NINF;
                lp.post[r] = pv;
                if constexpr (COST) lc.diff[r] = tgt >= 0 ? expf(pv) * ((q == 0 ? u0 : lc.diff[r]) - ubar) : 0.f;
                if (tgt < 0) continue;
                const unsigned long long s = atomicExch(&sum[tgt], 0ull);
                if (s) {
                    const float v = lp_dec(Y[tgt]) + lp_log(s);
                    Y[tgt] = lp_enc(v);
                    lm = fmaxf(lm, v);
                    if constexpr (COST) {
                        const float c = lc_val(csum[tgt], s, wmax);
                        csum[tgt] = 0ll;
                        C[tgt] = c;
                        lcm = fmaxf(lcm, c);
                    }
                }
            }
            if (t == len - 1) {
                if (tid == 0) X[fin] = MM_LP_EMPTY;
            } else {
                q = 0;
                for (long long r = plo + tid; r < phi; r += NT, ++q) {
                    const int s = q == 0 ? ptgt : lp_target(lp, u, r, false);
                    if (s >= 0) X[s] = MM_LP_EMPTY;
                }
            }
        }
        if constexpr (COST) lp_wave_max(slot_c + par, lcm);
        const float Mn = lp_block_max(slot_m + par, lm);
        if (Mn > MM_NINF) {
            M = Mn;
            if constexpr (COST) Cm = lp_dec(slot_c[par]);
        } else
            alive = false;  // (cannot happen behind a forward pass that found a path; the records in front become -inf)
        unsigned *const sw = X;
        X = Y;
        Y = sw;
        plo = lo;
        phi = hi;
        ptgt = tgt0;
        cur = nxt;
        lp_ahead0(lp, costp, fcostp, u, cell0, t - 2, true, nxt);
    }
}

template <int NT>
__global__ void __launch_bounds__(NT) mm_latpost_fb_kernel(RunParams p, LatPostParams lp) {
    extern __shared__ __attribute__((aligned(16))) char lp_smem[];
    lp_fb<NT, false>(lp_smem, p, lp, LatCostParams{});
}
template <int NT>
__global__ void __launch_bounds__(NT) mm_latcost_fb_kernel(RunParams p, LatPostParams lp, LatCostParams lc) {
    extern __shared__ __attribute__((aligned(16))) char lp_smem[];
    lp_fb<NT, true>(lp_smem, p, lp, lc);
}

template <int NT>
__global__ void __launch_bounds__(NT) mm_latpost_gamma_kernel(RunParams p, LatPostParams lp) {
    extern __shared__ __attribute__((aligned(16))) char lp_smem[];
    unsigned long long *const acc = reinterpret_cast<unsigned long long *>(lp_smem);  // [P]
    const long long c = blockIdx.x;
    const int b = int(c / p.N), n = int(c - (long long)b * p.N), tid = threadIdx.x;
    const UttDesc &ud = p.utts[b];
    const int P = ud.P1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    float *const row = lp.gamma + (long long)b * lp.gsb + (long long)n * lp.gsn;
    for (int q = tid; q < P; q += NT) acc[q] = 0ull;
    __syncthreads();
    if (n < len) {
        LpUtt u;
        u.ld = lp.arcs + b;
        long long lo, hi;
        lp_cell(lp, c, lo, hi);
        for (long long r = lo + tid; r < hi; r += NT) {
            const float pr = lp.post[r];
            if (!(pr > MM_NINF)) continue;
            const int i = lp_target(lp, u, r, false);
            if (i < 0) continue;
            const int pdf = ud.s2p[i];
            if (pdf < P) atomicAdd(&acc[pdf], lp_fix(pr));
        }
    }
    __syncthreads();
    for (int q = tid; q < P; q += NT) row[q] = float(__ull2double_rn(acc[q]) * (1.0 / 1099511627776.0));
}

// the rows (b, n) of grad and of gamma, either of which may be NULL (not both: the launch is skipped then)
template <int NT>
__global__ void __launch_bounds__(NT) mm_latcost_grad_kernel(RunParams p, LatPostParams lp, LatCostParams lc) {
    extern __shared__ __attribute__((aligned(16))) char lp_smem[];
    unsigned *const slot = reinterpret_cast<unsigned *>(lp_smem);  // the cell's largest |diff|
    const long long c = blockIdx.x;
    const int b = int(c / p.N), n = int(c - (long long)b * p.N), tid = threadIdx.x;
    const UttDesc &ud = p.utts[b];
    const int P = ud.P1 - 1;
    unsigned long long *const accp = reinterpret_cast<unsigned long long *>(lp_smem + 16);  // [P] exp(post)
    long long *const accd = reinterpret_cast<long long *>(accp + P);                         // [P] diff / dmax
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const long long rowoff = (long long)b * lp.gsb + (long long)n * lp.gsn;
    for (int q = tid; q < P; q += NT) {
        accp[q] = 0ull;
        accd[q] = 0ll;
    }
    if (tid == 0) *slot = MM_LP_EMPTY;
    __syncthreads();
    LpUtt u;
    u.ld = lp.arcs + b;
    long long lo = 0, hi = 0;
    if (n < len) lp_cell(lp, c, lo, hi);
    float lm = MM_NINF;
    if (lc.grad)
        for (long long r = lo + tid; r < hi; r += NT)
            if (lp.post[r] > MM_NINF) lm = fmaxf(lm, fabsf(lc.diff[r]));
    const float dmax = lp_block_max(slot, lm);
    for (long long r = lo + tid; r < hi; r += NT) {
        const float pr = lp.post[r];
        if (!(pr > MM_NINF)) continue;
        const int i = lp_target(lp, u, r, false);
        if (i < 0) continue;
        const int pdf = ud.s2p[i];
        if (pdf >= P) continue;
        if (lp.gamma) atomicAdd(&accp[pdf], lp_fix(pr));
        if (lc.grad) lc_add(&accd[pdf], __float2ll_rn(lc_ratio(lc.diff[r], dmax) * MM_LP_ONE));
    }
    __syncthreads();
    for (int q = tid; q < P; q += NT) {
        if (lp.gamma) lp.gamma[rowoff + q] = float(__ull2double_rn(accp[q]) * (1.0 / 1099511627776.0));
        if (lc.grad) lc.grad[rowoff + q] = dmax > 0.f ? float(__ll2double_rn(accd[q]) * (1.0 / 1099511627776.0)) * dmax : 0.f;
    }
}

}  // namespace mm
