// mm_kernel_cost.hip -- expected path cost under the path posterior and its gradient (mm_expectedcost_f32; with
// cost = -[pdf is the reference alignment's pdf] over the denominator graph: lattice-free sMBR) on the item form.
// Included by mm_cost_tu.hip only.
//
// For utterance b with costs cost_b(n, p) on the len_b real frames and the P real pdfs (the phony pdf costs 0):
//     A(pi)       = sum_{n=1..len_b} cost_b(n, pdf(s_n))                 for a complete state sequence pi = s_1 .. s_{N+1}
//     risk_b      = sum_pi P(pi | V_b) A(pi)
//     grad_b(n,p) = d risk_b / d V_b(n,p) = sum_{j : pdf(j) = p} gamma_n(j) (E[A | s_n = j] - risk_b)
// E[A | s_n = j] = r_n(j) + s_n(j), two conditional expectations that ride on the alpha- and the beta-recursion:
//     r_1(j) = cost(1, pdf j)    r_n(j) = cost(n, pdf j) + sum_i P(s_{n-1} = i | s_n = j, V_{1..n}) r_{n-1}(i),   P(i | j) ~ alpha_{n-1}(i) T_ij
//     s_{N+1} = 0                s_n(i) = sum_j P(s_{n+1} = j | s_n = i, V) (cost(n+1, pdf j) + s_{n+1}(j)),      P(j | i) ~ T_ij lhs_{n+1}(j) beta_{n+1}(j)
// Both are convex combinations with the very weights 2^(x - m) the log-sum-exp of a row forms anyway, so each arc costs one more
// gathered operand and one FMA, each row one more group sum and one reciprocal.  The vector an arc gathers from holds 8-byte
// entries -- {alpha~, r} forward, {y = beta~ + e, t = cost + s} backward -- so the second operand rides on the same LDS access.
//
// mm_cost_fwd_kernel   alpha~, C_n and log2 Z exactly as mm_log_kernel<MODE_FB, NI, 1> leaves them, plus the r store and risk_b
// mm_cost_bwd_kernel   PASS 2's beta~ recursion carrying t; per state the posterior q and q (r + s - risk) written over the staged
//                      alpha~ / r rows, per pdf their sums through the pdf_rows lists (8 lanes per pdf, fixed order, no atomics: the
//                      same bits on every run), then gamma = sum q / frame sum, grad = sum q (r + s - risk) / frame sum with the
//                      frame's posterior mean of r + s - risk (zero in exact arithmetic) taken out
//
// Numerics.  r grows like the path's cost so far, s like the cost still to come, while the gradient needs r + s - risk, a few
// units.  Both are therefore carried CENTRED: r'_n = r_n - O_n, t'_n = t_n - Q_n, where O_n adds up the filtering means of r' of the
// frames before n and Q_n the posterior means of t' of the frames after n (one frame late, like the lagged maximum that
// normalises alpha~: the mean of a frame is known when the next one starts).  O_n and Q_n are float64, one per utterance and frame;
// they meet the float32 values only where risk_b = r'_{len+1}(final) + O_{len+1} and r' + s' + (O_n + Q_n - risk_b) are formed.
// Any offsets would do for exactness; the means keep the float32 values near zero.  A state no path reaches has weight zero in
// every sum it enters and carries r' = t' = 0 (0 / 0 := 0), so a finite cost never meets an infinity.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

// LDS carve of both kernels, in floats (the pair vectors first: 8-byte aligned)
struct CostLds {
    int buf, sta, str, em, cs, bins, gbins, part, psum, total;
};
__host__ __device__ inline CostLds cost_lds_plan(int S1p, int P1p) {
    CostLds l;
    l.buf = 0;                  // [2][S1p] pairs
    l.sta = l.buf + 4 * S1p;    // [2][S1p] alpha~ of a frame, then its state posteriors (backward)
    l.str = l.sta + 2 * S1p;    // [2][S1p] r' of a frame, then q (r + s - risk) (backward)
    l.em = l.str + 2 * S1p;     // [2][P1p] emissions
    l.cs = l.em + 2 * P1p;      // [2][P1p] costs
    l.bins = l.cs + 2 * P1p;    // [2][P1p] per-pdf sums of q
    l.gbins = l.bins + 2 * P1p; // [2][P1p] per-pdf sums of q (r + s - risk)
    l.part = l.gbins + 2 * P1p; // [2][MM_MAX_WAVES] the waves' maxima
    l.psum = l.part + 2 * MM_MAX_WAVES;  // [2][2][MM_MAX_WAVES] the waves' two sums behind a frame's mean
    l.total = l.psum + 4 * MM_MAX_WAVES;
    return l;
}

__device__ __forceinline__ float cost_load_raw(const float *Cb, long long csn, int n, int len, int P, int q) {
    // frames 1 .. len only (len >= 1): what lies beyond the length is never read
    const int nn = n < 1 ? 1 : (n > len ? len : n), qq = q < P ? q : P - 1;
    return Cb[(long long)(nn - 1) * csn + qq];
}
__device__ __forceinline__ float cost_value(float raw, int n, int len, int P, int q) { return (q < P && n <= len) ? raw : 0.f; }
__device__ __forceinline__ void stage_cost(float *dst, const float *Cb, long long csn, int n, int len, int P, int tid, int NT) {
    for (int q = tid; q <= P; q += NT) dst[q] = (q < P && n <= len) ? Cb[(long long)(n - 1) * csn + q] : 0.f;
}

// mean = (sum of weight x value) / (sum of weights) of the frame whose partials are at ps; 0 where no weight is left
__device__ __forceinline__ float frame_mean(const float *ps, int NW, int lane) {
    const float sw = part_sum(ps, NW, lane), swv = part_sum(ps + MM_MAX_WAVES, NW, lane);
    const float m = swv * __builtin_amdgcn_rcpf(sw);
    return (sw > 0.f && fabsf(m) < 1e30f) ? m : 0.f;
}
__device__ __forceinline__ void frame_mean_put(float *ps, int wave, int lane, float sw, float swv) {
    sw = wave_sum(sw);
    swv = wave_sum(swv);
    if (lane == 0) {
        ps[wave] = sw;
        ps[MM_MAX_WAVES + wave] = swv;
    }
}

// Every item of this wave over a vector of pairs `a`: the log-sum-exp of w_k + a[col_k].x and, with the same weights, the mean of
// a[col_k].y (0 for a row without weight).  epi(lse, mean, row, pdf, e, c) runs on the leader lane of each row group; e, c: the
// row's emission and cost, fetched before the arithmetic.
template <int NI, class Epi>
__device__ __forceinline__ void for_items_pair(const ItemRegs<NI> &rg, const GraphDev &g, int wave, int NW, int lane, const float2 *a,
                                               const float *emn, const float *csn, Epi &&epi) {
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int meta = rg.meta[i];
        if (meta != 0) {
            int R = meta & 0xff, lg = meta >> 8;
            asm volatile("" : "+s"(R), "+s"(lg));  // (opaque per frame: see for_items)
            const unsigned row = rg.ri[i] & 0xffffu;
            const bool real = row != 0xffffu;
            const unsigned pdf = real ? (rg.ri[i] >> 16) : 0u;
            const float e = emn[pdf], c = csn[pdf];
            const unsigned c01 = rg.c[i][0], c23 = rg.c[i][1];
            const float2 v0 = a[c01 & 0xffffu], v1 = a[c01 >> 16];
            const float x0 = rg.w[i][0] + v0.x, x1 = rg.w[i][1] + v1.x;
            float x2 = MM_NINF, x3 = MM_NINF;
            float2 v2 = make_float2(0.f, 0.f), v3 = v2;
            if (R > 2) {
                v2 = a[c23 & 0xffffu];
                v3 = a[c23 >> 16];
                x2 = rg.w[i][2] + v2.x;
                x3 = rg.w[i][3] + v3.x;
            }
            float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
            m = grp_max_rt(m, lg);
            const float m0 = (m > MM_NINF) ? m : 0.f;
            const float e0 = fast_exp2(x0 - m0), e1 = fast_exp2(x1 - m0);
            float sum = e0 + e1, num = fmaf(e1, v1.y, e0 * v0.y);
            if (R > 2) {
                const float e2 = fast_exp2(x2 - m0), e3 = fast_exp2(x3 - m0);
                sum += e2 + e3;
                num += fmaf(e3, v3.y, e2 * v2.y);
            }
            sum = grp_sum_rt(sum, lg);
            num = grp_sum_rt(num, lg);
            if (real && (lane & ((1 << lg) - 1)) == 0)
                epi(m0 + fast_log2(sum), sum > 0.f ? num * __builtin_amdgcn_rcpf(sum) : 0.f, (int)row, (int)pdf, e, c);
        }
    });
    // items beyond the register window, and long rows: streamed from L2
    const int resident = NI * NW < g.n_short ? NI * NW : g.n_short;
    for (int it = wave; it < g.n_items; it += NW) {
        if (it < resident) continue;
        const ItemMeta im = load_item(g.items, it);
        const RowInfo r = g.rowinfo[(size_t)it * 64 + lane];
        const int pdf = r.row >= 0 ? r.pdf : 0;
        const float e = emn[pdf], c = csn[pdf];
        const Slot *sp = g.slots + (size_t)im.slot_row * 64 + lane;
        const int R = im.R, lg = im.log2g;
        float sum = 0.f, num = 0.f, m0;
        if (R <= 4) {  // one pass: the row's terms stay in registers
            float x[4], vy[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = MM_NINF;
                vy[k] = 0.f;
                if (k < R) {
                    const Slot s = load_slot(sp + k * 64);
                    const float2 v = a[s.col];
                    x[k] = s.w + v.x;
                    vy[k] = v.y;
                }
            }
            const float m = grp_max_rt(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), lg);
            m0 = (m > MM_NINF) ? m : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float ek = fast_exp2(x[k] - m0);
                sum += ek;
                num = fmaf(ek, vy[k], num);
            }
        } else {  // long rows: two passes over the row's slots
            float m = MM_NINF;
            for (int k = 0; k < R; ++k) {
                const Slot s = load_slot(sp + k * 64);
                m = fmaxf(m, s.w + a[s.col].x);
            }
            m = grp_max_rt(m, lg);
            m0 = (m > MM_NINF) ? m : 0.f;
            for (int k = 0; k < R; ++k) {
                const Slot s = load_slot(sp + k * 64);
                const float2 v = a[s.col];
                const float ek = fast_exp2(s.w + v.x - m0);
                sum += ek;
                num = fmaf(ek, v.y, num);
            }
        }
        sum = grp_sum_rt(sum, lg);
        num = grp_sum_rt(num, lg);
        if (r.row >= 0 && (lane & ((1 << lg) - 1)) == 0)
            epi(m0 + fast_log2(sum), sum > 0.f ? num * __builtin_amdgcn_rcpf(sum) : 0.f, r.row, pdf, e, c);
    }
}

// forward: alpha~ rows, C_n, log2 Z (wsC[0]) as the item kernel's forward half, the r' rows, O_n, risk (wsO[0]).
// grid = B workgroups (one utterance each), block = 64 * NW threads, NW <= 8.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_cost_fwd_kernel(RunParams p, CostParams cp) {
    extern __shared__ float4 cost_lds4[];
    float *lds = reinterpret_cast<float *>(cost_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const CostLds L = cost_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *cs = lds + L.cs, *part = lds + L.part, *psum = lds + L.psum;
    float *big = BIGV ? cp.ws_big + (long long)b * cp.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    const float *Cb = cp.cost + (long long)b * cp.csb;
    float *wsR = cp.ws_r + u.s1p_prefix * (long long)(p.N + 1);
    double *wsO = cp.ws_o + (long long)b * (p.N + 2);
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, MM_LOG2E);
    stage_cost(cs + 1 * P1p, Cb, cp.csn, 1, len, P, tid, NT);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    vsync();
    {   // frame 1: alpha_hat (*) lhs[:,1], r_1 = the frame's cost
        float wm = MM_NINF, sw = 0.f, swv = 0.f;
        float2 *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p, *c1 = cs + 1 * P1p;
        for (int s = tid; s < S1; s += NT) {
            const int pdf = u.s2p[s];
            const float v = u.init[s] + e1[pdf], r = c1[pdf];
            a1[s] = make_float2(v, r);
            wm = fmaxf(wm, v);
            const float wgt = fast_exp2(v);
            sw += wgt;
            swv = fmaf(wgt, r, swv);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        frame_mean_put(psum + 1 * 2 * MM_MAX_WAVES, wave, lane, sw, swv);
        if (NF >= 2) {
            stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, MM_LOG2E);
            stage_cost(cs + 0 * P1p, Cb, cp.csn, 2, len, P, tid, NT);
        }
        if (tid == 0) {
            wsC[1] = 0.0;
            wsO[1] = 0.0;
        }
    }
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, u.g[0], wave, NW, lane);
    const GraphDev gf = u.g[0];
    double C = 0.0, O = 0.0;
    // emissions and costs travel one frame ahead in a register (as in mm_log_kernel)
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    float cvp = len >= 1 ? cost_load_raw(Cb, cp.csn, 3, len, P, tid) : 0.f;
    const int n4 = S1p >> 2;
    for (int n = 2; n <= NF; ++n) {
        const float2 *ap = buf + ((n - 1) & 1) * S1p;
        float2 *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p, *csn = cs + (n & 1) * P1p;
        const float M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        const float mu = frame_mean(psum + ((n - 1) & 1) * 2 * MM_MAX_WAVES, NW, lane);  // filtering mean of r' of frame n - 1
        C += (double)M;
        O += (double)mu;
        if (tid == 0) {
            wsC[n] = C;
            wsO[n] = O;
        }
        if (n + 1 <= NF) {
            stage_em_ahead<em_value>(em + ((n + 1) & 1) * P1p, evp, Vb, p.vsn, n + 1, len, P, tid, NT, MM_LOG2E);
            if (tid <= P) cs[((n + 1) & 1) * P1p + tid] = cost_value(cvp, n + 1, len, P, tid);
            if (P >= NT) stage_cost(cs + ((n + 1) & 1) * P1p + NT, Cb + NT, cp.csn, n + 1, len, P - NT, tid, NT);
        }
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        cvp = cost_load_raw(Cb, cp.csn, n + 2, len, P, tid);
        {   // frame n - 1 leaves the chip once, the pairs taken apart: alpha~ rows as the item kernel stores them, r' rows beside
            const float4 *src = reinterpret_cast<const float4 *>(ap);
            float4 *da = reinterpret_cast<float4 *>(wsA + (long long)(n - 1) * S1p);
            float4 *dr = reinterpret_cast<float4 *>(wsR + (long long)(n - 1) * S1p);
            for (int q = tid; q < n4; q += NT) {
                const float4 lo = src[2 * q], hi = src[2 * q + 1];
                da[q] = make_float4(lo.x, lo.z, hi.x, hi.z);
                dr[q] = make_float4(lo.y, lo.w, hi.y, hi.w);
            }
        }
        float wm = MM_NINF, sw = 0.f, swv = 0.f;
        for_items_pair<NI>(rg, gf, wave, NW, lane, ap, emn, csn, [&](float v, float rbar, int row, int pdf, float e, float c) {
            v = v + e - M;
            const float r = v > MM_NINF ? c + rbar - mu : 0.f;
            an[row] = make_float2(v, r);
            wm = max_nc(wm, v);
            const float wgt = fast_exp2(v);
            sw += wgt;
            swv = fmaf(wgt, r, swv);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        frame_mean_put(psum + (n & 1) * 2 * MM_MAX_WAVES, wave, lane, sw, swv);
        vsync();
    }
    if (tid == 0) {
        const float2 last = buf[(NF & 1) * S1p + fstate];
        wsC[0] = (double)last.x + C;  // log2 Z
        wsO[0] = (double)last.y + O;  // risk: r_{len+1}(final), the cost of frame len + 1 being 0
    }
}

// backward: gamma, grad, risk, ttl.  Same grid and block as the forward kernel.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_cost_bwd_kernel(RunParams p, CostParams cp) {
    extern __shared__ float4 cost_lds4[];
    float *lds = reinterpret_cast<float *>(cost_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const CostLds L = cost_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *cs = lds + L.cs, *part = lds + L.part, *psum = lds + L.psum;
    float *big = BIGV ? cp.ws_big + (long long)b * cp.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    const float *Cb = cp.cost + (long long)b * cp.csb;
    float *wsR = cp.ws_r + u.s1p_prefix * (long long)(p.N + 1);
    double *wsO = cp.ws_o + (long long)b * (p.N + 2);
    float *bins = lds + L.bins, *gbins = lds + L.gbins;
    float *sta = BIGV ? big + 4 * S1p : lds + L.sta;
    float *str = BIGV ? big + 6 * S1p : lds + L.str;
    const GraphDev gb = u.g[1];
    const double logZ2 = wsC[0], risk = wsO[0];
    const long long gbase = (long long)b * cp.gsb;
    const bool ok = logZ2 > -1e300;
    if (tid == 0) {
        cp.risk[b] = ok ? (float)risk : 0.f;
        if (cp.ttl) cp.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    }
    // frames without a result: all of them without an accepting path, else those beyond the length
    const int z0 = ok ? len : 0;
    // (not zero_gamma_from: two outputs on one walk, its 64-bit index arithmetic once)
    for (long long q = tid; q < (long long)(p.N - z0) * P; q += NT) {
        const long long o = gbase + (z0 + q / P) * cp.gsn + (q % P) * cp.gsp;
        cp.grad[o] = 0.f;
        if (cp.gamma) cp.gamma[o] = 0.f;
    }
    if (!ok || len < 1) return;

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = make_float2(0.f, 0.f);  // frame len + 1: the final state alone, nothing to come
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    stage_cost(cs + (len & 1) * P1p, Cb, cp.csn, len, len, P, tid, NT);
    copy_row_pair(sta + (len & 1) * S1p, wsA + (long long)len * S1p, str + (len & 1) * S1p, wsR + (long long)len * S1p, S1p >> 2, tid, NT);
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0, Q = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f, cvp = 0.f;
    double Cn = wsC[len], On = wsO[len], Cpre = 0.0, Opre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions, costs, C_f and O_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        cvp = cost_load_raw(Cb, cp.csn, f, len, P, tid);
        Cpre = wsC[f];
        Opre = wsO[f];
    };
    // gamma and grad of frame f from its per-pdf sums (one wave).  Not finalise_gamma: two sums per pdf, the second with the frame's mean taken out
    auto finalise = [&](int f) {
        const float *bf = bins + (f & 1) * P1p, *gf = gbins + (f & 1) * P1p;
        float s = 0.f, gs = 0.f;
        for (int q = lane; q < P1; q += 64) {
            s += bf[q];
            gs += gf[q];
        }
        s = wave_sum(s);
        gs = wave_sum(gs);
        const float inv = s > 0.f ? 1.f / s : 0.f;
        // E[A | s_n] - risk has posterior mean zero (law of total expectation): what the frame's sum of q (r + s - risk) is left
        // with is the rounding all states of the frame share -- of risk, and of r' and s' along their common history -- and is
        // taken out, so sum_p grad(n, p) = 0 holds to the rounding of this line
        const float mean = gs * inv;
        const long long o = gbase + (long long)(f - 1) * cp.gsn;
        for (int q = lane; q < P; q += 64) {
            cp.grad[o + q * cp.gsp] = (gf[q] - bf[q] * mean) * inv;
            if (cp.gamma) cp.gamma[o + q * cp.gsp] = bf[q] * inv;
        }
    };
    if (len >= 2) prefetch(len - 1);
    for (int n = len; n >= 1; --n) {
        const float2 *yp = buf + ((n + 1) & 1) * S1p;
        float2 *yn = buf + (n & 1) * S1p;
        float *ast = sta + (n & 1) * S1p;  // alpha~ of frame n, replaced by the state posteriors as they are made
        float *rst = str + (n & 1) * S1p;  // r' of frame n, replaced by q (r + s - risk)
        const float *emn = em + (n & 1) * P1p, *csn = cs + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        // posterior mean of t' of frame n + 1
        const float mu = (n == len) ? 0.f : frame_mean(psum + ((n + 1) & 1) * 2 * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        Q += (double)mu;  // = Q_n: s_n = s'_n + Q_n
        const float kappa = (float)(logZ2 - Cn - D);
        const float off = (float)(On + Q - risk);  // E[A | s_n = j] - risk = r'_n(j) + s'_n(j) + off
        if (n < len && wave == NW - 1) finalise(n + 1);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            if (tid <= P) cs[((n - 1) & 1) * P1p + tid] = cost_value(cvp, n - 1, len, P, tid);
            if (P >= NT) stage_cost(cs + ((n - 1) & 1) * P1p + NT, Cb + NT, cp.csn, n - 1, len, P - NT, tid, NT);
            stage_row_pair<BIGV>(sta + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, str + ((n - 1) & 1) * S1p,
                                 wsR + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            On = Opre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        float wm = MM_NINF, sq = 0.f, sqt = 0.f;
        for_items_pair<NI>(rg, gb, wave, NW, lane, yp, emn, csn, [&](float v, float tbar, int row, int pdf, float e, float c) {
            const float beta = v - M;  // T (B[:,n+1] (*) lhs[:,n+1])
            const float q = fast_exp2(ast[row] + beta - kappa);  // state posterior
            const float s = beta > MM_NINF ? tbar - mu : 0.f;    // s'_n
            const float d = rst[row] + s + off;
            ast[row] = q;
            rst[row] = q > 0.f ? q * d : 0.f;
            const float t = c + s;
            yn[row] = make_float2(beta + e, t);
            wm = max_nc(wm, beta + e);
            sq += q;
            sqt = fmaf(q, t, sqt);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        frame_mean_put(psum + (n & 1) * 2 * MM_MAX_WAVES, wave, lane, sq, sqt);
        stage_row_wait<BIGV>();  // this wave's part of frame n - 1 is in LDS
        vsync();
        // per pdf, over the pdf's states in pdf_rows: 8 lanes add the two products in a fixed order, a 3-step DPP reduction ends
        // it (mm_log_kernel's deterministic mode).  The second barrier also guards the staging buffers.
        for_pdf_rows<2>(u, P1, wave, NW, lane, {bins + (n & 1) * P1p, gbins + (n & 1) * P1p}, [](int) { return 0; },
                        [&](int row, int, float(&acc)[2]) {
                            acc[0] += ast[row];
                            acc[1] += rst[row];
                        });
        vsync();
    }
    if (wave == 0) finalise(1);
}

}  // namespace mm
