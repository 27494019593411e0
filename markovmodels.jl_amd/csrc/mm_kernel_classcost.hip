// mm_kernel_classcost.hip -- expected arc-class cost under the path posterior and its gradient (mm_classcost_f32; with
// A = -[class is the reference's class at that transition] over the denominator graph: lattice-free MPE / MWE) on the item form.
// Included by mm_classcost_tu.hip only.
//
// Under the class plan of mm_batch_set_arc_classes, with class costs A_b(t, c) on the len_b transitions (entry k_t leads from frame
// t + 1 to frame t + 2, 1-based frames; t = len_b - 1: the arc into the phony final state) and pdf costs D_b(n, p) as
// mm_expectedcost_f32 takes them (NULL: zeros):
//     A(pi)       = sum_{n=1..len} D(n, pdf(s_n)) + sum_{t=0..len-1} A(t, cls(k_t))
//     risk_b      = sum_pi P(pi | V_b) A(pi)
//     grad_b(n,p) = d risk_b / d V_b(n,p) = sum_{j : pdf(j) = p} gamma_n(j) (r_n(j) + s_n(j) - risk_b)
//     r_1(j) = D(1, pdf j)   r_n(j) = D(n, pdf j) + sum_{k into j} P(k | s_n = j, V_{1..n}) (r_{n-1}(i_k) + A(n-2, cls k)),   P(k | j) ~ alpha_{n-1}(i_k) T_hat[k]
//     s_{N+1} = 0            s_n(i) = sum_{k out of i} P(k | s_n = i, V) (A(n-1, cls k) + D(n+1, pdf j_k) + s_{n+1}(j_k)),     P(k | i) ~ T_hat[k] lhs_{n+1}(j_k) beta_{n+1}(j_k)
// This is the recursion of mm_kernel_cost.hip with one more term on every arc: the second operand of the 8-byte gather becomes
// v.y + arow[id] forward and t_{n+1}[j] + arow[id] backward, id the arc's class -- one LDS gather and one add per arc.
//
// mm_classcost_fwd_kernel   mm_cost_fwd_kernel's loop with the class term: alpha~, C_n, log2 Z, the r' store, O_n, risk
// mm_classcost_bwd_kernel   mm_cost_bwd_kernel's loop with the class term: gamma, grad, risk, ttl
// The loops are written out here (mm_kernel_cost.hip keeps its text and its bits); what the cost kernels' small parts do
// unchanged -- the LDS plan, the staging of D, the frames' means -- is taken from that file, the class ids of the resident items
// (ScoreIds, load_score_ids) and the clamped raw load of a row (score_load_raw) from mm_kernel_scored.hip.
//
// The class planes are the scored entry's (ScoredDev::plane): one 16-bit id per slot; an entry of class -1, the phony self-loop and
// every padding slot carry the id C.  The cost row of a transition: C + 1 floats in LDS padded as mm_scored_urow pads, double-buffered
// behind the cost kernels' LDS plan, fetched one step ahead; slot [C] holds 0, so no arc branches on its class.  Unlike the score
// row it is NOT scaled by log2 e: it is a value, not an exponent.  The forward step that forms frame n reads the row of transition
// n - 2, the backward step at frame n the row of transition n - 1; no row t >= len is fetched.
// Centring as in the cost kernels: the class term enters r and t before the frames' means are formed, so it is centred with the rest.
// A weight of zero meets only finite operands (A and D are finite where they are read): no NaN for finite costs.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"
#include "mm_kernel_cost.hip"    // cost_lds_plan, cost_load_raw, cost_value, stage_cost, frame_mean, frame_mean_put
#include "mm_kernel_scored.hip"  // ScoreIds, load_score_ids, score_load_raw

namespace mm {

// where both kernels keep the two cost rows: behind the cost kernels' plan
__device__ __forceinline__ float *classcost_rows(float *lds, const CostLds &L) { return lds + L.total; }

// the cost row of transition t (stage_score / stage_score_ahead without the scaling)
__device__ __forceinline__ void stage_arow(float *dst, const float *Ab, long long asn, long long asc, int t, int C, int from, int NT) {
    for (int q = from; q < C; q += NT) dst[q] = Ab[(long long)t * asn + (long long)q * asc];
}
__device__ __forceinline__ void stage_arow_ahead(float *dst, float raw, const float *Ab, long long asn, long long asc, int t, int C, int tid, int NT) {
    if (tid < C) dst[tid] = raw;
    if (C > NT) stage_arow(dst, Ab, asn, asc, t, C, tid + NT, NT);
}
// the pdf costs: D NULL costs nothing and is not read
__device__ __forceinline__ float classcost_load_d(const float *Db, long long dsn, int n, int len, int P, int q) {
    return Db ? cost_load_raw(Db, dsn, n, len, P, q) : 0.f;
}
__device__ __forceinline__ void classcost_stage_d(float *dst, const float *Db, long long dsn, int n, int len, int P, int tid, int NT) {
    if (Db) stage_cost(dst, Db, dsn, n, len, P, tid, NT);
    else
        for (int q = tid; q <= P; q += NT) dst[q] = 0.f;
}

// for_items_pair (mm_kernel_cost.hip) with the class term: the mean is that of a[col_k].y + ar[id_k] under the weights of the
// log-sum-exp.  Resident items take their ids from si, streamed items and long rows from the plane beside their slots.
template <int NI, class Epi>
__device__ __forceinline__ void for_items_pair_class(const ItemRegs<NI> &rg, const ScoreIds<NI> &si, const GraphDev &g, const unsigned short *plane,
                                                     int wave, int NW, int lane, const float2 *a, const float *emn, const float *csn, const float *ar,
                                                     Epi &&epi) {
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
            const unsigned i01 = si.id[i][0], i23 = si.id[i][1];
            const float2 v0 = a[c01 & 0xffffu], v1 = a[c01 >> 16];
            const float y0 = v0.y + ar[i01 & 0xffffu], y1 = v1.y + ar[i01 >> 16];
            const float x0 = rg.w[i][0] + v0.x, x1 = rg.w[i][1] + v1.x;
            float x2 = MM_NINF, x3 = MM_NINF, y2 = 0.f, y3 = 0.f;
            if (R > 2) {
                const float2 v2 = a[c23 & 0xffffu], v3 = a[c23 >> 16];
                x2 = rg.w[i][2] + v2.x;
                x3 = rg.w[i][3] + v3.x;
                y2 = v2.y + ar[i23 & 0xffffu];
                y3 = v3.y + ar[i23 >> 16];
            }
            float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
            m = grp_max_rt(m, lg);
            const float m0 = (m > MM_NINF) ? m : 0.f;
            const float e0 = fast_exp2(x0 - m0), e1 = fast_exp2(x1 - m0);
            float sum = e0 + e1, num = fmaf(e1, y1, e0 * y0);
            if (R > 2) {
                const float e2 = fast_exp2(x2 - m0), e3 = fast_exp2(x3 - m0);
                sum += e2 + e3;
                num += fmaf(e3, y3, e2 * y2);
            }
            sum = grp_sum_rt(sum, lg);
            num = grp_sum_rt(num, lg);
            if (real && (lane & ((1 << lg) - 1)) == 0)
                epi(m0 + fast_log2(sum), sum > 0.f ? num * __builtin_amdgcn_rcpf(sum) : 0.f, (int)row, (int)pdf, e, c);
        }
    });
    // items beyond the register window, and long rows: streamed from L2, the plane beside the slots
    const int resident = NI * NW < g.n_short ? NI * NW : g.n_short;
    for (int it = wave; it < g.n_items; it += NW) {
        if (it < resident) continue;
        const ItemMeta im = load_item(g.items, it);
        const RowInfo r = g.rowinfo[(size_t)it * 64 + lane];
        const int pdf = r.row >= 0 ? r.pdf : 0;
        const float e = emn[pdf], c = csn[pdf];
        const Slot *sp = g.slots + (size_t)im.slot_row * 64 + lane;
        const unsigned short *ip = plane + (size_t)im.slot_row * 64 + lane;
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
                    vy[k] = v.y + ar[ip[k * 64]];
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
        } else {  // long rows: two passes over the row's slots (a padding slot: the weight -inf, the id C)
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
                num = fmaf(ek, v.y + ar[ip[k * 64]], num);
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
__global__ void __launch_bounds__(512) mm_classcost_fwd_kernel(RunParams p, ClassCostParams cp) {
    extern __shared__ float4 classcost_lds4[];
    float *lds = reinterpret_cast<float *>(classcost_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const CostLds L = cost_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *cs = lds + L.cs, *part = lds + L.part, *psum = lds + L.psum;
    float *ar = classcost_rows(lds, L);  // [2][UR]
    float *big = BIGV ? cp.ws_big + (long long)b * cp.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    const float *Db = cp.D ? cp.D + (long long)b * cp.dsb : nullptr;
    const float *Ab = cp.A + (long long)b * cp.asb;
    const unsigned short *plane = cp.sc[b].plane[0];
    const int NC = cp.C, UR = cp.urow;
    float *wsR = cp.ws_r + u.s1p_prefix * (long long)(p.N + 1);
    double *wsO = cp.ws_o + (long long)b * (p.N + 2);
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, MM_LOG2E);
    classcost_stage_d(cs + 1 * P1p, Db, cp.dsn, 1, len, P, tid, NT);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    for (int q = tid; q < 2 * UR; q += NT) ar[q] = 0.f;
    vsync();
    {   // frame 1: alpha_hat (*) lhs[:,1], r_1 = the frame's pdf cost
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
            classcost_stage_d(cs + 0 * P1p, Db, cp.dsn, 2, len, P, tid, NT);
            stage_arow(ar, Ab, cp.asn, cp.asc, 0, NC, tid, NT);  // transition 0 (step 2)
        }
        if (tid == 0) {
            wsC[1] = 0.0;
            wsO[1] = 0.0;
        }
    }
    vsync();
    ItemRegs<NI> rg;
    ScoreIds<NI> si;
    load_item_regs<NI>(rg, u.g[0], wave, NW, lane);
    load_score_ids<NI>(si, u.g[0], plane, NC, wave, NW, lane);
    const GraphDev gf = u.g[0];
    double C = 0.0, O = 0.0;
    // emissions, pdf costs and the cost row travel one step ahead in a register (as in mm_cost_fwd_kernel / mm_scored_fwd_kernel)
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    float cvp = len >= 1 ? classcost_load_d(Db, cp.dsn, 3, len, P, tid) : 0.f;
    float avp = len >= 1 ? score_load_raw(Ab, cp.asn, cp.asc, 1, len - 1, NC, tid) : 0.f;
    const int n4 = S1p >> 2;
    for (int n = 2; n <= NF; ++n) {
        const float2 *ap = buf + ((n - 1) & 1) * S1p;
        float2 *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p, *csn = cs + (n & 1) * P1p;
        const float *arn = ar + (n & 1) * UR;  // transition n - 2
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
            if (P >= NT) classcost_stage_d(cs + ((n + 1) & 1) * P1p + NT, Db ? Db + NT : nullptr, cp.dsn, n + 1, len, P - NT, tid, NT);
            stage_arow_ahead(ar + ((n + 1) & 1) * UR, avp, Ab, cp.asn, cp.asc, n - 1, NC, tid, NT);  // (n - 1 <= len - 1)
        }
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        cvp = classcost_load_d(Db, cp.dsn, n + 2, len, P, tid);
        avp = score_load_raw(Ab, cp.asn, cp.asc, n, len - 1, NC, tid);
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
        for_items_pair_class<NI>(rg, si, gf, plane, wave, NW, lane, ap, emn, csn, arn,
                                 [&](float v, float rbar, int row, int pdf, float e, float c) {
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
        wsO[0] = (double)last.y + O;  // risk: r_{len+1}(final), the pdf cost of frame len + 1 being 0
    }
}

// backward: gamma, grad, risk, ttl.  Same grid and block as the forward kernel.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_classcost_bwd_kernel(RunParams p, ClassCostParams cp) {
    extern __shared__ float4 classcost_lds4[];
    float *lds = reinterpret_cast<float *>(classcost_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const CostLds L = cost_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *cs = lds + L.cs, *part = lds + L.part, *psum = lds + L.psum;
    float *ar = classcost_rows(lds, L);  // [2][UR]
    float *big = BIGV ? cp.ws_big + (long long)b * cp.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    const float *Db = cp.D ? cp.D + (long long)b * cp.dsb : nullptr;
    const float *Ab = cp.A + (long long)b * cp.asb;
    const unsigned short *plane = cp.sc[b].plane[1];
    const int NC = cp.C, UR = cp.urow;
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
    for (long long q = tid; q < (long long)(p.N - z0) * P; q += NT) {
        const long long o = gbase + (z0 + q / P) * cp.gsn + (q % P) * cp.gsp;
        cp.grad[o] = 0.f;
        if (cp.gamma) cp.gamma[o] = 0.f;
    }
    if (!ok || len < 1) return;

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    for (int q = tid; q < 2 * UR; q += NT) ar[q] = 0.f;
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = make_float2(0.f, 0.f);  // frame len + 1: the final state alone, nothing to come
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    classcost_stage_d(cs + (len & 1) * P1p, Db, cp.dsn, len, len, P, tid, NT);
    stage_arow(ar + ((len - 1) & 1) * UR, Ab, cp.asn, cp.asc, len - 1, NC, tid, NT);  // transition len - 1 (step len)
    copy_row_pair(sta + (len & 1) * S1p, wsA + (long long)len * S1p, str + (len & 1) * S1p, wsR + (long long)len * S1p, S1p >> 2, tid, NT);
    vsync();
    ItemRegs<NI> rg;
    ScoreIds<NI> si;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    load_score_ids<NI>(si, gb, plane, NC, wave, NW, lane);
    double D = 0.0, Q = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f, cvp = 0.f, avp = 0.f;
    double Cn = wsC[len], On = wsO[len], Cpre = 0.0, Opre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions, pdf costs, the cost row of the transition out of it, C_f and O_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        cvp = classcost_load_d(Db, cp.dsn, f, len, P, tid);
        avp = score_load_raw(Ab, cp.asn, cp.asc, f - 1, len - 1, NC, tid);
        Cpre = wsC[f];
        Opre = wsO[f];
    };
    // gamma and grad of frame f from its per-pdf sums (one wave), as mm_cost_bwd_kernel: the frame's posterior mean of
    // r + s - risk (zero in exact arithmetic) is taken out
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
        const float *arn = ar + ((n - 1) & 1) * UR;  // transition n - 1: frame n -> frame n + 1
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        // posterior mean of t' of frame n + 1
        const float mu = (n == len) ? 0.f : frame_mean(psum + ((n + 1) & 1) * 2 * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        Q += (double)mu;  // = Q_n: s_n = s'_n + Q_n
        const float kappa = (float)(logZ2 - Cn - D);
        const float off = (float)(On + Q - risk);  // E[A | s_n = j] - risk = r'_n(j) + s'_n(j) + off
        if (n < len && wave == NW - 1) finalise(n + 1);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_cost_bwd_kernel)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            if (tid <= P) cs[((n - 1) & 1) * P1p + tid] = cost_value(cvp, n - 1, len, P, tid);
            if (P >= NT) classcost_stage_d(cs + ((n - 1) & 1) * P1p + NT, Db ? Db + NT : nullptr, cp.dsn, n - 1, len, P - NT, tid, NT);
            stage_arow_ahead(ar + (n & 1) * UR, avp, Ab, cp.asn, cp.asc, n - 2, NC, tid, NT);  // transition n - 2 (step n - 1)
            stage_row_pair<BIGV>(sta + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, str + ((n - 1) & 1) * S1p,
                                 wsR + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            On = Opre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        float wm = MM_NINF, sq = 0.f, sqt = 0.f;
        for_items_pair_class<NI>(rg, si, gb, plane, wave, NW, lane, yp, emn, csn, arn,
                                 [&](float v, float tbar, int row, int pdf, float e, float c) {
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
        // per pdf, over the pdf's states in pdf_rows: a fixed order, no atomics.  The second barrier also guards the staging buffers.
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
