// mm_kernel_scored.hip -- posteriors with per-frame arc-class scores and their gradient (mm_scoredposteriors_f32) on the item form.
// Included by mm_scored_tu.hip only.
//
// A path's weight is alpha_hat * prod lhs * prod_t T_hat[k_t] * exp(U[b, t, cls(k_t)]): the entry k_t taken between frames t + 1 and
// t + 2 (1-based frames, 0-based t) is scored by the row t of U at the class mm_batch_set_arc_classes gave it.  Two launches:
//   mm_scored_fwd_kernel   mm_log_kernel<MODE_FB,NI,1>'s forward loop with the scored gather: every arc does w + a[col] + urow[id].
//                          It leaves alpha~, C_n and log2 Z in the workspace as the item kernel's forward half does.
//   mm_scored_bwd_kernel   mm_arcclass_kernel's loop -- the same ranks and ClassRec records, the same class_pass, the same two
//                          placements of the term rows -- with the score in the beta~ recursion and in every classified entry's
//                          term, and mm_window_bwd_kernel's pass over the pdf -> states lists behind a barrier of its own: it forms
//                          the state posteriors, adds the emissions to beta~ and sums the posteriors per pdf (8 lanes per pdf, a
//                          fixed order) for gamma.  The pass runs whether gamma is asked for or not: its sums are the frame's
//                          correction of kappa, so gamma only, xi only and ttl only give the bits of the full call.
// The class plane: one 16-bit class id per slot of an item form, parallel to GraphDev::slots (ScoredDev::plane); an entry without
// a class, the phony self-loop and every padding slot carry the id C.  Register-resident items hold their four ids in two more
// registers (ScoreIds) beside ItemRegs::c, streamed items read the plane beside their slots.
// The score row of a transition: C + 1 floats in LDS, double-buffered, scaled by log2 e, fetched one step ahead as the emissions
// are; its slot [C] holds 0, so no arc branches on its class.  U NULL: both rows stay zero and nothing is fetched.
// -inf + -inf is the only sum of infinities these kernels form: no NaN for finite or -inf inputs.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"
#include "mm_kernel_arcclass.hip"  // class_pass, MM_CLASS_UNROLL

namespace mm {

template <int NI>
struct ScoreIds {
    unsigned id[NI > 0 ? NI : 1][2];  // id0 | id1 << 16, id2 | id3 << 16 (a slot the item does not have: C)
};

template <int NI>
__device__ __forceinline__ void load_score_ids(ScoreIds<NI> &si, const GraphDev &g, const unsigned short *plane, int C, int wave, int NW, int lane) {
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int it = wave + i * NW;
        const unsigned none = (unsigned)C;
        unsigned i0 = none, i1 = none, i2 = none, i3 = none;
        if (it < g.n_items) {
            const ItemMeta im = load_item(g.items, it);
            if (im.R <= 4) {
                const unsigned short *ip = plane + (size_t)im.slot_row * 64 + lane;
                i0 = ip[0];
                if (im.R > 1) i1 = ip[64];
                if (im.R > 2) i2 = ip[128];
                if (im.R > 3) i3 = ip[192];
            }
        }
        si.id[i][0] = i0 | (i1 << 16);
        si.id[i][1] = i2 | (i3 << 16);
    });
}

// lse_regs with the score of every arc's class
__device__ __forceinline__ float lse_regs_scored(float w0, float w1, float w2, float w3, unsigned c01, unsigned c23, unsigned i01, unsigned i23,
                                                 int R, int lg, const float *a, const float *ur) {
    float x0 = w0 + a[c01 & 0xffffu] + ur[i01 & 0xffffu];
    float x1 = w1 + a[c01 >> 16] + ur[i01 >> 16];
    float x2 = MM_NINF, x3 = MM_NINF;
    if (R > 2) {
        x2 = w2 + a[c23 & 0xffffu] + ur[i23 & 0xffffu];
        x3 = w3 + a[c23 >> 16] + ur[i23 >> 16];
    }
    float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
    m = grp_max_rt(m, lg);
    const float m0 = (m > MM_NINF) ? m : 0.f;
    float sum = fast_exp2(x0 - m0) + fast_exp2(x1 - m0);
    if (R > 2) sum += fast_exp2(x2 - m0) + fast_exp2(x3 - m0);
    sum = grp_sum_rt(sum, lg);
    return m0 + fast_log2(sum);
}

// lse_item with the plane beside the slots: rows of up to 4 arcs per lane in two passes, longer ones online in chunks of 4 (their R is a
// multiple of 4; a padding slot has the weight -inf and the id C)
__device__ __forceinline__ float lse_item_scored(const Slot *slots, const unsigned short *plane, const ItemMeta &im, int lane, const float *a,
                                                 const float *ur) {
    const Slot *sp = slots + (size_t)im.slot_row * 64 + lane;
    const unsigned short *ip = plane + (size_t)im.slot_row * 64 + lane;
    const int R = im.R, lg = im.log2g;
    if (R <= 4) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = MM_NINF;
            if (k < R) {
                const Slot s = load_slot(sp + k * 64);
                x[k] = s.w + a[s.col] + ur[ip[k * 64]];
            }
        }
        float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        m = grp_max_rt(m, lg);
        const float m0 = (m > MM_NINF) ? m : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) sum += fast_exp2(x[k] - m0);
        sum = grp_sum_rt(sum, lg);
        return m0 + fast_log2(sum);
    }
    float m = MM_NINF, sum = 0.f;
    for (int k0 = 0; k0 < R; k0 += 4) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Slot s = load_slot(sp + (k0 + k) * 64);
            x[k] = s.w + a[s.col] + ur[ip[(k0 + k) * 64]];
        }
        const float cm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        const float mn = fmaxf(m, cm);
        const float mn0 = (mn > MM_NINF) ? mn : 0.f;
        sum = sum * fast_exp2(m - mn0);
#pragma unroll
        for (int k = 0; k < 4; ++k) sum += fast_exp2(x[k] - mn0);
        m = mn;
    }
    const float M = grp_max_rt(m, lg);
    const float M0 = (M > MM_NINF) ? M : 0.f;
    sum = grp_sum_rt(sum * fast_exp2(m - M0), lg);
    return M0 + fast_log2(sum);
}

// for_items with the scored gather: epi(value, row, pdf, emn[pdf]) on the leader lane of each row group
template <int NI, class Epi>
__device__ __forceinline__ void for_items_scored(const ItemRegs<NI> &rg, const ScoreIds<NI> &si, const GraphDev &g, const unsigned short *plane,
                                                 int wave, int NW, int lane, const float *a, const float *emn, const float *ur, Epi &&epi) {
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int meta = rg.meta[i];
        if (meta != 0) {
            int R = meta & 0xff, lg = meta >> 8;
            asm volatile("" : "+s"(R), "+s"(lg));  // (opaque per frame, as in for_items)
            const unsigned row = rg.ri[i] & 0xffffu;
            const float e = emn[row != 0xffffu ? (rg.ri[i] >> 16) : 0u];
            const float v = lse_regs_scored(rg.w[i][0], rg.w[i][1], rg.w[i][2], rg.w[i][3], rg.c[i][0], rg.c[i][1], si.id[i][0], si.id[i][1], R, lg, a, ur);
            if (row != 0xffffu && (lane & ((1 << lg) - 1)) == 0) epi(v, (int)row, (int)(rg.ri[i] >> 16), e);
        }
    });
    const int resident = NI * NW < g.n_short ? NI * NW : g.n_short;
    for (int it = wave; it < g.n_items; it += NW) {
        if (it < resident) continue;
        const ItemMeta im = load_item(g.items, it);
        const RowInfo r = g.rowinfo[(size_t)it * 64 + lane];
        const float e = emn[r.row >= 0 ? r.pdf : 0];
        const float v = lse_item_scored(g.slots, plane, im, lane, a, ur);
        if (r.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) epi(v, r.row, r.pdf, e);
    }
}

// The score row of transition t one step ahead: EVERY thread loads a raw value from a clamped, always valid address (row
// 0 <= t <= tmax = len - 1: no row of a frame t >= len is ever read); stage_score_ahead stores it scaled a phase later.  The classes
// beyond the block's threads are staged from memory.  (factor: log2 e here; 1 for the tropical mm_classpath_fwd_kernel)
__device__ __forceinline__ float score_load_raw(const float *Ub, long long usn, long long usc, int t, int tmax, int C, int q) {
    const int tt = t < 0 ? 0 : (t > tmax ? tmax : t), cc = q < C ? q : C - 1;
    return Ub[(long long)tt * usn + (long long)cc * usc];
}
__device__ __forceinline__ void stage_score(float *dst, const float *Ub, long long usn, long long usc, int t, int C, int from, int NT,
                                            float factor = MM_LOG2E) {
    for (int q = from; q < C; q += NT) dst[q] = Ub[(long long)t * usn + (long long)q * usc] * factor;
}
__device__ __forceinline__ void stage_score_ahead(float *dst, float raw, const float *Ub, long long usn, long long usc, int t, int C, int tid, int NT,
                                                  float factor = MM_LOG2E) {
    if (tid < C) dst[tid] = raw * factor;
    if (C > NT) stage_score(dst, Ub, usn, usc, t, C, tid + NT, NT, factor);
}

// where both kernels keep the two score rows: behind the arc kernel's plan and its waves' sums
__device__ __forceinline__ float *score_rows(float *lds, const LdsPlan &L) { return lds + L.total + 2 * MM_MAX_WAVES; }

// forward: the alpha~ rows of frames 1..len and C_n in the workspace, log2 Z in wsC[0].  grid = B workgroups (one utterance each),
// block = 64 * NW threads, NW <= 8.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_scored_fwd_kernel(RunParams p, ScoredParams sp) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *part = lds + L.part;
    float *ur = score_rows(lds, L);  // [2][UR]
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    const GraphDev gf = u.g[0];
    const unsigned short *plane = sp.sc[b].plane[0];
    const int NC = sp.C, UR = sp.urow;
    const float *Ub = sp.U ? sp.U + (long long)b * sp.usb : nullptr;

    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, MM_LOG2E);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    for (int q = tid; q < 2 * UR; q += NT) ur[q] = 0.f;
    vsync();
    {   // frame 1: alpha_hat (*) lhs[:,1]
        float wm = MM_NINF;
        float *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        for (int s = tid; s < S1; s += NT) {
            const float v = u.init[s] + e1[u.s2p[s]];
            a1[s] = v;
            wm = fmaxf(wm, v);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        if (NF >= 2) {
            stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, MM_LOG2E);
            if (Ub) stage_score(ur, Ub, sp.usn, sp.usc, 0, NC, tid, NT);  // transition 0 (step 2)
        }
        if (tid == 0) wsC[1] = 0.0;
    }
    vsync();
    ItemRegs<NI> rg;
    ScoreIds<NI> si;
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    load_score_ids<NI>(si, gf, plane, NC, wave, NW, lane);
    double Cc = 0.0;
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    float uvp = (Ub && len >= 1) ? score_load_raw(Ub, sp.usn, sp.usc, 1, len - 1, NC, tid) : 0.f;
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        const float *urn = ur + (n & 1) * UR;  // transition n - 2
        const float M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        Cc += (double)M;
        if (tid == 0) wsC[n] = Cc;
        if (n + 1 <= NF) {
            stage_em_ahead<em_value>(em + ((n + 1) & 1) * P1p, evp, Vb, p.vsn, n + 1, len, P, tid, NT, MM_LOG2E);
            if (Ub) stage_score_ahead(ur + ((n + 1) & 1) * UR, uvp, Ub, sp.usn, sp.usc, n - 1, NC, tid, NT);
        }
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        if (Ub) uvp = score_load_raw(Ub, sp.usn, sp.usc, n, len - 1, NC, tid);
        copy_row(wsA + (long long)(n - 1) * S1p, ap, S1p >> 2, tid, NT);  // frame n - 1 leaves the chip once, while frame n is computed
        float wm = MM_NINF;
        for_items_scored<NI>(rg, si, gf, plane, wave, NW, lane, ap, emn, urn, [&](float v, int row, int, float e) {
            v = v + e - M;
            an[row] = v;
            wm = max_nc(wm, v);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        vsync();
    }
    if (tid == 0) wsC[0] = (double)buf[(NF & 1) * S1p + fstate] + Cc;
}

// backward: gamma, xi and ttl, each where it is asked for.  Same grid and block as the forward kernel.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_scored_bwd_kernel(RunParams p, ScoredParams sp) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *bins = lds + L.bins, *part = lds + L.part;
    float *psum = lds + L.total;  // [2][MM_MAX_WAVES] the waves' sums of the state posteriors of a frame (as mm_arc_kernel)
    float *ur = score_rows(lds, L);  // [2][UR]
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    const GraphDev gb = u.g[1];
    const ClassDev cd = sp.cls[b];
    const ScoredDev sd = sp.sc[b];
    const unsigned short *plane = sd.plane[1];
    const int NC = sp.C, UR = sp.urow;
    const float *Ub = sp.U ? sp.U + (long long)b * sp.usb : nullptr;
    const bool want_x = sp.xi != nullptr, want_g = p.gamma != nullptr;  // (kernel arguments: wave-uniform)
    const bool tg = sp.terms_global != 0;
    float *terms = tg ? sp.terms + 2 * cd.term_off : ur + 2 * UR;  // [2][cd.M]
    float *xb = sp.xi + (long long)b * sp.xsb;
    float *gout = p.gamma + (long long)b * p.gsb;
    const double logZ2 = wsC[0];
    const bool ok = logZ2 > -1e300;
    if (sp.ttl && tid == 0) sp.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    // frames beyond the utterance: only the phony self-loop is alive (no accepting path: nothing is)
    const int zfrom = (ok && len >= 1) ? len : 0;
    if (want_x)
        for (long long q = tid; q < (long long)(p.N - (ok ? len : 0)) * cd.C; q += NT) {
            const int c = (int)(q % cd.C);
            xb[((ok ? len : 0) + q / cd.C) * sp.xsn + c * sp.xsc] = (ok && c == cd.cphony) ? 1.f : 0.f;
        }
    if (want_g) zero_gamma_from(gout, p.gsn, p.gsp, zfrom, p.N, P, tid, NT);
    if (!ok || len < 1) return;

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    for (int q = tid; q < 2 * UR; q += NT) ur[q] = 0.f;
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    copy_row(stage + (len & 1) * S1p, wsA + (long long)len * S1p, S1p >> 2, tid, NT);
    if (Ub) stage_score(ur + ((len - 1) & 1) * UR, Ub, sp.usn, sp.usc, len - 1, NC, tid, NT);  // transition len - 1 (step len)
    vsync();
    ItemRegs<NI> rg;
    ScoreIds<NI> si;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    load_score_ids<NI>(si, gb, plane, NC, wave, NW, lane);
    double D = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f, uvp = 0.f;
    double Cn = wsC[len], Cpre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions, C_f and the scores of the transition out of it, one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        Cpre = wsC[f];
        if (Ub) uvp = score_load_raw(Ub, sp.usn, sp.usc, f - 1, len - 1, NC, tid);
    };
    if (len >= 2) prefetch(len - 1);
    float corr = 0.f;  // log2 of the state posteriors' sum of frame n + 1 (1 in exact arithmetic)
    for (int n = len; n >= 1; --n) {
        const float *yp = buf + ((n + 1) & 1) * S1p;
        float *yn = buf + (n & 1) * S1p;
        const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
        const float *emn = em + (n & 1) * P1p;
        const float *urn = ur + ((n - 1) & 1) * UR;  // transition n - 1: frame n -> frame n + 1
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        if (n < len) {
            float s = 0.f;  // (the waves' sums one after the other, as mm_arc_kernel adds them)
            for (int w = 0; w < NW; ++w) s += psum[((n + 1) & 1) * MM_MAX_WAVES + w];
            if (s > 0.f) corr += fast_log2(s);
        }
        const float kappa = (float)(logZ2 - Cn - D + (double)corr);
        const float sh = -M - kappa;
        // gamma of frame n + 1 from its per-pdf sums (behind step n + 1's last barrier; one wave)
        if (want_g && n < len && wave == NW - 1) finalise_gamma(bins + ((n + 1) & 1) * P1p, P1, P, lane, gout + (long long)n * p.gsn, p.gsp);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            stage_row<BIGV>(stage + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            if (Ub) stage_score_ahead(ur + (n & 1) * UR, uvp, Ub, sp.usn, sp.usc, n - 2, NC, tid, NT);
            Cn = Cpre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        if (want_x) {
            // the classes of frame n + 1, from the half of the term row that frame's barriers closed
            if (n < len) class_pass(cd, terms + ((n + 1) & 1) * cd.M, xb + (long long)n * sp.xsn, sp.xsc, wave, NW, lane);
            // the terms of frame n: rank m by thread m mod NT (as mm_arcclass_kernel), the score of the rank's class added
            float *__restrict__ tn = terms + (n & 1) * cd.M;
            const ClassRec *__restrict__ recs = cd.recs;
            const unsigned short *__restrict__ rcls = sd.rcls;
            int m = tid;
            for (; m + (MM_CLASS_UNROLL - 1) * NT < cd.M; m += MM_CLASS_UNROLL * NT) {
                ClassRec r[MM_CLASS_UNROLL];
                unsigned short c[MM_CLASS_UNROLL];
#pragma unroll
                for (int q = 0; q < MM_CLASS_UNROLL; ++q) {
                    r[q] = recs[m + q * NT];
                    c[q] = rcls[m + q * NT];
                }
#pragma unroll
                for (int q = 0; q < MM_CLASS_UNROLL; ++q) tn[m + q * NT] = fast_exp2((r[q].w + yp[r[q].col] + urn[c[q]]) + (ast[r[q].row] + sh));
            }
            for (; m < cd.M; m += NT) {
                const ClassRec r = recs[m];
                tn[m] = fast_exp2((r.w + yp[r.col] + urn[rcls[m]]) + (ast[r.row] + sh));
            }
        }
        // z_n = T (b_{n+1} (*) lhs_{n+1}) with the scores of transition n - 1, into the vector
        for_items_scored<NI>(rg, si, gb, plane, wave, NW, lane, yp, emn, urn, [&](float v, int row, int, float) { yn[row] = v - M; });
        stage_row_wait<BIGV>();  // this wave's part of alpha~ of frame n - 1 is in LDS
        if constexpr (!BIGV) {  // (BIGV: vsync carries the fences)
            if (tg) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        vsync();
        if constexpr (!BIGV) {
            if (tg) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        // Per pdf, over the pdf's states (every state is in one list; the phony pdf's holds the final state): the posterior, y_n =
        // beta~_n + e_n, the frame's maximum; 8 lanes add a pdf's posteriors in a fixed order.  The second barrier publishes the sums
        // and guards the staging buffers.
        float wm = MM_NINF, qs = 0.f;
        float *const bn[1] = {bins + (n & 1) * P1p};
        for_pdf_rows<1>(
            u, P1, wave, NW, lane, bn, [&](int pdf) { return emn[pdf]; },
            [&](int row, float e, float(&acc)[1]) {
                const float beta = yn[row];
                const float q = fast_exp2(ast[row] + beta - kappa);
                acc[0] += q;
                qs += q;
                const float y = beta + e;
                yn[row] = y;
                wm = fmaxf(wm, y);
            });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        qs = wave_sum(qs);
        if (lane == 0) psum[(n & 1) * MM_MAX_WAVES + wave] = qs;
        vsync();
    }
    if (want_x) class_pass(cd, terms + cd.M, xb, sp.xsc, wave, NW, lane);  // frame 1
    if (want_g && wave == 0) finalise_gamma(bins + 1 * P1p, P1, P, lane, gout, p.gsp);
}

}  // namespace mm
