// mm_kernel_leaky.hip -- pdf posteriors of the leaky HMM (mm_leakyposteriors_f32: the denominator forward-backward of LF-MMI
// training as the chain-model trainers run it) on the item form.  Included by mm_leaky_tu.hip only.
//
// The FSM's T_hat is replaced by T_eps = (I + eps u pi') T_hat: after any frame, from any real state, a path may jump with weight
// eps pi(k) to initial state k and then takes an ordinary arc of k.  The rank-one term is never written out.  With
// rho(j) = (+)_k pi(k) T_hat(k, j) -- one constant per row, the "leak rows", made on the host -- and tot_n = (+)_{i real} alpha_n(i):
//     alpha_n(j) = lhs_n(j) [ (+)_i alpha_{n-1}(i) T_hat(i, j)  (+)  eps tot_{n-1} rho(j) ]
//     z_n(i)     = (+)_j T_hat(i, j) lhs_{n+1}(j) beta_{n+1}(j)          c_n = (+)_k pi(k) z_n(k)
//     beta_n(i)  = z_n(i) (+) eps c_n  for real i,   beta_n(final) = z_n(final)
//
// mm_leaky_fwd_kernel   mm_log_kernel<MODE_FB, NI, 1>'s step; the leak term joins a row's log-sum-exp as one more term (one
//                       maximum, one exponential and one add per ITEM, none per arc).  tot is one frame late, like the lagged
//                       maximum: every wave adds up 2^v of the rows it finishes, the partial sums sit beside the waves' maxima
//                       and are combined at the top of the next step -- no barrier more than the item kernel's one.
// mm_leaky_bwd_kernel   the fix-up form, on the two barriers of the item kernel's deterministic mode: the items leave z_n in the
//                       vector and each wave its part of c_n; behind the first barrier the pass over the pdf -> states lists,
//                       which the deterministic mode makes anyway, forms beta_n = z_n (+) eps c_n, the state posterior,
//                       y_n = beta_n + e and the frame's maximum while it adds the posteriors up per pdf (8 lanes per pdf, fixed
//                       order, no atomics: the same bits on every run).  rho (forward) and pi (backward) are read from a copy in LDS.
//
// Range.  The waves' sums behind tot and c are float32 sums of 2^(x + MM_LEAK_BIAS).  Forward, x = v - E_n: v is normalised by the
// maximum of the frame before and still carries its own frame's emission, so the largest real emission E_n of the frame (every wave
// takes it from the staged emissions) is taken out and put back when the sum is used -- a constant added to V changes no bit of the
// sum.  Backward, x = pi + z, z normalised by the maximum of y_{n+1}, which holds the emission already.  Both x are <= the largest
// arc / initial weight (0 for probabilities); a term more than 2^-158 below that bound is dropped, and a frame ALL of whose terms are
// (every live state's own emission 110 nats below the frame's largest, or every initial state's z that far below the largest z)
// loses its leak: the result there is the unleaked one, never a NaN.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

#define MM_LEAK_BIAS 32.f

// LDS carve of both kernels, in floats: the item kernel's plan with the stage rows, the row constants and the waves' sums
struct LeakLds {
    int buf, stage, rowc, em, bins, part, psum, total;
};
__host__ __device__ inline LeakLds leaky_lds_plan(int S1p, int P1p) {
    LeakLds l;
    l.buf = 0;                     // [2][S1p] the state vectors
    l.stage = l.buf + 2 * S1p;     // [2][S1p] alpha~ of a frame (backward)
    l.rowc = l.stage + 2 * S1p;    // [S1p] the row constants: rho (forward), pi (backward)
    l.em = l.rowc + S1p;           // [2][P1p] emissions
    l.bins = l.em + 2 * P1p;       // [2][P1p] per-pdf sums of the posteriors
    l.part = l.bins + 2 * P1p;     // [2][MM_MAX_WAVES] the waves' maxima
    l.psum = l.part + 2 * MM_MAX_WAVES;  // [2][MM_MAX_WAVES] the waves' sums behind tot / c
    l.total = l.psum + 2 * MM_MAX_WAVES;
    return l;
}

// a wave's partial sum where part_sum reads it
__device__ __forceinline__ void leak_part_put(float *ps, int wave, int lane, float s) {
    s = wave_sum(s);
    if (lane == 0) ps[wave] = s;
}
__device__ __forceinline__ float logaddexp2(float a, float b) {
    const float m = fmaxf(a, b);
    const float m0 = (m > MM_NINF) ? m : 0.f;
    return m0 + fast_log2(fast_exp2(a - m0) + fast_exp2(b - m0));
}

// the row constants of a kernel where its items read them: a copy in LDS (visible behind the next barrier), or BIGV: where they are
template <bool BIGV>
__device__ __forceinline__ const float *stage_rowc(float *dst, const float *src, int S1, int tid, int NT) {
    if constexpr (BIGV) return src;
    for (int s = tid; s < S1; s += NT) dst[s] = src[s];
    return dst;
}

// for_items with the row constant: FOLD -- the row's value is (+)_k w_k a[col_k] (+) (rowc[row] + add), the term joined to the
// log-sum-exp; else the value is the plain log-sum-exp.  epi(value, rowc[row], row, pdf, e) on the leader lane of each row group.
template <int NI, bool FOLD, class Epi>
__device__ __forceinline__ void for_items_leak(const ItemRegs<NI> &rg, const GraphDev &g, const float *rowc, float add, int wave, int NW,
                                               int lane, const float *a, const float *emn, Epi &&epi) {
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int meta = rg.meta[i];
        if (meta != 0) {
            int R = meta & 0xff, lg = meta >> 8;
            asm volatile("" : "+s"(R), "+s"(lg));  // (opaque per frame: see for_items)
            const unsigned row = rg.ri[i] & 0xffffu;
            const float e = emn[row != 0xffffu ? (rg.ri[i] >> 16) : 0u];
            const unsigned c01 = rg.c[i][0], c23 = rg.c[i][1];
            const float x0 = rg.w[i][0] + a[c01 & 0xffffu], x1 = rg.w[i][1] + a[c01 >> 16];
            float x2 = MM_NINF, x3 = MM_NINF;
            if (R > 2) {
                x2 = rg.w[i][2] + a[c23 & 0xffffu];
                x3 = rg.w[i][3] + a[c23 >> 16];
            }
            float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
            m = grp_max_rt(m, lg);
            // (read here, not beside e: one live register less over the gathers.  A padding lane's value is never used.)
            const float k = rowc[row != 0xffffu ? row : 0u];
            const float t = k + add;
            if (FOLD) m = fmaxf(m, t);
            const float m0 = (m > MM_NINF) ? m : 0.f;
            float sum = fast_exp2(x0 - m0) + fast_exp2(x1 - m0);
            if (R > 2) sum += fast_exp2(x2 - m0) + fast_exp2(x3 - m0);
            sum = grp_sum_rt(sum, lg);
            if (FOLD) sum += fast_exp2(t - m0);
            if (row != 0xffffu && (lane & ((1 << lg) - 1)) == 0) epi(m0 + fast_log2(sum), k, (int)row, (int)(rg.ri[i] >> 16), e);
        }
    });
    // items beyond the register window, and long rows: streamed from L2
    const int resident = NI * NW < g.n_short ? NI * NW : g.n_short;
    for (int it = wave; it < g.n_items; it += NW) {
        if (it < resident) continue;
        const ItemMeta im = load_item(g.items, it);
        const RowInfo r = g.rowinfo[(size_t)it * 64 + lane];
        const float e = emn[r.row >= 0 ? r.pdf : 0];
        const float k = rowc[r.row >= 0 ? r.row : 0];
        float v = lse_item(g.slots, im, lane, a);
        if (FOLD) v = logaddexp2(v, k + add);
        if (r.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) epi(v, k, r.row, r.pdf, e);
    }
}

// forward: alpha~ rows, C_n and log2 Z (wsC[0]) in the workspace, laid out as the item kernel's forward half leaves them.
// grid = B workgroups (one utterance each), block = 64 * NW threads, NW <= 8.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_leaky_fwd_kernel(RunParams p, LeakParams lp) {
    extern __shared__ float4 leaky_lds4[];
    float *lds = reinterpret_cast<float *>(leaky_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const LeakLds L = leaky_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    const float *rho = stage_rowc<BIGV>(lds + L.rowc, lp.rows[b].rho, S1, tid, NT);
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, MM_LOG2E);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    vsync();
    float eprev;  // E_{n-1}: what the sums behind tot_{n-1} were taken relative to
    {   // frame 1: alpha_hat (*) lhs[:,1]
        float wm = MM_NINF, sw = 0.f;
        float *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        eprev = frame_emax(e1, P, lane);
        const float sb = MM_LEAK_BIAS - eprev;
        for (int s = tid; s < S1; s += NT) {
            const float v = u.init[s] + e1[u.s2p[s]];
            a1[s] = v;
            wm = fmaxf(wm, v);
            sw += fast_exp2(v + sb);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        leak_part_put(psum + 1 * MM_MAX_WAVES, wave, lane, sw);
        if (NF >= 2) stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, MM_LOG2E);
        if (tid == 0) wsC[1] = 0.0;
    }
    vsync();
    ItemRegs<NI> rg;
    const GraphDev gf = u.g[0];
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    double C = 0.0;
    // the emissions travel one frame ahead in a register (as in mm_log_kernel)
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        const float M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        // log2 (eps tot_{n-1}) in the normalisation of alpha~_{n-1}.  (The final state is in the sum: it is -inf up to frame len.)
        const float add = lp.leps2 + fast_log2(part_sum(psum + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane)) - (MM_LEAK_BIAS - eprev);
        eprev = frame_emax(emn, P, lane);
        const float sb = MM_LEAK_BIAS - eprev;
        C += (double)M;
        if (tid == 0) wsC[n] = C;
        if (n + 1 <= NF) stage_em_ahead<em_value>(em + ((n + 1) & 1) * P1p, evp, Vb, p.vsn, n + 1, len, P, tid, NT, MM_LOG2E);
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        copy_row(wsA + (long long)(n - 1) * S1p, ap, S1p >> 2, tid, NT);  // frame n - 1 leaves the chip once, while frame n is computed
        float wm = MM_NINF, sw = 0.f;
        for_items_leak<NI, true>(rg, gf, rho, add, wave, NW, lane, ap, emn, [&](float v, float, int row, int, float e) {
            v = v + e - M;
            an[row] = v;
            wm = max_nc(wm, v);
            sw += fast_exp2(v + sb);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        leak_part_put(psum + (n & 1) * MM_MAX_WAVES, wave, lane, sw);
        vsync();
    }
    if (tid == 0) wsC[0] = (double)buf[(NF & 1) * S1p + fstate] + C;  // log2 Z
}

// backward: gamma and ttl.  Same grid and block as the forward kernel.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_leaky_bwd_kernel(RunParams p, LeakParams lp) {
    extern __shared__ float4 leaky_lds4[];
    float *lds = reinterpret_cast<float *>(leaky_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const LeakLds L = leaky_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *bins = lds + L.bins;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    const GraphDev gb = u.g[1];
    const double logZ2 = wsC[0];
    float *gam = p.gamma + (long long)b * p.gsb;
    if (!(logZ2 > -1e300)) {  // no path even with the leak: gamma = 0, ttl = -inf
        zero_gamma_from(gam, p.gsn, p.gsp, 0, p.N, P, tid, NT);
        if (tid == 0) p.ttl[b] = MM_NINF;
        return;
    }
    // (log2 Z is finite: len >= 1)
    const float *pi = stage_rowc<BIGV>(lds + L.rowc, u.init, S1, tid, NT);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;  // frame len + 1: the final state alone
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    copy_row(stage + (len & 1) * S1p, wsA + (long long)len * S1p, S1p >> 2, tid, NT);
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0;
    float tmin = (float)logZ2;
    const int n4 = S1p >> 2;
    float evp = 0.f;
    double Cn = wsC[len], Cpre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions and C_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        Cpre = wsC[f];
    };
    // gamma of frame f from its per-pdf sums (one wave).  Not finalise_gamma: the phony pdf's bin is in the sum, which the leak keeps
    // positive (no guard), and the sum also gives the frame's ttl
    auto finalise = [&](int f) {
        const float *bf = bins + (f & 1) * P1p;
        float s = 0.f;
        for (int q = lane; q < P1; q += 64) s += bf[q];
        s = wave_sum(s);
        const float inv = 1.f / s;
        float *gp = gam + (long long)(f - 1) * p.gsn;
        for (int q = lane; q < P; q += 64) gp[q * p.gsp] = bf[q] * inv;
        tmin = fminf(tmin, (float)(logZ2 + (double)fast_log2(s)));
    };
    if (len >= 2) prefetch(len - 1);
    for (int n = len; n >= 1; --n) {
        const float *yp = buf + ((n + 1) & 1) * S1p;
        float *yn = buf + (n & 1) * S1p;
        const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
        const float *emn = em + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        const float kappa = (float)(logZ2 - Cn - D);
        if (n < len && wave == NW - 1) finalise(n + 1);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            stage_row<BIGV>(stage + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        // z_n = T (beta_{n+1} (*) lhs_{n+1}) into the vector, this wave's part of c_n = pi . z_n
        float cw = 0.f;
        for_items_leak<NI, false>(rg, gb, pi, 0.f, wave, NW, lane, yp, emn, [&](float v, float pik, int row, int, float) {
            const float z = v - M;
            yn[row] = z;
            cw += fast_exp2(pik + z + MM_LEAK_BIAS);
        });
        leak_part_put(psum, wave, lane, cw);
        stage_row_wait<BIGV>();  // this wave's part of alpha~ of frame n - 1 is in LDS
        vsync();
        // Per pdf, over the pdf's states in pdf_rows (every state is in one list; the phony pdf's holds the final state, which does
        // not leak): beta_n = z_n (+) eps c_n, the posterior, y_n = beta_n + e over z_n, the frame's maximum; 8 lanes add a pdf's
        // posteriors in a fixed order, a 3-step DPP reduction ends it.  The second barrier also guards the staging buffers.
        const float lc = lp.leps2 + fast_log2(part_sum(psum, NW, lane)) - MM_LEAK_BIAS;
        float wm = MM_NINF;
        for_pdf_rows<1>(u, P1, wave, NW, lane, {bins + (n & 1) * P1p}, [&](int pdf) { return make_float2(emn[pdf], pdf < P ? lc : MM_NINF); },
                        [&](int row, float2 c, float(&acc)[1]) {
                            const float beta = logaddexp2(yn[row], c.y);
                            acc[0] += fast_exp2(ast[row] + beta - kappa);
                            const float y = beta + c.x;
                            yn[row] = y;
                            wm = fmaxf(wm, y);
                        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        vsync();
    }
    if (wave == 0) finalise(1);
    // zero the frames beyond len, reduce ttl
    zero_gamma_from(gam, p.gsn, p.gsp, len, p.N, P, tid, NT);
    vsync();  // part[] is free again
    if (lane == 0) part[wave] = tmin;
    vsync();
    if (tid == 0) {
        float t = part[0];
        for (int w = 1; w < NW; ++w) t = fminf(t, part[w]);
        p.ttl[b] = t * MM_LN2;
    }
}

}  // namespace mm
