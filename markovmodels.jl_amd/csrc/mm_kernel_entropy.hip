// mm_kernel_entropy.hip -- entropy of the posterior over complete paths and its gradient in the emissions
// (mm_pathentropy_f32: the objective of semi-supervised sequence training, an entropy regulariser, a confidence figure) on the
// item form.  Included by mm_entropy_tu.hip only.
//
// For utterance b, over the complete state sequences pi = s_1 .. s_{N+1} with P(pi) = w(pi) / Z:
//     H_b         = - sum_pi P(pi) ln P(pi)
//     grad_b(n,p) = d H_b / d V_b(n,p) = sum_{j : pdf(j) = p} q_n(j) (Hf_n(j) + Hb_n(j) - ln q_n(j) - H_b),   q_n: state posterior
// Hf_n(j), the entropy of the prefix s_1 .. s_{n-1} given s_n = j, and Hb_n(i), that of the suffix s_{n+1} .. s_{N+1} given
// s_n = i, ride on the alpha- and the beta-recursion (the entropy semiring: Hernando et al. 2005, Li & Eisner 2009):
//     Hf_1 = 0       Hf_n(j) = sum_i P(i | j) (Hf_{n-1}(i) - ln P(i | j)),   P(i | j) ~ alpha_{n-1}(i) T_ij
//     Hb_{N+1} = 0   Hb_n(i) = sum_j P(j | i) (Hb_{n+1}(j) - ln P(j | i)),   P(j | i) ~ T_ij lhs_{n+1}(j) beta_{n+1}(j)
//     H_b = Hf_{N+1}(final)
// Both directions are ONE row function.  With x_k the row's log2 terms, m their maximum, d_k = x_k - m, e_k = 2^d_k and
// den = sum e_k -- all formed for the row's log-sum-exp anyway --, P(k) = e_k / den and
//     row value = [sum_k e_k (H(k) - ln2 d_k)] / den + ln2 log2(den)
// so an arc costs one FMA and one multiply more than in mm_kernel_cost.hip, a row one reciprocal; log2(den) is the row's own.
// An arc from a dead state has d_k = -inf and e_k = 0: its term is SELECTED to 0, never multiplied (0 ln 0 := 0).  A row without
// weight, and a state no path reaches, carry 0.
//
// mm_entropy_fwd_kernel   alpha~, C_n and log2 Z exactly as mm_log_kernel<MODE_FB, NI, 1> leaves them, plus the Hf' store; writes
//                         entropy and ttl.  Without a store to fill (a value-only call) nothing but these two leaves the chip.
// mm_entropy_bwd_kernel   PASS 2's beta~ recursion carrying Hb'; per state q and q (Hf + Hb - ln q - H) written over the staged
//                         alpha~ / Hf' rows, per pdf their sums through the pdf_rows lists (8 lanes per pdf, fixed order, no
//                         atomics: the same bits on every run), then gamma and grad as mm_cost_bwd_kernel forms them, the
//                         frame's posterior mean of the bracket (zero by the chain rule of entropy) taken out.
//
// Numerics.  Hf grows about linearly with n, Hb with N - n, while the bracket of the gradient is a few nats.  Both are carried
// CENTRED like r' and t' of mm_kernel_cost.hip: Hf'_n = Hf_n - O_n, Hb'_n = Hb_n - Q_n with the float64 offsets O_n (filtering
// means of Hf' of the frames before n) and Q_n (posterior means of Hb' of the frames after n), applied one frame late.  They meet
// float32 only in H_b = Hf'_{len+1}(final) + O_{len+1} and in Hf' + Hb' - ln q + (O_n + Q_n - H_b).  ln q is ln2 times the
// exponent the row leader exponentiates for q anyway.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"
#include "mm_kernel_cost.hip"  // frame_mean, frame_mean_put: the frame means behind the offsets (no kernel of it is instantiated here)

namespace mm {

// LDS carve of both kernels, in floats (the pair vectors first: 8-byte aligned)
struct EntropyLds {
    int buf, sta, str, em, bins, gbins, part, psum, total;
};
__host__ __device__ inline EntropyLds entropy_lds_plan(int S1p, int P1p) {
    EntropyLds l;
    l.buf = 0;                  // [2][S1p] pairs
    l.sta = l.buf + 4 * S1p;    // [2][S1p] alpha~ of a frame, then its state posteriors (backward)
    l.str = l.sta + 2 * S1p;    // [2][S1p] Hf' of a frame, then q (Hf + Hb - ln q - H) (backward)
    l.em = l.str + 2 * S1p;     // [2][P1p] emissions
    l.bins = l.em + 2 * P1p;    // [2][P1p] per-pdf sums of q
    l.gbins = l.bins + 2 * P1p; // [2][P1p] per-pdf sums of q (Hf + Hb - ln q - H)
    l.part = l.gbins + 2 * P1p; // [2][MM_MAX_WAVES] the waves' maxima
    l.psum = l.part + 2 * MM_MAX_WAVES;  // [2][2][MM_MAX_WAVES] the waves' two sums behind a frame's mean
    l.total = l.psum + 4 * MM_MAX_WAVES;
    return l;
}

// one term of a row's numerator: e (h - ln2 d), 0 where the term has no weight (d = -inf there: select, do not multiply)
__device__ __forceinline__ float entropy_term(float e, float d, float h) { return e > 0.f ? e * fmaf(-MM_LN2, d, h) : 0.f; }
// the row value from its group sums
__device__ __forceinline__ float entropy_row(float num, float den, float log2den) {
    return den > 0.f ? fmaf(num, __builtin_amdgcn_rcpf(den), MM_LN2 * log2den) : 0.f;
}

// Every item of this wave over a vector of pairs `a` = {log2 weight, H'}: the log-sum-exp of w_k + a[col_k].x and the row value
// above over a[col_k].y.  epi(lse, value, row, pdf, e) runs on the leader lane of each row group; e: the row's emission, fetched
// before the arithmetic.
template <int NI, class Epi>
__device__ __forceinline__ void for_items_entropy(const ItemRegs<NI> &rg, const GraphDev &g, int wave, int NW, int lane, const float2 *a,
                                                  const float *emn, Epi &&epi) {
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int meta = rg.meta[i];
        if (meta != 0) {
            int R = meta & 0xff, lg = meta >> 8;
            asm volatile("" : "+s"(R), "+s"(lg));  // (opaque per frame: see for_items)
            const unsigned row = rg.ri[i] & 0xffffu;
            const bool real = row != 0xffffu;
            const unsigned pdf = real ? (rg.ri[i] >> 16) : 0u;
            const float e = emn[pdf];
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
            const float d0 = x0 - m0, d1 = x1 - m0;
            const float e0 = fast_exp2(d0), e1 = fast_exp2(d1);
            float sum = e0 + e1, num = entropy_term(e0, d0, v0.y) + entropy_term(e1, d1, v1.y);
            if (R > 2) {
                const float d2 = x2 - m0, d3 = x3 - m0;
                const float e2 = fast_exp2(d2), e3 = fast_exp2(d3);
                sum += e2 + e3;
                num += entropy_term(e2, d2, v2.y) + entropy_term(e3, d3, v3.y);
            }
            sum = grp_sum_rt(sum, lg);
            num = grp_sum_rt(num, lg);
            if (real && (lane & ((1 << lg) - 1)) == 0) {
                const float l2 = fast_log2(sum);
                epi(m0 + l2, entropy_row(num, sum, l2), (int)row, (int)pdf, e);
            }
        }
    });
    // items beyond the register window, and long rows: streamed from L2
    const int resident = NI * NW < g.n_short ? NI * NW : g.n_short;
    for (int it = wave; it < g.n_items; it += NW) {
        if (it < resident) continue;
        const ItemMeta im = load_item(g.items, it);
        const RowInfo r = g.rowinfo[(size_t)it * 64 + lane];
        const int pdf = r.row >= 0 ? r.pdf : 0;
        const float e = emn[pdf];
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
                const float dk = x[k] - m0, ek = fast_exp2(dk);
                sum += ek;
                num += entropy_term(ek, dk, vy[k]);
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
                const float dk = s.w + v.x - m0, ek = fast_exp2(dk);
                sum += ek;
                num += entropy_term(ek, dk, v.y);
            }
        }
        sum = grp_sum_rt(sum, lg);
        num = grp_sum_rt(num, lg);
        if (r.row >= 0 && (lane & ((1 << lg) - 1)) == 0) {
            const float l2 = fast_log2(sum);
            epi(m0 + l2, entropy_row(num, sum, l2), r.row, pdf, e);
        }
    }
}

// forward: log2 Z (wsC[0]) and H (wsO[0]), entropy and ttl; with a store to fill (ep.ws_h) also the alpha~ rows and C_n as the
// item kernel's forward half leaves them, the Hf' rows and O_n.
// grid = B workgroups (one utterance each), block = 64 * NW threads, NW <= 8.
// (Written out, prologue included, none of the parts of mm_item_parts.hip: the value-only call is this kernel alone, and moved onto the
// parts it measured 0.5 - 1.3 % slower.)
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_entropy_fwd_kernel(RunParams p, EntropyParams ep) {
    extern __shared__ float4 entropy_lds4[];
    float *lds = reinterpret_cast<float *>(entropy_lds4);
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;
    const int S1 = u.S1, S1p = u.S1p, P1 = u.P1, P = P1 - 1, P1p = (P1 + 3) & ~3;
    const int fstate = S1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int NF = len + 1;
    const EntropyLds L = entropy_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum;
    float *big = BIGV ? ep.ws_big + (long long)b * ep.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    auto vsync = [&]() {
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    };
    const float *Vb = p.V + (long long)b * p.vsb;
    float *wsA = p.ws_alpha + u.s1p_prefix * (long long)(p.N + 1);
    float *wsH = ep.ws_h ? ep.ws_h + u.s1p_prefix * (long long)(p.N + 1) : nullptr;
    double *wsC = p.ws_c + (long long)b * (p.N + 2);
    double *wsO = ep.ws_o + (long long)b * (p.N + 2);
    const bool store = wsH != nullptr;  // (uniform: a value-only call keeps no frame)
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, MM_LOG2E);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    vsync();
    {   // frame 1: alpha_hat (*) lhs[:,1], Hf_1 = 0: no prefix
        float wm = MM_NINF;
        float2 *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        for (int s = tid; s < S1; s += NT) {
            const float v = u.init[s] + e1[u.s2p[s]];
            a1[s] = make_float2(v, 0.f);
            wm = fmaxf(wm, v);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        frame_mean_put(psum + 1 * 2 * MM_MAX_WAVES, wave, lane, 0.f, 0.f);
        if (NF >= 2) stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, MM_LOG2E);
        if (tid == 0 && store) {
            wsC[1] = 0.0;
            wsO[1] = 0.0;
        }
    }
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, u.g[0], wave, NW, lane);
    const GraphDev gf = u.g[0];
    double C = 0.0, O = 0.0;
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);  // emissions travel one frame ahead in a register (as in mm_log_kernel)
    const int n4 = S1p >> 2;
    for (int n = 2; n <= NF; ++n) {
        const float2 *ap = buf + ((n - 1) & 1) * S1p;
        float2 *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        const float M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        const float mu = frame_mean(psum + ((n - 1) & 1) * 2 * MM_MAX_WAVES, NW, lane);  // filtering mean of Hf' of frame n - 1
        C += (double)M;
        O += (double)mu;
        if (tid == 0 && store) {
            wsC[n] = C;
            wsO[n] = O;
        }
        if (n + 1 <= NF) {
            if (tid <= P) em[((n + 1) & 1) * P1p + tid] = em_value(evp, n + 1, len, P, tid);
            if (P >= NT) stage_em(em + ((n + 1) & 1) * P1p + NT, Vb + NT, p.vsn, n + 1, len, P - NT, tid, NT, MM_LOG2E);
        }
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        if (store) {  // frame n - 1 leaves the chip once, the pairs taken apart: alpha~ rows as the item kernel stores them, Hf' rows beside
            const float4 *src = reinterpret_cast<const float4 *>(ap);
            float4 *da = reinterpret_cast<float4 *>(wsA + (long long)(n - 1) * S1p);
            float4 *dh = reinterpret_cast<float4 *>(wsH + (long long)(n - 1) * S1p);
            for (int q = tid; q < n4; q += NT) {
                const float4 lo = src[2 * q], hi = src[2 * q + 1];
                da[q] = make_float4(lo.x, lo.z, hi.x, hi.z);
                dh[q] = make_float4(lo.y, lo.w, hi.y, hi.w);
            }
        }
        float wm = MM_NINF, sw = 0.f, swv = 0.f;
        for_items_entropy<NI>(rg, gf, wave, NW, lane, ap, emn, [&](float v, float hbar, int row, int pdf, float e) {
            v = v + e - M;
            const float h = v > MM_NINF ? hbar - mu : 0.f;
            an[row] = make_float2(v, h);
            wm = max_nc(wm, v);
            const float wgt = fast_exp2(v);
            sw += wgt;
            swv = fmaf(wgt, h, swv);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        frame_mean_put(psum + (n & 1) * 2 * MM_MAX_WAVES, wave, lane, sw, swv);
        vsync();
    }
    if (tid == 0) {
        const float2 last = buf[(NF & 1) * S1p + fstate];
        const double logZ2 = (double)last.x + C, H = (double)last.y + O;  // H = Hf_{len+1}(final)
        wsC[0] = logZ2;
        wsO[0] = H;
        const bool ok = logZ2 > -1e300;
        ep.entropy[b] = ok ? (float)H : 0.f;
        if (ep.ttl) ep.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    }
}

// backward: gamma and grad (either may be NULL).  Same grid and block as the forward kernel.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_entropy_bwd_kernel(RunParams p, EntropyParams ep) {
    extern __shared__ float4 entropy_lds4[];
    float *lds = reinterpret_cast<float *>(entropy_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const EntropyLds L = entropy_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum;
    float *big = BIGV ? ep.ws_big + (long long)b * ep.big_stride : nullptr;
    float2 *buf = reinterpret_cast<float2 *>(BIGV ? big : lds + L.buf);
    float *wsH = ep.ws_h ? ep.ws_h + u.s1p_prefix * (long long)(p.N + 1) : nullptr;
    double *wsO = ep.ws_o + (long long)b * (p.N + 2);
    float *bins = lds + L.bins, *gbins = lds + L.gbins;
    float *sta = BIGV ? big + 4 * S1p : lds + L.sta;
    float *str = BIGV ? big + 6 * S1p : lds + L.str;
    const GraphDev gb = u.g[1];
    const double logZ2 = wsC[0], H = wsO[0];
    const long long gbase = (long long)b * ep.gsb;
    const bool ok = logZ2 > -1e300;
    // frames without a result: all of them without an accepting path, else those beyond the length
    const int z0 = ok ? len : 0;
    // (not zero_gamma_from: two outputs on one walk, its 64-bit index arithmetic once)
    for (long long q = tid; q < (long long)(p.N - z0) * P; q += NT) {
        const long long o = gbase + (z0 + q / P) * ep.gsn + (q % P) * ep.gsp;
        if (ep.grad) ep.grad[o] = 0.f;
        if (ep.gamma) ep.gamma[o] = 0.f;
    }
    if (!ok || len < 1) return;

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = make_float2(MM_NINF, 0.f);
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = make_float2(0.f, 0.f);  // frame len + 1: the final state alone, no suffix
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    copy_row_pair(sta + (len & 1) * S1p, wsA + (long long)len * S1p, str + (len & 1) * S1p, wsH + (long long)len * S1p, S1p >> 2, tid, NT);
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0, Q = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f;
    double Cn = wsC[len], On = wsO[len], Cpre = 0.0, Opre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions, C_f and O_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
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
        // H(prefix | s_n) + H(suffix | s_n) - ln q(s_n) has posterior mean H (chain rule, Markov property): what the frame's sum of
        // the bracket is left with is the rounding all states of the frame share -- of H, and of Hf' and Hb' along their common
        // history -- and is taken out, so sum_p grad(n, p) = 0 holds to the rounding of this line
        const float mean = gs * inv;
        const long long o = gbase + (long long)(f - 1) * ep.gsn;
        for (int q = lane; q < P; q += 64) {
            if (ep.grad) ep.grad[o + q * ep.gsp] = (gf[q] - bf[q] * mean) * inv;
            if (ep.gamma) ep.gamma[o + q * ep.gsp] = bf[q] * inv;
        }
    };
    if (len >= 2) prefetch(len - 1);
    for (int n = len; n >= 1; --n) {
        const float2 *yp = buf + ((n + 1) & 1) * S1p;
        float2 *yn = buf + (n & 1) * S1p;
        float *ast = sta + (n & 1) * S1p;  // alpha~ of frame n, replaced by the state posteriors as they are made
        float *hst = str + (n & 1) * S1p;  // Hf' of frame n, replaced by q (Hf + Hb - ln q - H)
        const float *emn = em + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        // posterior mean of Hb' of frame n + 1
        const float mu = (n == len) ? 0.f : frame_mean(psum + ((n + 1) & 1) * 2 * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        Q += (double)mu;  // = Q_n: Hb_n = Hb'_n + Q_n
        const float kappa = (float)(logZ2 - Cn - D);
        const float off = (float)(On + Q - H);  // Hf_n(j) + Hb_n(j) - H = Hf'_n(j) + Hb'_n(j) + off
        if (n < len && wave == NW - 1) finalise(n + 1);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            stage_row_pair<BIGV>(sta + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, str + ((n - 1) & 1) * S1p,
                                 wsH + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            On = Opre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        float wm = MM_NINF, sq = 0.f, sqh = 0.f;
        for_items_entropy<NI>(rg, gb, wave, NW, lane, yp, emn, [&](float v, float hbar, int row, int pdf, float e) {
            const float beta = v - M;  // T (B[:,n+1] (*) lhs[:,n+1])
            const float lq = ast[row] + beta - kappa;         // log2 of the state posterior
            const float q = fast_exp2(lq);
            const float hb = beta > MM_NINF ? hbar - mu : 0.f;  // Hb'_n
            const float d = fmaf(-MM_LN2, lq, hst[row] + hb + off);
            ast[row] = q;
            hst[row] = q > 0.f ? q * d : 0.f;  // (q = 0: lq may be -inf)
            yn[row] = make_float2(beta + e, hb);
            wm = max_nc(wm, beta + e);
            sq += q;
            sqh = fmaf(q, hb, sqh);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        frame_mean_put(psum + (n & 1) * 2 * MM_MAX_WAVES, wave, lane, sq, sqh);
        stage_row_wait<BIGV>();  // this wave's part of frame n - 1 is in LDS
        vsync();
        // per pdf, over the pdf's states in pdf_rows: 8 lanes add the two products in a fixed order, a 3-step DPP reduction ends
        // it (mm_log_kernel's deterministic mode).  The second barrier also guards the staging buffers.
        for_pdf_rows<2>(u, P1, wave, NW, lane, {bins + (n & 1) * P1p, gbins + (n & 1) * P1p}, [](int) { return 0; },
                        [&](int row, int, float(&acc)[2]) {
                            acc[0] += ast[row];
                            acc[1] += hst[row];
                        });
        vsync();
    }
    if (wave == 0) finalise(1);
}

}  // namespace mm
