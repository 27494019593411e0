// mm_kernel_filter.hip -- forward filtering posteriors with a carried state (mm_filterposteriors_f32: the causal quantities of a log
// batch -- the filtering posterior P(pdf_n = p | V_1..n), the per-frame increments of the prefix log-likelihood and the one-step
// prediction a later call continues from) on the item form.  Included by mm_filter_tu.hip only.
//
// mm_filter_kernel   mm_leaky_fwd_kernel's step without the leak term and without a store: the vector a~_n = log2 a_n - C_n is carried
//                    normalised by the maximum of the frame before (C_n in float64), no row of it leaves the chip.  The start vector
//                    is the FSM's own (u.init) or the caller's state_in.  What a frame gives -- filt(n, .) and incr(n) -- is made
//                    from the finished vector, one frame late and on no barrier of its own:
//                      step n + 1  (the vector of frame n is the step's SOURCE: every wave may read all of it) the pass over the
//                                  pdf -> states lists adds 2^(a~_n(j) - M) per pdf, M = the maximum of a~_n itself -- the same
//                                  number the step normalises by --, 8 lanes per pdf in a fixed order, a 3-step DPP reduction, no
//                                  atomics: bins[n & 1];
//                      step n + 2  one wave adds the per-pdf sums in a fixed order (tot_n), writes filt(n, p) = bin_p / tot_n and
//                                  incr(n) = ln 2 (M + log2 tot_n - log2 tot_{n-1}) + E_n: the difference of the float64 offsets C
//                                  (E_n: the frame's largest emission, taken out of the vector and kept in C).
//                    The last frame is finished behind the loop.  In the last step (n = len + 1: every real emission is
//                    -inf, the phony one 0) the row epilogue keeps the row's value BEFORE the emission, a~ = log2 (+)_i a_len(i)
//                    T_hat(i, j) - C_{len+1}; behind the loop state_out(j) = ln 2 (a~(j) - log2 tot_len) leaves in one coalesced
//                    pass and the final state's row gives ttl = ln 2 (C_{len+1} + a~(final)).
//
// Range.  The per-pdf sums are float32 sums of 2^x with x = a~_n(j) - max_j a~_n(j) <= 0: the largest term is 1, the sum is within
// [1, S], a term below 2^-126 of the largest is dropped (its posterior is below 1e-37).  The frame's largest emission E_n never
// enters the vector (the rows add e - E_n, E_n goes to the float64 offset), so a constant added to a frame's emissions changes
// no bit of a~_n, hence none of filt, and moves incr(n) by itself.  (Relative to the LAGGED maximum x would carry the frame's own emission
// level: +100 nats overflow the sum, -150 nats flush it to zero.)  A frame without a live state has tot = 0: filt = 0, incr = -inf
// from there on, state_out = -inf, ttl = -inf; nothing is divided by it.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

// LDS carve, in floats: the item kernel's export plan (no stage rows) and two scalars the finishing wave hands to the others
struct FilterLds {
    int buf, em, bins, part, fin, total;
};
__host__ __device__ inline FilterLds filter_lds_plan(int S1p, int P1p) {
    FilterLds l;
    l.buf = 0;                    // [2][S1p] the state vectors
    l.em = l.buf + 2 * S1p;       // [2][P1p] emissions
    l.bins = l.em + 2 * P1p;      // [2][P1p] per-pdf sums of 2^(a~ - M)
    l.part = l.bins + 2 * P1p;    // [2][MM_MAX_WAVES] the waves' maxima
    l.fin = l.part + 2 * MM_MAX_WAVES;  // [4] log2 tot_len, alive (behind the loop)
    l.total = l.fin + 4;
    return l;
}

// grid = B workgroups (one utterance each), block = 64 * NW threads, NW <= 8.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_filter_kernel(RunParams p, FilterParams fp) {
    extern __shared__ float4 filter_lds4[];
    float *lds = reinterpret_cast<float *>(filter_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const FilterLds L = filter_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *bins = lds + L.bins, *fin = lds + L.fin;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    const float *sin = fp.state_in ? fp.state_in + u.state_off : nullptr;
    float *sout = fp.state_out ? fp.state_out + u.state_off : nullptr;
    float *fb = fp.filt ? fp.filt + (long long)b * fp.fsb : nullptr;
    float *ib = fp.incr ? fp.incr + (long long)b * fp.isb : nullptr;
    // the frames beyond len: exact zeros
    if (fb) zero_gamma_from(fb, fp.fsn, fp.fsp, len, p.N, P, tid, NT);
    if (ib)
        for (int q = len + tid; q < p.N; q += NT) ib[q] = 0.f;
    if (len == 0) {  // nothing to filter: the state passes through (NULL in: ln alpha_hat, the vector NULL stands for)
        if (sout)
            for (int s = tid; s < S1; s += NT) sout[s] = sin ? sin[s] : u.init[s] * MM_LN2;
        if (fp.ttl && tid == 0) fp.ttl[b] = MM_NINF;
        return;
    }
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, 1.f);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    vsync();
    // E_n, the largest real emission of frame n (natural log), is taken out of the frame's emissions and kept in the offset: the
    // vector stays near 0 whatever the level of V, and e - E_n is exact where the rounding of e * log2(e) at that level is not
    float Ec = 0.f, E1 = 0.f, E2 = 0.f;  // of the step's frame n, of frames n - 1 and n - 2
    {   // frame 1: start (*) lhs[:,1]; the phony final state starts empty.  (state_in is read here alone and state_out written
        // behind the loop: they may be one buffer)
        float wm = MM_NINF;
        float *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        Ec = frame_emax(e1, P, lane);
        for (int s = tid; s < S1; s += NT) {
            const float st = sin ? (s < fstate ? sin[s] * MM_LOG2E : MM_NINF) : u.init[s];
            const float v = st + (e1[u.s2p[s]] - Ec) * MM_LOG2E;
            a1[s] = v;
            wm = fmaxf(wm, v);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        if (NF >= 2) stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, 1.f);
    }
    vsync();
    ItemRegs<NI> rg;
    const GraphDev gf = u.g[0];
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    double C = (double)Ec * 1.4426950408889634;
    float M = 0.f, Mp = 0.f;     // the maxima of the step and of the step before: frame n - 1's and frame n - 2's own
    float ltp = 0.f;             // (finishing wave) log2 tot of the frame finished last; l_0 = 0
    bool alive = true;           // (finishing wave) no frame so far without a live state
    // (not finalise_gamma: a frame without mass ends every frame behind it, and the sum also gives incr)
    // frame f from its per-pdf sums (one wave): Mf = the maximum of a~_f, what the sums were taken relative to
    auto finalise = [&](int f, float Mf, float Ef) {
        const float *bf = bins + (f & 1) * P1p;
        float s = 0.f;
        for (int q = lane; q < P; q += 64) s += bf[q];
        s = wave_sum(s);
        alive = alive && s > 0.f;
        const float inv = alive ? 1.f / s : 0.f;
        if (fb) {
            float *gp = fb + (long long)(f - 1) * fp.fsn;
            for (int q = lane; q < P; q += 64) gp[q * fp.fsp] = bf[q] * inv;
        }
        const float lt = fast_log2(s);
        if (ib && lane == 0) ib[f - 1] = alive ? (Mf + (lt - ltp)) * MM_LN2 + Ef : MM_NINF;
        ltp = lt;
    };
    // the emissions travel one frame ahead in a register (as in mm_log_kernel)
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        Mp = M;
        M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        E2 = E1;
        E1 = Ec;
        Ec = frame_emax(emn, P, lane);  // (the last step: no real emission, 0)
        C += (double)M + (double)Ec * 1.4426950408889634;
        if (n >= 3 && wave == NW - 1) finalise(n - 2, Mp, E2);
        if (n + 1 <= NF) stage_em_ahead<em_value_nat>(em + ((n + 1) & 1) * P1p, evp, Vb, p.vsn, n + 1, len, P, tid, NT, 1.f);
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        // frame n - 1 per pdf, over the pdf's states (the phony pdf's list holds the final state alone: -inf up to frame len, left out)
        for_pdf_rows<1>(u, P, wave, NW, lane, {bins + ((n - 1) & 1) * P1p}, [](int) { return 0; },
                        [&](int row, int, float(&acc)[1]) { acc[0] += fast_exp2(ap[row] - M); });
        float wm = MM_NINF;
        const bool last = n == NF;
        for_items<NI>(rg, gf, wave, NW, lane, ap, emn, [&](float v, int row, int, float e) {
            v -= M;
            if (!last) v += (e - Ec) * MM_LOG2E;  // (last step: e is -inf for the real rows, 0 for the final state's)
            an[row] = v;
            wm = max_nc(wm, v);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        vsync();
    }
    // frame len (the last step finished frame len - 1); what the other waves need of it
    if (wave == NW - 1) {
        finalise(len, M, E1);
        if (lane == 0) {
            fin[0] = ltp;
            fin[1] = alive ? 1.f : 0.f;
        }
    }
    vsync();
    const float *av = buf + (NF & 1) * S1p;
    const float lt = fin[0];
    const bool ok = fin[1] != 0.f;
    if (sout)
        for (int s = tid; s < S1; s += NT) sout[s] = ok ? (av[s] - lt) * MM_LN2 : MM_NINF;
    if (fp.ttl && tid == 0) fp.ttl[b] = ok ? (float)((C + (double)av[fstate]) * (double)MM_LN2) : MM_NINF;
}

}  // namespace mm
