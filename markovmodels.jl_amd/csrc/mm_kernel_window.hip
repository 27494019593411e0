// mm_kernel_window.hip -- fixed-lag smoothing posteriors (mm_windowposteriors_f32: the forward-backward of a log batch over a WINDOW of
// the audio -- it starts from a carried vector instead of the FSM's initial one and ends open, beta = 1 on every real state, or on
// the final weights) on the item form.  Included by mm_window_tu.hip only.
//
// mm_window_fwd_kernel   mm_filter_kernel's step with mm_leaky_fwd_kernel's store: the vector a~_n = log2 a_n - C_n is carried
//                        normalised by the maximum of the frame before, the frame's largest emission E_n is taken out of its
//                        emissions and kept in the float64 offset C_n (a constant added to a frame moves C and no bit of a~), and
//                        every a~_n and C_n leaves for the workspace.  No per-pdf sums: the totals of two frames alone are taken,
//                        tot_n = sum_j 2^(a~_n(j) - max a~_n) of frame c (the commit frame: l_c, what state_out is normalised by)
//                        and of frame len (the open window's total), at the step whose source the frame is.  Step c + 1 keeps
//                        its rows' values BEFORE the emission in a vector of their own: state_out, written behind the loop.
//                        Step len + 1 (no real emission) finishes the final state's row: the closed window's total.
// mm_window_bwd_kernel   mm_leaky_bwd_kernel without the leak: z_n = T (b_{n+1} (*) lhs_{n+1}) by the items, then the pass over
//                        the pdf -> states lists forms the state posteriors, y_n = b~_n + (e - E_n) and the frame's maximum while it
//                        adds the posteriors up per pdf (8 lanes per pdf, fixed order, no atomics: the same bits on every run).
//                        An open utterance starts from b~_len = 0 on the real states in the place of the item pass of frame len.
//                        E_n is kept out of y as it is kept out of a~: it goes to the float64 offset D.
//
// Range.  As the filter kernel's: the totals are float32 sums of 2^x, x <= 0 with a term 1 among them.  The posterior of state j
// at frame n is 2^(a~_n(j) + b~_n(j) - kappa_n), kappa_n = log2 total - C_n - D_n in float64: the frame's sum is 1 up to the
// rounding of the two recursions, and the frame is normalised by its own sum.  A window without mass (the total zero or not
// finite) never enters the backward loop: gamma = 0, ttl = -inf.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

// LDS carve of both kernels, in floats: the item kernel's plan with the stage rows (forward: the first stage row holds the rows of
// step c + 1 before the emission) and the waves' sums behind the two totals.  Its size is the arc kernel's (lds_plan with the
// stage rows + MM_ARC_LDS_EXTRA): a batch whose vectors are global for this entry has the global vectors mm_batch_create allocates.
struct WindowLds {
    int buf, stage, em, bins, part, psum, total;
};
__host__ __device__ inline WindowLds window_lds_plan(int S1p, int P1p) {
    WindowLds l;
    l.buf = 0;                     // [2][S1p] the state vectors
    l.stage = l.buf + 2 * S1p;     // [2][S1p] alpha~ of a frame (backward); [S1p] state_out before its normalisation (forward)
    l.em = l.stage + 2 * S1p;      // [2][P1p] emissions
    l.bins = l.em + 2 * P1p;       // [2][P1p] per-pdf sums of the posteriors (backward)
    l.part = l.bins + 2 * P1p;     // [2][MM_MAX_WAVES] the waves' maxima
    l.psum = l.part + 2 * MM_MAX_WAVES;  // [2][MM_MAX_WAVES] the waves' sums behind tot_c and tot_len (forward)
    l.total = l.psum + 2 * MM_MAX_WAVES;
    return l;
}

// forward: the a~ rows of frames 1..len and C_n in the workspace (laid out as the item kernel's forward half leaves them), log2 of
// the window's total in wsC[0]; state_out and lcommit.  grid = B workgroups (one utterance each), block = 64 * NW threads, NW <= 8.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_window_fwd_kernel(RunParams p, WindowParams wp) {
    extern __shared__ float4 window_lds4[];
    float *lds = reinterpret_cast<float *>(window_lds4);
    MM_ITEM_PROLOGUE(BIGV);
    const bool closed = wp.closed ? __builtin_amdgcn_readfirstlane(wp.closed[b]) != 0 : false;
    const WindowLds L = window_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    const float *sin = wp.state_in ? wp.state_in + u.state_off : nullptr;
    float *sout = wp.state_out ? wp.state_out + u.state_off : nullptr;
    int c = wp.commit ? __builtin_amdgcn_readfirstlane(wp.commit[b]) : len;
    c = c < 0 ? 0 : (c > len ? len : c);
    if (c == 0) {  // nothing is committed: the start vector passes through (NULL in: ln alpha_hat, the vector NULL stands for).
        // Every thread reads what it overwrites: state_in and state_out may be one buffer.
        if (sout)
            for (int s = tid; s < S1; s += NT) sout[s] = sin ? sin[s] : u.init[s] * MM_LN2;
        if (wp.lcommit && tid == 0) wp.lcommit[b] = 0.f;
    }
    if (len == 0) {
        if (tid == 0) wsC[0] = (double)MM_NINF;
        return;
    }
    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, 1.f);
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    float *sv = stage;  // the rows of step c + 1 before the emission
    for (int q = tid; q < S1p; q += NT) sv[q] = MM_NINF;
    vsync();
    float Ec = 0.f;  // E_n, the largest real emission of the step's frame (natural log): kept in the offset, not in the vector
    {   // frame 1: start (*) lhs[:,1]; the phony final state starts empty.  (state_in is read here alone, state_out of a commit
        // c >= 1 written behind the loop)
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
        stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, 1.f);
    }
    vsync();
    ItemRegs<NI> rg;
    const GraphDev gf = u.g[0];
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    double C = (double)Ec * 1.4426950408889634;
    double Cc = 0.0, Cl = 0.0;  // C_n + max a~_n of frames c and len: what their totals are relative to
    if (tid == 0) wsC[1] = C;
    // the emissions travel one frame ahead in a register (as in mm_log_kernel)
    float evp = em_load_raw(Vb, p.vsn, 3, p.N, P, tid);
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        const float M = part_max_dpp(part + ((n - 1) & 1) * MM_MAX_WAVES, NW, lane);
        const bool at_c = n - 1 == c, at_len = n == NF;
        if (at_c) Cc = C + (double)M;
        if (at_len) Cl = C + (double)M;
        Ec = frame_emax(emn, P, lane);  // (the last step: no real emission, 0)
        C += (double)M + (double)Ec * 1.4426950408889634;
        if (tid == 0) wsC[n] = C;
        if (n + 1 <= NF) stage_em_ahead<em_value_nat>(em + ((n + 1) & 1) * P1p, evp, Vb, p.vsn, n + 1, len, P, tid, NT, 1.f);
        evp = em_load_raw(Vb, p.vsn, n + 2, p.N, P, tid);
        copy_row(wsA + (long long)(n - 1) * S1p, ap, S1p >> 2, tid, NT);  // frame n - 1 leaves the chip once, while frame n is computed
        if (at_c || at_len) {  // the total of frame n - 1 over the real states, relative to the frame's own maximum
            float sw = 0.f;
            for (int s = tid; s < fstate; s += NT) sw += fast_exp2(ap[s] - M);
            sw = wave_sum(sw);
            if (lane == 0) {
                if (at_c) psum[0 * MM_MAX_WAVES + wave] = sw;
                if (at_len) psum[1 * MM_MAX_WAVES + wave] = sw;
            }
        }
        float wm = MM_NINF;
        for_items<NI>(rg, gf, wave, NW, lane, ap, emn, [&](float v, int row, int, float e) {
            v -= M;
            if (at_c) sv[row] = v;
            if (!at_len) v += (e - Ec) * MM_LOG2E;  // (last step: e is -inf for the real rows, 0 for the final state's)
            an[row] = v;
            wm = max_nc(wm, v);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        vsync();
    }
    // (the barrier of the last step: the waves' sums, sv and the final state's row are visible)
    const float tl = part_sum(psum + 1 * MM_MAX_WAVES, NW, lane);
    if (c >= 1) {
        const float tc = part_sum(psum + 0 * MM_MAX_WAVES, NW, lane);
        const bool ok = tc > 0.f;  // mass at frame c: every frame up to c is alive
        const float lt = fast_log2(tc);
        if (sout)
            for (int s = tid; s < S1; s += NT) sout[s] = ok ? (sv[s] - lt) * MM_LN2 : MM_NINF;
        if (wp.lcommit && tid == 0) wp.lcommit[b] = ok ? (float)((Cc + (double)lt) * (double)MM_LN2) : MM_NINF;
    }
    if (tid == 0) {
        double tot;
        if (closed)
            tot = (double)buf[(NF & 1) * S1p + fstate] + C;
        else
            tot = tl > 0.f ? Cl + (double)fast_log2(tl) : (double)MM_NINF;
        wsC[0] = tot;
    }
}

// backward: gamma and ttl.  Same grid and block as the forward kernel.
// (Written out, prologue included, none of the parts and not segment_bwd_body, the segment kernel's loop on the parts: as one body with
// the segment kernel, this kernel's <8,lds> instance measured 0.3 - 0.6 % slower on the large batches in three sessions.)
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_window_bwd_kernel(RunParams p, WindowParams wp) {
    extern __shared__ float4 window_lds4[];
    float *lds = reinterpret_cast<float *>(window_lds4);
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;
    const int S1 = u.S1, S1p = u.S1p, P1 = u.P1, P = P1 - 1, P1p = (P1 + 3) & ~3;
    const int fstate = S1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int NF = len + 1;
    const bool closed = wp.closed ? __builtin_amdgcn_readfirstlane(wp.closed[b]) != 0 : false;
    const WindowLds L = window_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    auto vsync = [&]() {
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    };
    const float *Vb = p.V + (long long)b * p.vsb;
    float *wsA = p.ws_alpha + u.s1p_prefix * (long long)(p.N + 1);
    double *wsC = p.ws_c + (long long)b * (p.N + 2);
    float *bins = lds + L.bins;
    const GraphDev gb = u.g[1];
    const double logZ2 = wsC[0];
    const long long gbase = (long long)b * p.gsb;
    if (!(logZ2 > -1e300) || !(logZ2 < 1e300)) {  // no mass in the window (or no frame): gamma = 0, ttl = -inf
        for (long long q = tid; q < (long long)p.N * P; q += NT) p.gamma[gbase + (q / P) * p.gsn + (q % P) * p.gsp] = 0.f;
        if (p.ttl && tid == 0) p.ttl[b] = MM_NINF;
        return;
    }
    // (the total is finite: len >= 1)
    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    vsync();
    if (closed && tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;  // frame len + 1: the final state alone
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, 1.f);
    {
        const float4 *src = reinterpret_cast<const float4 *>(wsA + (long long)len * S1p);
        float4 *dst = reinterpret_cast<float4 *>(stage + (len & 1) * S1p);
        for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
    }
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f;
    float Enext = 0.f;  // E_{n+1}: out of y_{n+1}, into D
    double Cn = wsC[len], Cpre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions and C_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        Cpre = wsC[f];
    };
    // gamma of frame f from its per-pdf sums (one wave)
    auto finalise = [&](int f) {
        const float *bf = bins + (f & 1) * P1p;
        float s = 0.f;
        for (int q = lane; q < P; q += 64) s += bf[q];
        s = wave_sum(s);
        const float inv = s > 0.f ? 1.f / s : 0.f;
        float *gp = p.gamma + gbase + (long long)(f - 1) * p.gsn;
        for (int q = lane; q < P; q += 64) gp[q * p.gsp] = bf[q] * inv;
    };
    if (len >= 2) prefetch(len - 1);
    for (int n = len; n >= 1; --n) {
        const float *yp = buf + ((n + 1) & 1) * S1p;
        float *yn = buf + (n & 1) * S1p;
        const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
        const float *emn = em + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        D += (double)M + (double)Enext * 1.4426950408889634;
        const float En = frame_emax(emn, P, lane);
        Enext = En;
        const float kappa = (float)(logZ2 - Cn - D);
        if (n < len && wave == NW - 1) finalise(n + 1);
        if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
            if (tid <= P) em[((n - 1) & 1) * P1p + tid] = em_value_nat(evp, n - 1, len, P, tid);
            if (P >= NT) stage_em(em + ((n - 1) & 1) * P1p + NT, Vb + NT, p.vsn, n - 1, len, P - NT, tid, NT, 1.f);
            const float4 *src = reinterpret_cast<const float4 *>(wsA + (long long)(n - 1) * S1p);
            if constexpr (BIGV) {
                float4 *dst = reinterpret_cast<float4 *>(stage + ((n - 1) & 1) * S1p);
                for (int q = tid; q < n4; q += NT) dst[q] = src[q];
            } else {
                const unsigned dst = lds_addr_of(stage + ((n - 1) & 1) * S1p);
                for (int q0 = wave * 64; q0 < n4; q0 += NT)
                    if (q0 + lane < n4) dma_b128(src + q0 + lane, dst + 16u * (unsigned)q0);
            }
            Cn = Cpre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        if (n == len && !closed) {
            // the audio goes on behind the window: b_len = 1 on every real state, nothing on the phony one
            for (int s = tid; s < S1; s += NT) yn[s] = s < fstate ? 0.f : MM_NINF;
        } else {
            // z_n = T (b_{n+1} (*) lhs_{n+1}) into the vector
            for_items<NI>(rg, gb, wave, NW, lane, yp, emn, [&](float v, int row, int, float) { yn[row] = v - M; });
        }
        if constexpr (!BIGV) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of alpha~ of frame n - 1 is in LDS
        vsync();
        // Per pdf, over the pdf's states in pdf_rows (every state is in one list; the phony pdf's holds the final state): the
        // posterior, y_n = b~_n + (e - E_n), the frame's maximum; 8 lanes add a pdf's posteriors in a fixed order, a 3-step DPP
        // reduction ends it.  The second barrier also guards the staging buffers.
        float *bn = bins + (n & 1) * P1p;
        float wm = MM_NINF;
        for (int p0 = wave * 8; p0 < P1; p0 += NW * 8) {
            const int pdf = p0 + (lane >> 3);
            float sacc = 0.f;
            if (pdf < P1) {
                const float e = (emn[pdf] - En) * MM_LOG2E;
                const int e0 = u.pdf_ptr[pdf], e1 = u.pdf_ptr[pdf + 1];
                for (int k = e0 + (lane & 7); k < e1; k += 8) {
                    const int row = u.pdf_rows[k];
                    const float beta = yn[row];
                    sacc += fast_exp2(ast[row] + beta - kappa);
                    const float y = beta + e;
                    yn[row] = y;
                    wm = fmaxf(wm, y);
                }
            }
            sacc = grp_sum(sacc, 3);
            if (pdf < P1 && (lane & 7) == 0) bn[pdf] = sacc;
        }
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        vsync();
    }
    if (wave == 0) finalise(1);
    // zero the frames beyond len
    for (long long q = tid; q < (long long)(p.N - len) * P; q += NT) p.gamma[gbase + (len + q / P) * p.gsn + (q % P) * p.gsp] = 0.f;
    if (p.ttl && tid == 0) p.ttl[b] = (float)(logZ2 * (double)MM_LN2);
}

}  // namespace mm
