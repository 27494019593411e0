// mm_kernel_segment.hip -- segment posteriors (mm_segmentposteriors_f32: the forward-backward of a log batch over a SEGMENT of the
// audio -- it starts from a carried vector like a window and ends open, on the final weights or on a carried END vector, and hands
// the end vector of the segment before it back) on the item form.  Included by mm_segment_tu.hip only.
//
// The forward half is mm_window_fwd_kernel as it stands (mm_kernel_window.hip, launched by mm_launch_window_fwd): the a~ rows and
// C_n of frames 1..len in the workspace, log2 of the open or the closed total in wsC[0].
// mm_segment_bwd_kernel  mm_window_bwd_kernel's loop with
//                        - a third start: b~_len = end_in log2 e - its maximum, the maximum in the float64 offset D; the total of a
//                          carried end is taken here, from the stored a~ row of frame len and the end vector (relative to the largest
//                          term, the waves' sums added in a fixed order);
//                        - one more item pass behind frame 1: z_0 = T (b_1 (*) lhs_1) over ALL rows of the extended system, its
//                          maximum, then end_out = ln b_0 - lend and lend = ln max b_0, written coalesced;
//                        - end_mode wave-uniform (readfirstlane), as `closed` is in the window kernels.
//                        A segment of no frame hands its own end vector back: the carried one as given, the open one, or -- by the
//                        same item pass from the final state alone -- the final weights.
//
// Range.  As the window kernels'.  end_out is normalised by its own maximum (largest entry 0), so a chain of segments carries no
// level from one to the next in the vector: the level travels in lend, a float.  A segment without mass (the total zero or not
// finite) never enters the backward loop: gamma = 0, ttl = -inf, end_out = -inf everywhere, lend = -inf.
#pragma once
#include "mm_internal.h"
#include "mm_kernel_window.hip"

namespace mm {

// the largest of the waves' maxima, -inf kept (part_max_dpp turns it into 0): the same bits in every wave
__device__ __forceinline__ float segment_part_max_raw(const float *part, int NW, int lane) {
    float v = (lane < NW) ? part[lane] : MM_NINF;
    v = row16_max(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// backward: gamma, ttl, end_out and lend.  Grid, block and LDS carve (window_lds_plan) of the window kernels.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_segment_bwd_kernel(RunParams p, SegmentParams sp) {
    extern __shared__ float4 segment_lds4[];
    float *lds = reinterpret_cast<float *>(segment_lds4);
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;
    const int S1 = u.S1, S1p = u.S1p, P1 = u.P1, P = P1 - 1, P1p = (P1 + 3) & ~3;
    const int fstate = S1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int NF = len + 1;
    const int mode = sp.end_mode ? __builtin_amdgcn_readfirstlane(sp.end_mode[b]) : 0;
    const bool carried = mode == 2 && sp.end_in != nullptr;  // b_len = exp(end_in)
    const bool closed = mode != 0 && !carried;               // b_len = the final weights
    const WindowLds L = window_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *psum = lds + L.psum, *bins = lds + L.bins;
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
    const float *ein = carried ? sp.end_in + u.state_off : nullptr;
    float *eout = sp.end_out ? sp.end_out + u.state_off : nullptr;
    const GraphDev gb = u.g[1];
    const long long gbase = (long long)b * p.gsb;
    auto zero_gamma = [&](int from) {  // exact zeros on the frames from `from` (0-based) on
        for (long long q = tid; q < (long long)(p.N - from) * P; q += NT) p.gamma[gbase + (from + q / P) * p.gsn + (q % P) * p.gsp] = 0.f;
    };
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0;
    float Enext = 0.f;  // E_{n+1}: out of y_{n+1}, into D

    if (len == 0) {
        // no frame: the segment hands the end vector it was given to the segment before it
        zero_gamma(0);
        if (p.ttl && tid == 0) p.ttl[b] = MM_NINF;
        if (!closed) {
            // (every thread reads what it overwrites: end_in and end_out may be one buffer)
            if (eout)
                for (int s = tid; s < S1; s += NT) eout[s] = carried ? ein[s] : (s < fstate ? 0.f : MM_NINF);
            if (sp.lend && tid == 0) sp.lend[b] = 0.f;
            return;
        }
        // the final weights: the item pass below from frame len + 1 = 1, the final state alone
        for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
        vsync();
        if (tid == 0) buf[1 * S1p + fstate] = 0.f;
    } else {
        double logZ2 = wsC[0];
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
        double Cn = wsC[len];
        if (carried) {
            // b~_len = end_in log2 e - its maximum (entries at -inf stay there, the phony state keeps its -inf); the total
            // sum_j a_len(j) b_len(j) relative to its largest term
            float *yl = buf + (len & 1) * S1p;
            const float *al = stage + (len & 1) * S1p;
            float wm = MM_NINF;
            for (int s = tid; s < fstate; s += NT) {
                const float v = ein[s] * MM_LOG2E;
                yl[s] = v;
                wm = fmaxf(wm, v);
            }
            part_put(part + 0 * MM_MAX_WAVES, wave, lane, wm);
            vsync();
            const float m1 = part_max_dpp(part + 0 * MM_MAX_WAVES, NW, lane);
            wm = MM_NINF;
            for (int s = tid; s < fstate; s += NT) {
                const float v = yl[s] - m1;
                yl[s] = v;
                wm = fmaxf(wm, al[s] + v);
            }
            part_put(part + 1 * MM_MAX_WAVES, wave, lane, wm);
            vsync();
            const float m2 = part_max_dpp(part + 1 * MM_MAX_WAVES, NW, lane);
            float sw = 0.f;
            for (int s = tid; s < fstate; s += NT) sw += fast_exp2(al[s] + yl[s] - m2);
            sw = wave_sum(sw);
            if (lane == 0) psum[wave] = sw;
            vsync();
            const float tl = window_part_sum(psum, NW, lane);
            D = (double)m1;
            logZ2 = tl > 0.f ? Cn + (double)m1 + (double)m2 + (double)fast_log2(tl) : (double)MM_NINF;
        }
        if (!(logZ2 > -1e300) || !(logZ2 < 1e300)) {  // no mass in the segment: nothing to hand back either
            zero_gamma(0);
            if (p.ttl && tid == 0) p.ttl[b] = MM_NINF;
            if (eout)
                for (int s = tid; s < S1; s += NT) eout[s] = MM_NINF;
            if (sp.lend && tid == 0) sp.lend[b] = MM_NINF;
            return;
        }
        const int n4 = S1p >> 2;
        float evp = 0.f;
        double Cpre = 0.0;
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
            const float En = filter_emax(emn, P, lane);
            Enext = En;
            const float kappa = (float)(logZ2 - Cn - D);
            if (n < len && wave == NW - 1) finalise(n + 1);
            if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_window_bwd_kernel)
                if (tid <= P) em[((n - 1) & 1) * P1p + tid] = filter_em_value(evp, n - 1, len, P, tid);
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
            if (n == len && carried) {
                // the segment behind goes on from here: b~_len is in the vector already
            } else if (n == len && !closed) {
                // the audio goes on behind the segment: b_len = 1 on every real state, nothing on the phony one
                for (int s = tid; s < S1; s += NT) yn[s] = s < fstate ? 0.f : MM_NINF;
            } else {
                // z_n = T (b_{n+1} (*) lhs_{n+1}) into the vector
                for_items<NI>(rg, gb, wave, NW, lane, yp, emn, [&](float v, int row, int, float) { yn[row] = v - M; });
            }
            if constexpr (!BIGV) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of alpha~ of frame n - 1 is in LDS
            vsync();
            // per pdf, over the pdf's states (as mm_window_bwd_kernel): the posterior, y_n = b~_n + (e - E_n), the frame's maximum
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
        zero_gamma(len);
        if (p.ttl && tid == 0) p.ttl[b] = (float)(logZ2 * (double)MM_LN2);
    }
    if (!eout && !sp.lend) return;
    // behind frame 1: z_0 = T (b_1 (*) lhs_1) on every row of the extended system (y_1 is in the odd vector, its maximum with the
    // waves; frame 2's vector has been read for the last time).  The final state hands nothing back.
    float *y0 = buf;
    const float *y1 = buf + S1p;
    for (int q = tid; q < S1p; q += NT) y0[q] = MM_NINF;
    vsync();
    const float M = len ? part_max_dpp(part + 1 * MM_MAX_WAVES, NW, lane) : 0.f;
    D += (double)M + (double)Enext * 1.4426950408889634;
    float wm = MM_NINF;
    for_items<NI>(rg, gb, wave, NW, lane, y1, em, [&](float v, int row, int, float) {
        v = row < fstate ? v - M : MM_NINF;
        y0[row] = v;
        wm = fmaxf(wm, v);
    });
    part_put(part + 0 * MM_MAX_WAVES, wave, lane, wm);
    vsync();
    const float M0 = segment_part_max_raw(part + 0 * MM_MAX_WAVES, NW, lane);
    const bool ok = M0 > MM_NINF;  // (no state leads into the segment: all -inf, never a NaN)
    if (eout)
        for (int s = tid; s < S1; s += NT) eout[s] = ok ? (y0[s] - M0) * MM_LN2 : MM_NINF;
    if (sp.lend && tid == 0) sp.lend[b] = ok ? (float)((D + (double)M0) * (double)MM_LN2) : MM_NINF;
}

}  // namespace mm
