// mm_kernel_segment.hip -- segment posteriors (mm_segmentposteriors_f32: the forward-backward of a log batch over a SEGMENT of the
// audio -- it starts from a carried vector like a window and ends open, on the final weights or on a carried END vector, and hands
// the end vector of the segment before it back) on the item form.  Included by mm_segment_tu.hip only.
//
// The forward half is mm_window_fwd_kernel as it stands (mm_kernel_window.hip, launched by mm_launch_window_fwd): the a~ rows and
// C_n of frames 1..len in the workspace, log2 of the open or the closed total in wsC[0].
// mm_segment_bwd_kernel  segment_bwd_body: mm_window_bwd_kernel's loop on the parts of mm_item_parts.hip, with the hooks of SegmentEnd:
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

// what the backward body shares with the hooks of its end
template <int NI>
struct SegmentBwdCtx {
    int b, tid, NT, lane, wave, NW, S1, S1p, fstate, len;
    float *buf, *stage, *em, *part, *psum;
    GraphDev gb;
    ItemRegs<NI> rg;
    double D;     // the float64 offset of the y vector in hand
    float Enext;  // E_{n+1}: out of y_{n+1}, into D
};

// the end of a segment: open, on the final weights or on a carried end vector, and the end vector of the segment before it handed
// back (the hooks of segment_bwd_body)
template <int NI, bool BIGV>
struct SegmentEnd {
    bool carried;      // b_len = exp(end_in)
    bool closed;       // b_len = the final weights
    const float *ein;  // the carried end vector
    float *eout, *lend;
    __device__ __forceinline__ SegmentEnd(const RunParams &p, const SegmentParams &sp) {
        const int b = blockIdx.x;
        const int mode = sp.end_mode ? __builtin_amdgcn_readfirstlane(sp.end_mode[b]) : 0;  // (wave-uniform, as `closed` of a window)
        carried = mode == 2 && sp.end_in != nullptr;
        closed = mode != 0 && !carried;
        ein = carried ? sp.end_in + p.utts[b].state_off : nullptr;
        eout = sp.end_out ? sp.end_out + p.utts[b].state_off : nullptr;
        lend = sp.lend ? sp.lend + b : nullptr;
    }
    // no frame: the segment hands the end vector it was given to the segment before it.  true: the final weights -- the pass
    // behind frame 1 makes them from frame len + 1 = 1, the final state alone
    __device__ __forceinline__ bool no_frame(SegmentBwdCtx<NI> &c) const {
        if (!closed) {
            // (every thread reads what it overwrites: end_in and end_out may be one buffer)
            if (eout)
                for (int s = c.tid; s < c.S1; s += c.NT) eout[s] = carried ? ein[s] : (s < c.fstate ? 0.f : MM_NINF);
            if (lend && c.tid == 0) *lend = 0.f;
            return false;
        }
        for (int q = c.tid; q < 2 * c.S1p; q += c.NT) c.buf[q] = MM_NINF;
        item_vsync<BIGV>();
        if (c.tid == 0) c.buf[1 * c.S1p + c.fstate] = 0.f;
        return true;
    }
    // a carried end: b~_len = end_in log2 e - its maximum (entries at -inf stay there, the phony state keeps its -inf), the maximum
    // in the offset D; the total sum_j a_len(j) b_len(j) relative to its largest term, the waves' sums added in a fixed order
    __device__ __forceinline__ void start(SegmentBwdCtx<NI> &c, double Cn, double &logZ2) const {
        if (!carried) return;
        const int tid = c.tid, NT = c.NT, fstate = c.fstate;
        float *yl = c.buf + (c.len & 1) * c.S1p;
        const float *al = c.stage + (c.len & 1) * c.S1p;
        float wm = MM_NINF;
        for (int s = tid; s < fstate; s += NT) {
            const float v = ein[s] * MM_LOG2E;
            yl[s] = v;
            wm = fmaxf(wm, v);
        }
        part_put(c.part + 0 * MM_MAX_WAVES, c.wave, c.lane, wm);
        item_vsync<BIGV>();
        const float m1 = part_max_dpp(c.part + 0 * MM_MAX_WAVES, c.NW, c.lane);
        wm = MM_NINF;
        for (int s = tid; s < fstate; s += NT) {
            const float v = yl[s] - m1;
            yl[s] = v;
            wm = fmaxf(wm, al[s] + v);
        }
        part_put(c.part + 1 * MM_MAX_WAVES, c.wave, c.lane, wm);
        item_vsync<BIGV>();
        const float m2 = part_max_dpp(c.part + 1 * MM_MAX_WAVES, c.NW, c.lane);
        float sw = 0.f;
        for (int s = tid; s < fstate; s += NT) sw += fast_exp2(al[s] + yl[s] - m2);
        sw = wave_sum(sw);
        if (c.lane == 0) c.psum[c.wave] = sw;
        item_vsync<BIGV>();
        const float tl = part_sum(c.psum, c.NW, c.lane);
        c.D = (double)m1;
        logZ2 = tl > 0.f ? Cn + (double)m1 + (double)m2 + (double)fast_log2(tl) : (double)MM_NINF;
    }
    // no mass in the segment: nothing to hand back either
    __device__ __forceinline__ void no_mass(const SegmentBwdCtx<NI> &c) const {
        if (eout)
            for (int s = c.tid; s < c.S1; s += c.NT) eout[s] = MM_NINF;
        if (lend && c.tid == 0) *lend = MM_NINF;
    }
    // behind frame 1: z_0 = T (b_1 (*) lhs_1) on every row of the extended system (y_1 is in the odd vector, its maximum with the
    // waves; frame 2's vector has been read for the last time).  The final state hands nothing back.
    __device__ __forceinline__ void behind(SegmentBwdCtx<NI> &c) const {
        if (!eout && !lend) return;
        const int tid = c.tid, NT = c.NT, fstate = c.fstate;
        float *y0 = c.buf;
        const float *y1 = c.buf + c.S1p;
        for (int q = tid; q < c.S1p; q += NT) y0[q] = MM_NINF;
        item_vsync<BIGV>();
        const float M = c.len ? part_max_dpp(c.part + 1 * MM_MAX_WAVES, c.NW, c.lane) : 0.f;
        c.D += (double)M + (double)c.Enext * 1.4426950408889634;
        float wm = MM_NINF;
        for_items<NI>(c.rg, c.gb, c.wave, c.NW, c.lane, y1, c.em, [&](float v, int row, int, float) {
            v = row < fstate ? v - M : MM_NINF;
            y0[row] = v;
            wm = fmaxf(wm, v);
        });
        part_put(c.part + 0 * MM_MAX_WAVES, c.wave, c.lane, wm);
        item_vsync<BIGV>();
        const float M0 = segment_part_max_raw(c.part + 0 * MM_MAX_WAVES, c.NW, c.lane);
        const bool ok = M0 > MM_NINF;  // (no state leads into the segment: all -inf, never a NaN)
        if (eout)
            for (int s = tid; s < c.S1; s += NT) eout[s] = ok ? (y0[s] - M0) * MM_LN2 : MM_NINF;
        if (lend && tid == 0) *lend = ok ? (float)((c.D + (double)M0) * (double)MM_LN2) : MM_NINF;
    }
};

// The backward body: mm_window_bwd_kernel's loop on the parts of mm_item_parts.hip, with what the segment's end adds as the hooks of `end`: end.start (the start and the total of a carried end), end.carried at n == len (b~_len is in the vector already), and what is
// handed back -- end.behind (the pass behind frame 1), end.no_frame and end.no_mass where the loop does not run.
template <int NI, bool BIGV, class End>
__device__ __forceinline__ void segment_bwd_body(const RunParams &p, const End &end, float *lds) {
    MM_ITEM_PROLOGUE(BIGV);
    const bool carried = end.carried, closed = end.closed;
    const WindowLds L = window_lds_plan(BIGV ? 0 : S1p, P1p);
    float *em = lds + L.em, *part = lds + L.part, *bins = lds + L.bins;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    float *gam = p.gamma + (long long)b * p.gsb;
    SegmentBwdCtx<NI> c{b, tid, NT, lane, wave, NW, S1, S1p, fstate, len, buf, stage, em, part, lds + L.psum, u.g[1], {}, 0.0, 0.f};
    const GraphDev &gb = c.gb;
    load_item_regs<NI>(c.rg, gb, wave, NW, lane);
    double logZ2 = (double)MM_NINF;
    bool live = len >= 1;
    double Cn = 0.0, Cpre = 0.0;
    if (live) {
        logZ2 = wsC[0];
        for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
        vsync();
        if (closed && tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;  // frame len + 1: the final state alone
        stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, 1.f);
        copy_row(stage + (len & 1) * S1p, wsA + (long long)len * S1p, S1p >> 2, tid, NT);
        vsync();
        Cn = wsC[len];
        end.start(c, Cn, logZ2);
        live = logZ2 > -1e300 && logZ2 < 1e300;  // else: no mass in the window
    }
    if (live) {
        const int n4 = S1p >> 2;
        float evp = 0.f;
        auto prefetch = [&](int f) {  // frame f >= 1: emissions and C_f one step ahead
            evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
            Cpre = wsC[f];
        };
        // gamma of frame f from its per-pdf sums (one wave)
        auto finalise = [&](int f) { finalise_gamma(bins + (f & 1) * P1p, P, P, lane, gam + (long long)(f - 1) * p.gsn, p.gsp); };
        if (len >= 2) prefetch(len - 1);
        for (int n = len; n >= 1; --n) {
            const float *yp = buf + ((n + 1) & 1) * S1p;
            float *yn = buf + (n & 1) * S1p;
            const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
            const float *emn = em + (n & 1) * P1p;
            const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
            c.D += (double)M + (double)c.Enext * 1.4426950408889634;
            const float En = frame_emax(emn, P, lane);
            c.Enext = En;
            const float kappa = (float)(logZ2 - Cn - c.D);
            if (n < len && wave == NW - 1) finalise(n + 1);
            if (n - 1 >= 1) {  // frame n - 1 into the buffers frame n + 1 has left (as mm_log_kernel's PASS 2)
                stage_em_ahead<em_value_nat>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, 1.f);
                stage_row<BIGV>(stage + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
                Cn = Cpre;
                if (n - 2 >= 1) prefetch(n - 2);
            }
            if (n == len && carried) {
                // the segment behind goes on from here: b~_len is in the vector already
            } else if (n == len && !closed) {
                // the audio goes on behind the window: b_len = 1 on every real state, nothing on the phony one
                for (int s = tid; s < S1; s += NT) yn[s] = s < fstate ? 0.f : MM_NINF;
            } else {
                // z_n = T (b_{n+1} (*) lhs_{n+1}) into the vector
                for_items<NI>(c.rg, gb, wave, NW, lane, yp, emn, [&](float v, int row, int, float) { yn[row] = v - M; });
            }
            stage_row_wait<BIGV>();
            vsync();
            // Per pdf, over the pdf's states: the posterior, y_n = b~_n + (e - E_n), the frame's maximum while the posteriors are
            // added up per pdf.  The second barrier also guards the staging buffers.  E_n is kept out of y as it is kept out of a~.
            float wm = MM_NINF;
            for_pdf_rows<1>(u, P1, wave, NW, lane, {bins + (n & 1) * P1p}, [&](int pdf) { return (emn[pdf] - En) * MM_LOG2E; },
                            [&](int row, float e, float(&acc)[1]) {
                                const float beta = yn[row];
                                acc[0] += fast_exp2(ast[row] + beta - kappa);
                                const float y = beta + e;
                                yn[row] = y;
                                wm = fmaxf(wm, y);
                            });
            part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
            vsync();
        }
        if (wave == 0) finalise(1);
    }
    // no frame, or no mass: gamma = 0 on every frame, ttl = -inf; else on the frames beyond len
    zero_gamma_from(gam, p.gsn, p.gsp, live ? len : 0, p.N, P, tid, NT);
    if (p.ttl && tid == 0) p.ttl[b] = live ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    if (!live && len >= 1) {
        end.no_mass(c);
        return;
    }
    if (len == 0 && !end.no_frame(c)) return;
    end.behind(c);
}

// backward: gamma, ttl, end_out and lend.  Grid, block and LDS carve (window_lds_plan) of the window kernels.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_segment_bwd_kernel(RunParams p, SegmentParams sp) {
    extern __shared__ float4 segment_lds4[];
    segment_bwd_body<NI, BIGV>(p, SegmentEnd<NI, BIGV>(p, sp), reinterpret_cast<float *>(segment_lds4));
}

}  // namespace mm
