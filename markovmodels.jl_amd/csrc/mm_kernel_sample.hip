// mm_kernel_sample.hip -- posterior path sampling (forward filtering, backward sampling) on the sampling form.
// Included by mm_sample_tu.hip only.
//
// The forward half is mm_log_kernel<MODE_FB, NI, 1> as pdfposteriors runs it: it leaves the normalised alpha~ rows and log2 Z
// (wsC[0]) in the workspace.  mm_sample_kernel then walks the frames backwards, one CHAIN per sample (b, k): with j the state of
// frame n + 1 (the phony final state at n = len), it draws the state i of frame n with probability proportional to
//     2^(alpha~_n[i] + w_ij)        over the in-arcs i -> j of the sampling form
// (the per-frame normaliser of alpha~ is common to all i: it cancels, so the walk needs no beta, no offsets and no range
// handling).  A wave runs a chain; the lanes take the in-arcs of j in chunks of 64.  Inside a chunk the draw is an inverse CDF
// (2^(x - max), DPP inclusive scan, one uniform, the first lane past the target); across chunks the running choice is replaced by
// the chunk's with probability chunk total / running total (a second uniform).  A lane of probability zero is never taken: the
// test of a lane asks for its own term to be positive, and when rounding leaves no lane past the target the last positive lane is
// taken.
// Workgroup (b, y) runs the chains k = y * NW * CW + c * NW + wave, c < CW, of utterance b, their state in registers (CW = 1, 2,
// 4 or 8 chains per wave: the fewest that keep all workgroups of the call resident at once -- a wave's chains take turns, so
// fewer chains per wave and more waves per compute unit is faster while there is room).  The row alpha~_(n-1) comes into LDS
// by DMA while frame n is drawn (STAGE; one row load serves all chains of the workgroup; the staging is done by the waves
// without a chain: a ninth wave that never has one, and the idle ones when K is small); without STAGE (graphs beyond the LDS)
// the lanes gather alpha~ from global memory and the waves never meet.  The uniforms come from Philox-4x32-10, key = seed,
// counter = (b, k, frame, chunk): no generator state, so a sample depends on its indices alone (the words of the first chunk
// are computed 64 at a time, a frame and a chain per lane).  Results leave through vector stores, the paths 64 frames at a time.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"
#include "mm_philox.h"  // philox_4x32_10, unit_open

namespace mm {

#define MM_DPP_ROW_SHR(n) (0x110 + (n))
#define MM_DPP_ROW_BCAST15 0x142
#define MM_DPP_ROW_BCAST31 0x143
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v) {  // v + (the lane CTRL names, 0 where there is none / in the rows not in ROWS)
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xF, CTRL != MM_DPP_ROW_BCAST15 && CTRL != MM_DPP_ROW_BCAST31));
}
// inclusive prefix sums over the 64 lanes
__device__ __forceinline__ float wave_iscan(float v) {
    v = dpp_add<MM_DPP_ROW_SHR(1), 0xF>(v);
    v = dpp_add<MM_DPP_ROW_SHR(2), 0xF>(v);
    v = dpp_add<MM_DPP_ROW_SHR(4), 0xF>(v);
    v = dpp_add<MM_DPP_ROW_SHR(8), 0xF>(v);
    v = dpp_add<MM_DPP_ROW_BCAST15, 0xA>(v);
    v = dpp_add<MM_DPP_ROW_BCAST31, 0xC>(v);
    return v;
}
__device__ __forceinline__ float lane_value(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
// the maximum over the 64 lanes, in every lane: the scan's six steps as v_max_f32_dpp (a lane the step names no source for
// keeps its value) and one v_readlane -- no trip through the LDS crossbar
#define MM_SCAN_MAX(ctrl) asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " ctrl " bank_mask:0xf" : "+v"(v))
__device__ __forceinline__ float wave_max_scan(float v) {
    MM_SCAN_MAX("row_shr:1 row_mask:0xf");
    MM_SCAN_MAX("row_shr:2 row_mask:0xf");
    MM_SCAN_MAX("row_shr:4 row_mask:0xf");
    MM_SCAN_MAX("row_shr:8 row_mask:0xf");
    MM_SCAN_MAX("row_bcast:15 row_mask:0xa");
    MM_SCAN_MAX("row_bcast:31 row_mask:0xc");
    return lane_value(v, 63);
}

__device__ __forceinline__ SampleRec load_sample_rec(const SampleRec *p) {
    const int4 r = *reinterpret_cast<const int4 *>(p);
    SampleRec s;
    s.src = r.x;
    s.w = __int_as_float(r.y);
    s.start = r.z;
    s.deg = r.w;
    return s;
}

template <bool STAGE, int CW>
__global__ void __launch_bounds__(64 * (MM_SAMPLE_NW + 1)) mm_sample_kernel(RunParams p, SampleParams sp) {
    extern __shared__ float lds[];
    // (not MM_ITEM_PROLOGUE: the block's shape is a compile-time constant here, and a workgroup is a set of chains, not an utterance)
    constexpr int NW = MM_SAMPLE_NW, NT = 64 * (NW + 1);  // NW waves for the chains + one that only stages
    constexpr int FR = 64 / CW;                           // frames whose random words one vector evaluation of the generator makes
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S1p = u.S1p;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int k0 = blockIdx.y * (NW * CW);
    const int nch = sp.K - k0 < NW * CW ? sp.K - k0 : NW * CW;  // chains of this workgroup
    const double logZ2 = p.ws_c[(long long)b * (p.N + 2)];
    const bool haspath = logZ2 > -1e300;
    const bool ok = haspath && len >= 1;
    int *const pb = sp.paths + (long long)b * sp.psb;
    float *const lpb = sp.logprob ? sp.logprob + (long long)b * sp.lsb : nullptr;
    if (sp.ttl && blockIdx.y == 0 && tid == 0) sp.ttl[b] = haspath ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    // frames beyond the length (every frame of an utterance without a path)
    for (int c = 0; c < nch; ++c)
        for (int f = (ok ? len : 0) + tid; f < p.N; f += NT) pb[(long long)(k0 + c) * sp.psk + f] = -1;
    if (!ok) {  // (the empty path of an utterance of no frames has probability one)
        if (lpb)
            for (int c = tid; c < nch; c += NT) lpb[k0 + c] = haspath ? 0.f : MM_NINF;
        return;
    }
    const float *Vb = p.V + (long long)b * p.vsb;
    const float *wsA = p.ws_alpha + u.s1p_prefix * (long long)(p.N + 1);
    const SampleDev sd = sp.forms[b];
    const SampleRec *recs = sd.recs;
    const int nact = nch < NW ? nch : NW;  // waves that have a chain
    // who brings the rows in: the waves without a chain -- the last wave never has one.  A wave that draws never waits for a row
    // but at the frame's barrier (its own loads share vmcnt with whatever DMA it issued)
    const int sn = NW + 1 - nact, sw = wave - nact;
    const int n4 = S1p >> 2;
    auto stage_frame = [&](int f) {  // alpha~ of frame f into its half of the LDS, by the sn waves without a chain
        stage_row<false>(lds + (f & 1) * S1p, wsA + (long long)f * S1p, n4, tid, sn * 64, sw, lane);
    };
    if constexpr (STAGE) {
        if (sw >= 0) stage_frame(len);
        stage_row_wait<false>();
        __syncthreads();
    }
    // the chains' state: the state drawn last (the final state to begin with) as its in-list, the path's last 64 frames (lane
    // f & 63 holds frame f), the float64 log-probability (natural log) as per-lane partial sums: lane 0 adds the transitions frame
    // by frame, every lane the emission of its frame when 64 frames of the path are complete (one gather per lane and 64 frames,
    // off the chain's critical path, instead of two dependent loads per frame)
    int cur[CW], start[CW], deg[CW], pend[CW];
    double lp[CW];
    SampleRec r[CW];
    const int *const s2p = u.s2p;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        cur[c] = -1;
        start[c] = sd.fin_start;
        deg[c] = sd.fin_deg;
        pend[c] = -1;
        lp[c] = 0.0;
    }
    // the generator's words of the first chunk of FR frames x CW chains at a time, one (frame, chain) per lane: computed by the
    // scalar unit, which the waves of a compute unit share, ten rounds per chain and frame held every wave back
    static_assert(CW == 1 || CW == 2 || CW == 4 || CW == 8, "lane = chain + CW * frame");
    unsigned rx = 0, ry = 0;
    for (int n = len; n >= 1; --n) {
        const float *arow = STAGE ? lds + (n & 1) * S1p : wsA + (long long)n * S1p;
        const int ph = (len - n) & (FR - 1);
        if (ph == 0 && wave < nact) {
            const uint2 rnd = philox_4x32_10(sp.key0, sp.key1, (unsigned)b, (unsigned)(k0 + (lane % CW) * NW + wave), (unsigned)(n - lane / CW), 0u);
            rx = rnd.x;
            ry = rnd.y;
        }
        if (wave < nact) {  // the first chunk of every chain's in-list: all the loads in flight together
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                r[c].src = 0;
                r[c].w = MM_NINF;
                r[c].start = r[c].deg = 0;
                if (c * NW + wave < nch && lane < deg[c]) r[c] = load_sample_rec(recs + start[c] + lane);
            }
        }
        if constexpr (STAGE)
            if (n > 1 && sw >= 0) stage_frame(n - 1);
        if (wave < nact) {
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c * NW + wave >= nch) continue;
                const int k = k0 + c * NW + wave;
                float M = MM_NINF, R = 0.f;
                bool have = false;
                int c_src = -1, c_start = 0, c_deg = 0;
                float c_w = 0.f;
                const int dg = deg[c];
                for (int o = 0; o < dg; o += 64) {
                    SampleRec rc = r[c];
                    if (o > 0) {
                        rc.src = 0;
                        rc.w = MM_NINF;
                        rc.start = rc.deg = 0;
                        if (o + lane < dg) rc = load_sample_rec(recs + start[c] + o + lane);
                    }
                    const float x = o + lane < dg ? arow[rc.src] + rc.w : MM_NINF;
                    const float mc = wave_max_scan(x);
                    if (!(mc > MM_NINF)) continue;  // nothing alive in this chunk
                    const float Mn = fmaxf(M, mc);
                    const float e = fast_exp2(x - Mn);
                    const float cum = wave_iscan(e);
                    const float T = lane_value(cum, 63);
                    R = (M > MM_NINF ? R * fast_exp2(M - Mn) : 0.f) + T;
                    M = Mn;
                    uint2 rnd;
                    if (o == 0) {
                        rnd.x = (unsigned)__builtin_amdgcn_readlane((int)rx, c + CW * ph);
                        rnd.y = (unsigned)__builtin_amdgcn_readlane((int)ry, c + CW * ph);
                    } else {
                        rnd = philox_4x32_10(sp.key0, sp.key1, (unsigned)b, (unsigned)k, (unsigned)n, (unsigned)(o >> 6));
                    }
                    if (!have || unit_open(rnd.y) * R < T) {
                        const float target = unit_open(rnd.x) * T;
                        const unsigned long long pos = __ballot(e > 0.f);
                        const unsigned long long hit = __ballot(e > 0.f && cum > target);
                        if (pos) {
                            const int sel = hit ? __builtin_ctzll(hit) : 63 - __builtin_clzll(pos);
                            c_src = __builtin_amdgcn_readlane(rc.src, sel);
                            c_w = lane_value(rc.w, sel);
                            c_start = __builtin_amdgcn_readlane(rc.start, sel);
                            c_deg = __builtin_amdgcn_readlane(rc.deg, sel);
                            have = true;
                        }
                    }
                }
                // (a chain that finds nothing alive -- not possible behind a finite log Z in exact arithmetic -- ends: -1, -inf)
                cur[c] = c_src;
                start[c] = c_start;
                deg[c] = c_deg;
                if (lane == ((n - 1) & 63)) pend[c] = c_src;
                if (lpb && lane == 0) lp[c] += have ? (double)c_w * (double)MM_LN2 : (double)MM_NINF;
                if (((n - 1) & 63) == 0) {
                    const int f = n - 1 + lane;
                    if (f < len) {
                        pb[(long long)k * sp.psk + f] = pend[c];
                        if (lpb && pend[c] >= 0) lp[c] += (double)Vb[(long long)f * p.vsn + s2p[pend[c]]];
                    }
                }
            }
        }
        if constexpr (STAGE) {
            stage_row_wait<false>();  // this wave's part of alpha~ of frame n - 1 is in LDS
            __syncthreads();
        }
    }
    if (lpb && wave < nact) {
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (c * NW + wave >= nch) continue;
            const double a = cur[c] >= 0 ? (double)u.init[cur[c]] * (double)MM_LN2 : (double)MM_NINF;
            double t = lp[c];
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m);
            if (lane == 0) lpb[k0 + c * NW + wave] = (float)(t + a - logZ2 * (double)MM_LN2);
        }
    }
}

}  // namespace mm
