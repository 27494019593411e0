// mm_kernel_weighted.hip -- posteriors with call-time arc weights (mm_weightedposteriors_f32) on the item form.
// Included by mm_weighted_tu.hip only.
//
// The topology, the item forms and every plan stay the batch's; what a call brings is the arc log-weights W and the initial
// log-weights W_init as device tensors.  Four launches:
//   mm_weights_kernel           the call's copies of the {col, w} arrays of both item forms with w = W[k] * log2 e in every real
//                               slot, the dense init vector from W_init, and the call's copy of the utterance descriptors whose
//                               g[0].slots, g[1].slots and init point at them (nothing else of a descriptor changes)
//   mm_log_kernel<MODE_FB,NI,1> the item kernel's forward half, unchanged, on the call's descriptors
//   mm_weighted_bwd_kernel      mm_arc_kernel's backward recursion with its per-slot sums; the state posteriors q the row epilogue
//                               forms anyway also go to a row of their own, and a per-pdf pass over the pdf -> states lists (the
//                               item kernel's deterministic pass) turns the row into gamma
//   mm_weighted_scatter_kernel  counts in the caller's entry order, the phony self-loop's frames, init_counts, ttl
// No atomics anywhere: every slot, every state and every pdf has one owner, the sums run in a fixed order.
#pragma once
#include "mm_internal.h"
#include "mm_kernels.hip"

namespace mm {

#define MM_WEIGHTED_FLUSH 32  // frames between the flushes of the register partial sums (MM_ARC_FLUSH of mm_kernel_arcs.hip)

// grid (B, blocks), block 256.  One thread owns each slot of a plane and each state of an init vector; reads of the own slots and
// writes of the planes are coalesced, W is gathered through slot2k.
__global__ void __launch_bounds__(256) mm_weights_kernel(RunParams p, WeightedParams wp) {
    const int b = blockIdx.x;
    const UttDesc &u = wp.utts_own[b];
    const WeightDev wd = wp.wforms[b];
    const int t0 = blockIdx.y * blockDim.x + threadIdx.x, ts = gridDim.y * blockDim.x;
    const bool shared_w = wp.wsb == 0, shared_i = wp.wisb == 0;
    if (wp.W && (!shared_w || b == 0)) {
        const float *Wb = wp.W + (long long)b * wp.wsb;
        for (int d = 0; d < 2; ++d) {
            const Slot *own = u.g[d].slots;
            Slot *dst = wp.plane[d] + (shared_w ? 0 : wd.plane_off[d]);
            const int *s2k = wd.slot2k[d];
            for (int s = t0; s < wd.nslots[d]; s += ts) {
                Slot sl = load_slot(own + s);
                const int k = s2k[s];
                if (k >= 0) sl.w = Wb[k] * MM_LOG2E;
                *reinterpret_cast<uint2 *>(dst + s) = make_uint2(sl.col, __float_as_uint(sl.w));
            }
        }
    }
    if (wp.W_init && (!shared_i || b == 0)) {
        const float *Wi = wp.W_init + (long long)b * wp.wisb;
        float *dst = wp.init_plane + (shared_i ? 0 : u.s1p_prefix);
        for (int s = t0; s < u.S1p; s += ts) {
            const int m = s < u.S1 ? wd.state2init[s] : -1;
            dst[s] = m >= 0 ? Wi[m] * MM_LOG2E : MM_NINF;
        }
    }
    if (blockIdx.y == 0) {  // the call's descriptor: a copy through LDS, where one thread sets the three pointers
        static_assert(sizeof(UttDesc) % 4 == 0, "UttDesc is copied by words");
        __shared__ UttDesc c;
        const unsigned *src = reinterpret_cast<const unsigned *>(&u);
        unsigned *mid = reinterpret_cast<unsigned *>(&c);
        unsigned *dst = reinterpret_cast<unsigned *>(&wp.utts_call[b]);
        for (int q = threadIdx.x; q < (int)(sizeof(UttDesc) / 4); q += blockDim.x) mid[q] = src[q];
        __syncthreads();
        if (threadIdx.x == 0) {
            if (wp.W) {
                c.g[0].slots = wp.plane[0] + (shared_w ? 0 : wd.plane_off[0]);
                c.g[1].slots = wp.plane[1] + (shared_w ? 0 : wd.plane_off[1]);
            }
            if (wp.W_init) c.init = wp.init_plane + (shared_i ? 0 : u.s1p_prefix);
        }
        __syncthreads();
        for (int q = threadIdx.x; q < (int)(sizeof(UttDesc) / 4); q += blockDim.x) dst[q] = mid[q];
    }
}

// (Written out, none of the parts of mm_item_parts.hip: measured, every way of moving this kernel onto them costs the entry up to 1 % of
// a call -- it sits at the register ceiling with 210 spilled scalars, and the compiler lays the whole time loop out anew.)
template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_weighted_bwd_kernel(RunParams p, WeightedParams wp) {
    extern __shared__ float lds[];
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;
    const int S1p = u.S1p, P1 = u.P1, P = P1 - 1, P1p = (P1 + 3) & ~3;
    const int fstate = u.S1 - 1;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const int NF = len + 1;
    const bool want_c = wp.counts != nullptr, want_g = p.gamma != nullptr;  // (kernel arguments: wave-uniform)
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *bins = lds + L.bins, *part = lds + L.part;
    float *psum = lds + L.total;  // [2][MM_MAX_WAVES] the waves' sums of the state posteriors of a frame (LDS behind the plan)
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    auto vsync = [&]() {
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if constexpr (BIGV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    };
    const float *Vb = p.V + (long long)b * p.vsb;
    const float *wsA = p.ws_alpha + u.s1p_prefix * (long long)(p.N + 1);
    const double *wsC = p.ws_c + (long long)b * (p.N + 2);
    const GraphDev gb = u.g[1];
    double *acc = wp.acc + wp.arcs[b].slot_off;
    float *post1 = wp.post1 + u.s1p_prefix;
    // the state posteriors of the frame in hand, one float per state: rows without arcs have no item and stay 0 for good (so the
    // row cannot be alpha~'s staging buffer, as in the item kernel's deterministic mode).  BIGV: the post1 row itself -- it ends
    // with frame 1's posteriors
    float *qb = BIGV ? post1 : psum + 2 * MM_MAX_WAVES;
    const long long gbase = (long long)b * p.gsb;
    const double logZ2 = wsC[0];
    if (!(logZ2 > -1e300) || len < 1) {  // no accepting path, or no frame: gamma = 0; mm_weighted_scatter_kernel writes the rest
        if (want_g)
            for (long long q = tid; q < (long long)p.N * P; q += NT) p.gamma[gbase + (q / P) * p.gsn + (q % P) * p.gsp] = 0.f;
        return;
    }

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    for (int s = tid; s < S1p; s += NT) qb[s] = 0.f;
    if constexpr (!BIGV)
        for (int s = tid; s < u.S1; s += NT) post1[s] = 0.f;
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    {
        const float4 *src = reinterpret_cast<const float4 *>(wsA + (long long)len * S1p);
        float4 *dst = reinterpret_cast<float4 *>(stage + (len & 1) * S1p);
        for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
    }
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    float facc[NI > 0 ? NI : 1][4];
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        facc[i][0] = facc[i][1] = facc[i][2] = facc[i][3] = 0.f;
    });
    const int resident = NI * NW < gb.n_short ? NI * NW : gb.n_short;
    double D = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f;
    double Cn = wsC[len], Cpre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions and C_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        Cpre = wsC[f];
    };
    // gamma of a frame from its per-pdf sums: over their sum, so that the frame adds up to 1 whatever alpha~'s rounding left
    auto put_gamma = [&](int f) {  // frame f >= 1 -> 0-based index f - 1; one wave
        const float *bf = bins + (f & 1) * P1p;
        float s = 0.f;
        for (int q = lane; q < P1; q += 64) s += bf[q];
        s = wave_sum(s);
        const float inv = s > 0.f ? 1.f / s : 0.f;
        float *gp = p.gamma + gbase + (long long)(f - 1) * p.gsn;
        for (int q = lane; q < P; q += 64) gp[q * p.gsp] = bf[q] * inv;
    };
    if (len >= 2) prefetch(len - 1);
    int nflush = 0;
    float corr = 0.f;  // log2 of the state posteriors' sum of frame n + 1 (1 in exact arithmetic)
    for (int n = len; n >= 1; --n) {
        const float *yp = buf + ((n + 1) & 1) * S1p;
        float *yn = buf + (n & 1) * S1p;
        const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
        const float *emn = em + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        if (n < len) {
            float s = 0.f;
            for (int w = 0; w < NW; ++w) s += psum[((n + 1) & 1) * MM_MAX_WAVES + w];
            if (s > 0.f) corr += fast_log2(s);
        }
        // (the frame n + 1 sum corrects frame n, as in mm_arc_kernel: what is left is one step's drift)
        const float kappa = (float)(logZ2 - Cn - D + (double)corr);
        const float sh = -M - kappa;  // arc term of slot k of row i: 2^(alpha~_n[i] + sh + x_k), x_k = w_k + y_{n+1}[col_k]
        if (want_g && n < len && wave == NW - 1) put_gamma(n + 1);  // (the per-pdf sums of frame n + 1: behind step n + 1's last barrier)
        if (n - 1 >= 1) {  // frame n-1 into the buffers frame n+1 has left (as mm_log_kernel's PASS 2)
            if (tid <= P) em[((n - 1) & 1) * P1p + tid] = em_value(evp, n - 1, len, P, tid);
            if (P >= NT) stage_em(em + ((n - 1) & 1) * P1p + NT, Vb + NT, p.vsn, n - 1, len, P - NT, tid, NT, MM_LOG2E);
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
        float wm = MM_NINF, qs = 0.f;
        // the leader lane of a row group: beta~_n, y_n = beta~_n + e_n, the state posterior (summed; into its row; kept at frame 1)
        auto epi = [&](float v, int row, float e) {
            const float beta = v - M;
            const float q = fast_exp2(ast[row] + beta - kappa);
            qs += q;
            qb[row] = q;
            if constexpr (!BIGV)
                if (n == 1) post1[row] = q;
            const float y = beta + e;
            yn[row] = y;
            wm = max_nc(wm, y);
        };
        static_for<0, NI>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const int meta = rg.meta[i];
            if (meta != 0) {
                int R = meta & 0xff, lg = meta >> 8;
                asm volatile("" : "+s"(R), "+s"(lg));
                const unsigned row = rg.ri[i] & 0xffffu;
                const bool real = row != 0xffffu;
                const float e = emn[real ? (rg.ri[i] >> 16) : 0u];
                const float base = real ? ast[row] + sh : MM_NINF;
                const unsigned c01 = rg.c[i][0], c23 = rg.c[i][1];
                const float x0 = rg.w[i][0] + yp[c01 & 0xffffu];
                const float x1 = rg.w[i][1] + yp[c01 >> 16];
                float x2 = MM_NINF, x3 = MM_NINF;
                if (R > 2) {
                    x2 = rg.w[i][2] + yp[c23 & 0xffffu];
                    x3 = rg.w[i][3] + yp[c23 >> 16];
                }
                float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
                m = grp_max_rt(m, lg);
                const float m0 = (m > MM_NINF) ? m : 0.f;
                float sum = fast_exp2(x0 - m0) + fast_exp2(x1 - m0);
                if (R > 2) sum += fast_exp2(x2 - m0) + fast_exp2(x3 - m0);
                sum = grp_sum_rt(sum, lg);
                if (want_c) {
                    facc[i][0] += fast_exp2(x0 + base);
                    facc[i][1] += fast_exp2(x1 + base);
                    if (R > 2) {
                        facc[i][2] += fast_exp2(x2 + base);
                        facc[i][3] += fast_exp2(x3 + base);
                    }
                }
                if (real && (lane & ((1 << lg) - 1)) == 0) epi(m0 + fast_log2(sum), (int)row, e);
            }
        });
        // items beyond the register window, and long rows: streamed from L2, their sums in the float64 workspace
        for (int it = wave; it < gb.n_items; it += NW) {
            if (it < resident) continue;
            const ItemMeta im = load_item(gb.items, it);
            const RowInfo r = gb.rowinfo[(size_t)it * 64 + lane];
            const float e = emn[r.row >= 0 ? r.pdf : 0];
            const float v = lse_item(gb.slots, im, lane, yp);
            if (want_c) {
                const float base = r.row >= 0 ? ast[r.row] + sh : MM_NINF;
                const Slot *sp = gb.slots + (size_t)im.slot_row * 64 + lane;
                double *dp = acc + (size_t)im.slot_row * 64 + lane;
                for (int k = 0; k < im.R; ++k) {
                    const Slot s = load_slot(sp + k * 64);
                    const double t = (double)fast_exp2(s.w + yp[s.col] + base);
                    dp[k * 64] = (n == len ? 0.0 : dp[k * 64]) + t;
                }
            }
            if (r.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) epi(v, r.row, e);
        }
        if constexpr (NI > 0) {
            if (want_c && ((len - n) % MM_WEIGHTED_FLUSH == MM_WEIGHTED_FLUSH - 1 || n == 1)) {  // the register partial sums into the workspace
                static_for<0, NI>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    const int meta = rg.meta[i];
                    if (meta != 0) {
                        const int R = meta & 0xff;
                        const ItemMeta im = load_item(gb.items, wave + i * NW);
                        double *dp = acc + (size_t)im.slot_row * 64 + lane;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < R) {
                                dp[k * 64] = (nflush == 0 ? 0.0 : dp[k * 64]) + (double)facc[i][k];
                                facc[i][k] = 0.f;
                            }
                    }
                });
                ++nflush;
            }
        }
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        qs = wave_sum(qs);
        if (lane == 0) psum[(n & 1) * MM_MAX_WAVES + wave] = qs;
        if constexpr (!BIGV) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of alpha~ of frame n - 1 is in LDS
        vsync();
        if (want_g) {
            // C' * (A .* B) without atomics, as the item kernel's deterministic mode: a pdf's states are listed in pdf_rows; 8 lanes
            // per pdf add their posteriors in a fixed order, a 3-step DPP reduction ends it.  The second barrier guards the row (the
            // next step's epilogues write it) and publishes the sums to the wave that finishes the frame.
            float *bn = bins + (n & 1) * P1p;
            for (int p0 = wave * 8; p0 < P1; p0 += NW * 8) {
                const int pdf = p0 + (lane >> 3);
                float sacc = 0.f;
                if (pdf < P1) {
                    const int e0 = u.pdf_ptr[pdf], e1 = u.pdf_ptr[pdf + 1];
                    for (int k = e0 + (lane & 7); k < e1; k += 8) sacc += qb[u.pdf_rows[k]];
                }
                sacc = grp_sum(sacc, 3);
                if (pdf < P1 && (lane & 7) == 0) bn[pdf] = sacc;
            }
            vsync();
        }
    }
    if (want_g) {  // frame 1, and the frames beyond len
        if (wave == 0) put_gamma(1);
        for (long long q = tid; q < (long long)(p.N - len) * P; q += NT) p.gamma[gbase + (len + q / P) * p.gsn + (q % P) * p.gsp] = 0.f;
    }
}

// counts in the caller's entry order, initial-state counts, ttl (mm_arc_scatter_kernel's job; counts may be NULL).
// grid (B, blocks), block 256.
__global__ void __launch_bounds__(256) mm_weighted_scatter_kernel(RunParams p, WeightedParams wp) {
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const ArcDev ad = wp.arcs[b];
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const double logZ2 = p.ws_c[(long long)b * (p.N + 2)];
    const bool ok = logZ2 > -1e300;
    const double *acc = wp.acc + ad.slot_off;
    const int t0 = blockIdx.y * blockDim.x + threadIdx.x, ts = gridDim.y * blockDim.x;
    if (wp.counts) {
        float *cb = wp.counts + (long long)b * wp.csb;
        for (int k = t0; k < ad.nnz; k += ts) {
            float c = 0.f;
            if (ok) {
                const int s = ad.k2slot[k];
                double v = (s >= 0 && len >= 1) ? acc[s] : 0.0;
                if (k == ad.kphony) v += (double)(p.N - len);  // frames len+1 .. N: only the final state is alive
                c = (float)v;
            }
            cb[k] = c;
        }
    }
    if (wp.init_counts) {
        // frame 1's posteriors over their sum (the block's threads add them in a fixed order: the same bits on every run)
        __shared__ float red[256];
        float s1 = 0.f;
        if (ok && len >= 1)
            for (int s = threadIdx.x; s < u.S1; s += blockDim.x) s1 += wp.post1[u.s1p_prefix + s];
        red[threadIdx.x] = s1;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        const float inv = red[0] > 0.f ? 1.f / red[0] : 0.f;
        float *ib = wp.init_counts + (long long)b * wp.isb;
        for (int m = t0; m < ad.n_init; m += ts) {
            const int s = ad.init_states[m];
            float c = 0.f;
            if (ok) c = len >= 1 ? wp.post1[u.s1p_prefix + s] * inv : (s == u.S1 - 1 ? 1.f : 0.f);
            ib[m] = c;
        }
    }
    if (wp.ttl && t0 == 0) wp.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
}

}  // namespace mm
