// mm_kernel_arcs.hip -- arc posteriors (expected transition counts, Baum-Welch's xi summed over the frames) on the item form.
// Included by mm_arcs_tu.hip only.
//
// The forward half is mm_log_kernel<MODE_FB, NI, 1> as pdfposteriors runs it: it leaves the normalised alpha~ rows, the float64
// offsets C_n and log2 Z (wsC[0]) in the workspace.  mm_arc_kernel then runs the beta~ recursion of mm_log_kernel's PASS 2 over
// the backward (T_hat) item form, whose rows are the SOURCE states, and at every frame n adds to each arc slot it holds
//     2^(alpha~_n[i] + w_ij + e_{n+1}[j] + beta~_{n+1}[j] - M - kappa_n)  =  alpha_n(i) T_ij lhs_{n+1}(j) beta_{n+1}(j) / Z
// (the gathered y_{n+1}[j] = beta~_{n+1}[j] + e_{n+1}[j] is what the recursion reads anyway).  Every slot has exactly one owning
// lane, so the sums need no atomics and come out the same on every run:
//   register-resident items  float32 partial sums in registers, added to the float64 per-slot workspace every MM_ARC_FLUSH
//                            frames (a float32 sum of 32 terms in [0, 1] is good to ~2e-6 of itself)
//   streamed items           straight into the float64 per-slot workspace, every frame
// At n = 1 the kernel also leaves the state posteriors of frame 1 (the initial-state counts).  mm_arc_scatter_kernel then writes
// the counts in the caller's entry order, adds the phony self-loop's N - len_b frames, and writes ttl = log Z.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

#define MM_ARC_FLUSH 32  // frames between the flushes of the register partial sums

template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_arc_kernel(RunParams p, ArcParams ap) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *part = lds + L.part;
    float *psum = lds + L.total;  // [2][MM_MAX_WAVES] the waves' sums of the state posteriors of a frame (LDS behind the plan)
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    const GraphDev gb = u.g[1];
    double *acc = ap.acc + ap.arcs[b].slot_off;
    float *post1 = ap.post1 + u.s1p_prefix;
    const double logZ2 = wsC[0];
    if (!(logZ2 > -1e300) || len < 1) return;  // no accepting path, or no frame: mm_arc_scatter_kernel writes what is known

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    for (int s = tid; s < S1; s += NT) post1[s] = 0.f;  // (rows without arcs have no item)
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    copy_row(stage + (len & 1) * S1p, wsA + (long long)len * S1p, S1p >> 2, tid, NT);
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
            float s = 0.f;  // (not part_sum: the waves' sums are added one after the other, and these are the bits the counts carry)
            for (int w = 0; w < NW; ++w) s += psum[((n + 1) & 1) * MM_MAX_WAVES + w];
            if (s > 0.f) corr += fast_log2(s);
        }
        // (alpha~ carries the rounding of every forward step: normalised by log Z alone, the posteriors of a frame drift off 1 --
        // 1e-4 after 500 frames of sharp emissions.  The frame n + 1 sum corrects frame n: what is left is one step's drift)
        const float kappa = (float)(logZ2 - Cn - D + (double)corr);
        const float sh = -M - kappa;  // arc term of slot k of row i: 2^(alpha~_n[i] + sh + x_k), x_k = w_k + y_{n+1}[col_k]
        if (n - 1 >= 1) {  // frame n-1 into the buffers frame n+1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            stage_row<BIGV>(stage + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        float wm = MM_NINF, qs = 0.f;
        // the leader lane of a row group: beta~_n, y_n = beta~_n + e_n, the state posterior (summed; kept at frame 1)
        auto epi = [&](float v, int row, float e) {
            const float beta = v - M;
            const float q = fast_exp2(ast[row] + beta - kappa);
            qs += q;
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
                facc[i][0] += fast_exp2(x0 + base);
                facc[i][1] += fast_exp2(x1 + base);
                if (R > 2) {
                    facc[i][2] += fast_exp2(x2 + base);
                    facc[i][3] += fast_exp2(x3 + base);
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
            const float base = r.row >= 0 ? ast[r.row] + sh : MM_NINF;
            const Slot *sp = gb.slots + (size_t)im.slot_row * 64 + lane;
            double *dp = acc + (size_t)im.slot_row * 64 + lane;
            for (int k = 0; k < im.R; ++k) {
                const Slot s = load_slot(sp + k * 64);
                const double t = (double)fast_exp2(s.w + yp[s.col] + base);
                dp[k * 64] = (n == len ? 0.0 : dp[k * 64]) + t;
            }
            if (r.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) epi(v, r.row, e);
        }
        if constexpr (NI > 0) {
            if ((len - n) % MM_ARC_FLUSH == MM_ARC_FLUSH - 1 || n == 1) {  // the register partial sums into the workspace
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
        stage_row_wait<BIGV>();  // this wave's part of alpha~ of frame n - 1 is in LDS
        vsync();
    }
}

// counts in the caller's entry order, initial-state counts, ttl.  grid (B, blocks), block 256.
__global__ void __launch_bounds__(256) mm_arc_scatter_kernel(RunParams p, ArcParams ap) {
    const int b = blockIdx.x;
    const UttDesc &u = p.utts[b];
    const ArcDev ad = ap.arcs[b];
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const double logZ2 = p.ws_c[(long long)b * (p.N + 2)];
    const bool ok = logZ2 > -1e300;
    const double *acc = ap.acc + ad.slot_off;
    const int t0 = blockIdx.y * blockDim.x + threadIdx.x, ts = gridDim.y * blockDim.x;
    float *cb = ap.counts + (long long)b * ap.csb;
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
    if (ap.init_counts) {
        // frame 1's posteriors over their sum (the block's threads add them in a fixed order: the same bits on every run)
        __shared__ float red[256];
        float s1 = 0.f;
        if (ok && len >= 1)
            for (int s = threadIdx.x; s < u.S1; s += blockDim.x) s1 += ap.post1[u.s1p_prefix + s];
        red[threadIdx.x] = s1;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        const float inv = red[0] > 0.f ? 1.f / red[0] : 0.f;
        float *ib = ap.init_counts + (long long)b * ap.isb;
        for (int m = t0; m < ad.n_init; m += ts) {
            const int s = ad.init_states[m];
            float c = 0.f;
            if (ok) c = len >= 1 ? ap.post1[u.s1p_prefix + s] * inv : (s == u.S1 - 1 ? 1.f : 0.f);
            ib[m] = c;
        }
    }
    if (ap.ttl && t0 == 0) ap.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
}

}  // namespace mm
