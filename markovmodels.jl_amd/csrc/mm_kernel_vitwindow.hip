// mm_kernel_vitwindow.hip -- windowed best paths (mm_viterbiwindow_f32: the Viterbi recursion of a tropical batch over a WINDOW of the
// audio -- it starts from a carried vector instead of the FSM's initial one and ends open, on the best real state, or in the phony
// final state) on the item form.  Included by mm_vitwindow_tu.hip only.
//
// mm_vitwindow_fwd_kernel    mm_tropical_kernel's step (float adds and a max, nothing else) from the carried start vector.  What
//                            leaves for the workspace, per frame: the back-pointer row (whole and coalesced, one frame late), the
//                            row of PRE-EMISSION maxima `best` of the step (state_out of a commit frame the second kernel only
//                            learns later is best_{c+1} - m_c: the step has the value in a register, so it is one store per row and
//                            no arc pass in the second kernel; storing the d rows instead would cost the same workspace and a
//                            second copy of the item walk) and m_n, the frame's maximum over the real states (the waves' maxima
//                            ride on the step's barrier, wave 0 gathers them a step later).  Behind the loop: the window's end.
//                            Open: the (max, lowest arg) of d_len over the real states and the flags d_len(i) > -inf.  Closed:
//                            d_{len+1}(f) and bp_{len+1}(f) as mm_tropical_kernel leaves them, and one walk over the BACKWARD
//                            item form from the unit vector of f: T_hat(i, f), hence the flags d_len(i) + T_hat(i, f) > -inf.
// mm_vitwindow_trace_kernel  walks back from frame len.  The surviving set A_n lives in two byte vectors of LDS (beyond the LDS: of
//                            global memory): a thread owns the states tid, tid + NT, ...; per frame it counts and clears its
//                            flagged states of A_n and flags their back-pointers in the other vector (several threads may store
//                            the same 1 to a byte: a benign race), the waves' counts ride on the frame's ONE barrier.  The first
//                            frame with one survivor is `converged` (a singleton maps to a singleton: the set work ends there).
//                            One lane then follows the path, and the workgroup writes state_out at the commit frame.
// No atomics: the same bits on every run.  (Registers: the forward instance <8,global> spills one VGPR, 8 bytes of scratch per lane,
// under its 1024-thread bound; the others none.)
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

// LDS of the forward kernel, in floats: the tropical kernel's plan (the stage rows hold the back-pointers) and, behind it, the
// waves' (max, arg) of the open end -- MM_ARC_LDS_EXTRA bytes, the arc kernel's size: a batch whose vectors are global for this
// entry has the global vectors mm_batch_create allocates.
__host__ __device__ inline int vitwindow_lds_floats(int S1p, int P1p) { return lds_plan(S1p, P1p, true).total + 2 * MM_MAX_WAVES; }
// LDS of the trace kernel, in bytes: two flag vectors of S1p bytes (flags_global: none)
__host__ __device__ inline size_t vitwindow_trace_lds_bytes(int S1p, bool flags_global) { return flags_global ? 0 : 2 * size_t(S1p); }

// forward: rows 1..len of the back-pointers (row r: frame r + 1) and of `best` (row r: step r + 1), row 0 of the back-pointers: the
// flags of A_len; m_1..m_len, the end state and the score.  grid = B workgroups (one utterance each), block = 64 * NW threads.
template <int NI, bool BIGV>
__global__ void __launch_bounds__(1024) mm_vitwindow_fwd_kernel(RunParams p, VitWindowParams wp) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);  // (the prologue alone: the recursion is tropical, its parts are mm_tropical_kernel's)
    const bool closed = wp.closed ? __builtin_amdgcn_readfirstlane(wp.closed[b]) != 0 : false;
    const long long wsrow = u.s1p_prefix * (long long)(p.N + 1);
    int *wsBP = wp.ws_bp + wsrow;
    float *wsBest = wp.ws_best + wsrow;
    float *wsM = wp.ws_m + (long long)b * (p.N + 2);
    if (len == 0) {  // no frame: no path (the trace kernel passes the start vector through)
        if (tid == 0) {
            p.score[b] = MM_NINF;
            wp.ws_end[b] = -1;
        }
        return;
    }
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *part = lds + L.part;
    float *rbest = lds + L.total;
    int *rarg = reinterpret_cast<int *>(lds + L.total + MM_MAX_WAVES);
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;  // (BIGV: see mm_log_kernel)
    int *bpbuf = reinterpret_cast<int *>(BIGV ? buf + 2 * S1p : lds + L.stage);  // [2][S1p]
    const float *sin = wp.state_in ? wp.state_in + u.state_off : nullptr;
    const GraphDev gf = u.g[0];
    ItemRegs<NI> rg;

    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, 1.0f);
    for (int q = tid; q < 2 * S1p; q += NT) {
        buf[q] = MM_NINF;
        bpbuf[q] = -1;
    }
    vsync();
    {   // frame 1: start (+) lhs[:,1]; the phony final state starts empty.  (state_in is read here alone: the trace kernel writes
        // state_out)
        float *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        float wm = MM_NINF;
        for (int s = tid; s < S1; s += NT) {
            const float st = s < fstate ? (sin ? sin[s] : u.init[s]) : MM_NINF;
            const float v = st + e1[u.s2p[s]];
            a1[s] = v;
            if (s < fstate) wm = fmaxf(wm, v);
        }
        wm = wave_max(wm);
        if (lane == 0) part[1 * MM_MAX_WAVES + wave] = wm;
        stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, 1.0f);
    }
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    vsync();
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        int *bpn = bpbuf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        float *bestn = wsBest + (long long)(n - 1) * S1p;
        // emissions of frame n+1: raw load now (every thread, clamped address: nothing waits on it), stored to LDS at the end of the step
        float evraw;
        {
            const int nn = n + 1 > p.N ? p.N : n + 1, qq = tid < P ? tid : P - 1;
            evraw = Vb[(long long)(nn - 1) * p.vsn + qq];
        }
        if (wave == 0) {  // m_{n-1}: the waves' maxima the last barrier made visible (-inf stays -inf)
            float v = (lane < NW) ? part[((n - 1) & 1) * MM_MAX_WAVES + lane] : MM_NINF;
            v = row16_max(v);
            if (lane == 0) wsM[n - 1] = v;
        }
        if (n > 2) {  // back-pointers of frame n-1 (row n-2): whole row, coalesced
            const int4 *src = reinterpret_cast<const int4 *>(bpbuf + ((n - 1) & 1) * S1p);
            int4 *dst = reinterpret_cast<int4 *>(wsBP + (long long)(n - 2) * S1p);
            for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
        }
        float wm = MM_NINF;
        auto finish = [&](float best, int arg, int row, int pdf) {
            const float v = best + emn[pdf];
            an[row] = v;
            bpn[row] = arg;
            bestn[row] = best;
            if (row != fstate) wm = fmaxf(wm, v);
        };
        static_for<0, NI>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const int meta = rg.meta[i];
            if (meta != 0) {
                const int R = meta & 0xff, lg = meta >> 8;
                float best = MM_NINF;
                int arg = -1;
                const int c0 = rg.c[i][0] & 0xffffu, c1 = rg.c[i][0] >> 16;
                trop_better(best, arg, rg.w[i][0] + ap[c0], c0);
                trop_better(best, arg, rg.w[i][1] + ap[c1], c1);
                if (R > 2) {
                    const int c2 = rg.c[i][1] & 0xffffu, c3 = rg.c[i][1] >> 16;
                    trop_better(best, arg, rg.w[i][2] + ap[c2], c2);
                    trop_better(best, arg, rg.w[i][3] + ap[c3], c3);
                }
                trop_grp_reduce(best, arg, lg);
                const unsigned row = rg.ri[i] & 0xffffu;
                if (row != 0xffffu && (lane & ((1 << lg) - 1)) == 0) finish(best, arg, (int)row, (int)(rg.ri[i] >> 16));
            }
        });
        const int resident = NI * NW < gf.n_short ? NI * NW : gf.n_short;  // (known without touching memory)
        for (int it = wave; it < gf.n_items; it += NW) {
            if (it < resident) continue;
            const ItemMeta im = load_item(gf.items, it);
            const RowInfo ri = gf.rowinfo[(size_t)it * 64 + lane];
            const Slot *sp = gf.slots + (size_t)im.slot_row * 64 + lane;
            float best = MM_NINF;
            int arg = -1;
            for (int k = 0; k < im.R; ++k) {
                Slot s = load_slot(sp + k * 64);
                trop_better(best, arg, s.w + ap[s.col], (int)s.col);
            }
            trop_grp_reduce(best, arg, im.log2g);
            if (ri.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) finish(best, arg, ri.row, ri.pdf);
        }
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        if (n + 1 <= NF) {
            if (tid <= P) {
                float *dst = em + ((n + 1) & 1) * P1p;
                if (tid < P) dst[tid] = (n + 1 <= len) ? evraw : MM_NINF;
                else dst[tid] = (n + 1 <= len) ? MM_NINF : 0.f;
            }
            if (P >= NT) stage_em(em + ((n + 1) & 1) * P1p + NT, Vb + NT, p.vsn, n + 1, len, P - NT, tid, NT, 1.0f);
        }
        vsync();
    }
    {   // back-pointers of frame len + 1 (row len)
        const int4 *src = reinterpret_cast<const int4 *>(bpbuf + (NF & 1) * S1p);
        int4 *dst = reinterpret_cast<int4 *>(wsBP + (long long)len * S1p);
        for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
    }
    const float *dl = buf + (len & 1) * S1p;  // d_len
    int *flags = bpbuf + (len & 1) * S1p;     // (the row of frame len: it left at the last step, or is frame 1's and never leaves)
    if (closed) {
        // the path ends in the phony final state at frame len + 1, as mm_tropical_kernel's; T_hat(i, f) by the backward item form
        float *y = buf + (NF & 1) * S1p;
        const float sc = y[fstate];
        const int e_end = bpbuf[(NF & 1) * S1p + fstate];
        vsync();  // (everyone has read y and copied the last row)
        for (int q = tid; q < S1p; q += NT) {
            y[q] = q == fstate ? 0.f : MM_NINF;
            flags[q] = 0;
        }
        const GraphDev gb = u.g[1];
        load_item_regs<NI>(rg, gb, wave, NW, lane);
        vsync();
        for_items<NI, true>(rg, gb, wave, NW, lane, y, em, [&](float v, int row, int, float) {
            if (row != fstate && dl[row] + v > MM_NINF) flags[row] = 1;
        });
        if (tid == 0) {
            p.score[b] = sc;
            wp.ws_end[b] = sc > MM_NINF ? e_end : -1;
        }
    } else {
        // the audio goes on: the best real state of frame len, the lowest among equals
        float best = MM_NINF;
        int arg = -1;
        for (int s = tid; s < S1p; s += NT) {
            const bool real = s < fstate;
            if (real) trop_better(best, arg, dl[s], s);
            flags[s] = real && dl[s] > MM_NINF ? 1 : 0;
        }
        trop_grp_reduce(best, arg, 6);
        if (lane == 0) {
            rbest[wave] = best;
            rarg[wave] = arg;
        }
        __syncthreads();
        if (tid == 0) {
            best = MM_NINF;
            arg = -1;
            for (int w = 0; w < NW; ++w) trop_better(best, arg, rbest[w], rarg[w]);
            p.score[b] = best;
            wp.ws_end[b] = best > MM_NINF ? arg : -1;
        }
    }
    vsync();
    {   // the flags of A_len: row 0
        const int4 *src = reinterpret_cast<const int4 *>(flags);
        int4 *dst = reinterpret_cast<int4 *>(wsBP);
        for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
    }
}

// trace: path, converged, state_out, mcommit, ncommit.  grid = B workgroups, block = 256 threads.  GF: the flags in the global
// vectors of the utterance (FSMs whose two byte vectors do not fit the LDS), else in LDS.
template <bool GF>
__global__ void __launch_bounds__(256) mm_vitwindow_trace_kernel(RunParams p, VitWindowParams wp) {
    extern __shared__ float lds[];
    __shared__ int cnt[2][4];
    MM_ITEM_PROLOGUE(GF);
    const long long wsrow = u.s1p_prefix * (long long)(p.N + 1);
    int *wsBP = wp.ws_bp + wsrow;
    float *wsBest = wp.ws_best + wsrow;
    float *wsM = wp.ws_m + (long long)b * (p.N + 2);
    int *path = p.path + (long long)b * p.path_stride_b;
    for (int n = len + tid; n < p.N; n += NT) path[n] = -1;
    const bool ok = p.score[b] > MM_NINF;  // (the forward kernel's: -inf for a window without a frame or without a path)
    int conv = 0;
    if (ok) {
        unsigned char *fa = GF ? reinterpret_cast<unsigned char *>(p.ws_big + (long long)b * p.big_stride) : reinterpret_cast<unsigned char *>(lds);
        unsigned char *fb = fa + S1p;
        for (int j = tid; j < S1p; j += NT) {
            fa[j] = wsBP[j] != 0;
            fb[j] = 0;
        }
        vsync();
        for (int n = len; n >= 1; --n) {
            // A_n in fa: counted and cleared by its owners, A_{n-1} flagged in fb (clean since its owners cleared it a frame ago)
            const int *bpr = wsBP + (long long)(n - 1) * S1p;  // back-pointers of frame n (n >= 2)
            int c = 0;
            for (int j = tid; j < fstate; j += NT) {
                if (fa[j]) {
                    ++c;
                    fa[j] = 0;
                    if (n >= 2) {
                        const int i = bpr[j];
                        if ((unsigned)i < (unsigned)fstate) fb[i] = 1;
                    }
                }
            }
            c = (int)wave_sum((float)c);  // (a wave owns fewer than 2^24 states: exact)
            if (lane == 0) cnt[n & 1][wave] = c;
            vsync();
            int total = 0;
            for (int w = 0; w < NW; ++w) total += cnt[n & 1][w];
            if (total <= 1) {  // one survivor: every earlier frame has one too.  (none: not reached by a window with a path)
                conv = total == 1 ? n : 0;
                break;
            }
            unsigned char *t = fa;
            fa = fb;
            fb = t;
        }
    }
    if (tid == 0) {  // the best path: one lane follows the back-pointers from the end state
        int s = ok ? wp.ws_end[b] : -1;
        for (int n = len; n >= 1; --n) {
            path[n - 1] = s;
            if (n >= 2) s = (unsigned)s < (unsigned)S1 ? wsBP[(long long)(n - 1) * S1p + s] : -1;
        }
    }
    int c = wp.commit ? __builtin_amdgcn_readfirstlane(wp.commit[b]) : (wp.commit_converged ? 0 : len);
    c = c < 0 ? 0 : (c > len ? len : c);
    if (wp.commit_converged && conv > c) c = conv;
    const float mc = c >= 1 ? wsM[c] : 0.f;
    if (wp.state_out) {
        float *sout = wp.state_out + u.state_off;
        if (c == 0) {  // nothing is committed: the start vector passes through (NULL in: alpha_hat, the vector NULL stands for).
            // Every thread reads what it overwrites: state_in and state_out may be one buffer.
            const float *sin = wp.state_in ? wp.state_in + u.state_off : nullptr;
            for (int s = tid; s < S1; s += NT) sout[s] = sin ? sin[s] : u.init[s];
        } else {
            const float *bc = wsBest + (long long)c * S1p;  // best of step c + 1
            const bool alive = mc > MM_NINF;
            for (int s = tid; s < S1; s += NT) sout[s] = alive ? bc[s] - mc : MM_NINF;
        }
    }
    if (tid == 0) {
        if (wp.mcommit) wp.mcommit[b] = mc;
        if (wp.ncommit) wp.ncommit[b] = c;
        if (wp.converged) wp.converged[b] = conv;
    }
}

}  // namespace mm
