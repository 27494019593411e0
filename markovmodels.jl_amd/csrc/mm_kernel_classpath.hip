// mm_kernel_classpath.hip -- best paths that report arc classes, under per-frame arc-class scores (mm_classpath_f32: the Viterbi
// recursion of a tropical batch in which every arc adds its class's entry of the transition's score row, and which keeps, beside
// the source state, the CLASS of the arc that won every maximum) on the item form.  Included by mm_classpath_tu.hip only.
//
// mm_classpath_fwd_kernel    mm_vitwindow_fwd_kernel's step (float adds and a max, nothing else) from the FSM's own start vector to
//                            the phony final state.  MODE 0: that step as it stands (no plan: neither classes nor scores).  MODE 1:
//                            every arc carries its class id, and the maximiser is the lowest (source, class id) among the arcs of
//                            the greatest value -- the id C of an unclassified arc behind every class --: the triple (value, source,
//                            id) goes through the lane and the group reduction as the pair does in trop_grp_reduce, one more DPP
//                            move per level (NI = 0: the 70 000-state graph needs 17 + 16 bits beside the value); the instances with
//                            NI = 8 run on FSMs of at most 65 534 states only and carry (source, id) as one 32-bit key.
//                            MODE 2: and x = (w + d[source]) + urow[id], one add and then one more; slot [C] of the row holds 0, so
//                            no arc branches on its class.  MODE 1 forms no second add at all.
//                            The class ids: register-resident items keep their four in ScoreIds, streamed items read the plane
//                            beside their slots (mm_kernel_scored.hip).  The score row: C + 1 floats in LDS, double-buffered,
//                            UNSCALED (the tropical kernels stage emissions with factor 1), fetched one step ahead by
//                            score_load_raw / stage_score_ahead.  What leaves for the workspace, per frame: the back-pointer row
//                            and the 16-bit class row, whole and coalesced, one frame late.
// mm_classpath_trace_kernel  one lane per utterance follows the back-pointers from the phony final state and writes path and
//                            classes (both loads of a frame depend on the state alone); the rest of the workgroup writes the -1
//                            tails.
// No atomics: the same bits on every run.  -inf + -inf is the only sum of infinities: no NaN for finite or -inf inputs.
// Registers of the forward instances (the compiler's resource summary, gfx950, 1024-thread bound = 128 VGPRs; VGPRs / bytes of
// scratch per lane), <NI,lds> and <NI,global>:
//   MODE 0 (plain)             <8>: 114 / 0 and 128 / 8 (the one VGPR mm_vitwindow_fwd_kernel<8,global> spills)   <0>: 30 / 0, 32 / 0
//   MODE 1 (classes)           <8>: 123 / 0 and 123 / 0                                                           <0>: 37 / 0, 38 / 0
//   MODE 2 (classes + scores)  <8>: 128 / 20 and 128 / 16 (5 and 4 VGPRs spilled)                                 <0>: 71 / 0, 71 / 0
// The 16 id registers of <8> fit because the packed ids and state indices are made opaque once per frame (the asm below): left to
// itself the compiler unpacks and combines them ahead of the time loop, doubles their registers and spills 54 to 163 VGPRs.
// mm_classpath_trace_kernel: 6 VGPRs, no scratch.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"
#include "mm_kernel_scored.hip"  // ScoreIds, load_score_ids, score_load_raw, stage_score, stage_score_ahead

namespace mm {

// LDS of the forward kernel, in floats: the tropical kernel's plan (the stage rows hold the back-pointers) and, behind it, the two
// class rows (S1p 16-bit ids each); the two score rows come behind them (mm_scored_urow floats each).
__host__ __device__ inline int classpath_lds_floats(int S1p, int P1p) { return lds_plan(S1p, P1p, true).total + S1p; }

// trop_better with the class id as the last key: (greater value, lower source, lower id)
__device__ __forceinline__ void trop_better_cls(float &best, int &arg, int &cls, float v, int c, int k) {
    if (v > best || (v == best && v > MM_NINF && (c < arg || (c == arg && k < cls)))) {
        best = v;
        arg = c;
        cls = k;
    }
}
// trop_grp_reduce on the triple (the order is total: both partners of a butterfly step hold the same triple behind it)
__device__ __forceinline__ void trop_grp_reduce_cls(float &best, int &arg, int &cls, int log2g) {
    if (log2g == 0) return;
    if (log2g >= 1) trop_better_cls(best, arg, cls, dpp_mov<MM_DPP_XOR1>(best), dpp_mov_i<MM_DPP_XOR1>(arg), dpp_mov_i<MM_DPP_XOR1>(cls));
    if (log2g >= 2) trop_better_cls(best, arg, cls, dpp_mov<MM_DPP_XOR2>(best), dpp_mov_i<MM_DPP_XOR2>(arg), dpp_mov_i<MM_DPP_XOR2>(cls));
    if (log2g >= 3)
        trop_better_cls(best, arg, cls, dpp_mov<MM_DPP_HALF_MIRROR>(best), dpp_mov_i<MM_DPP_HALF_MIRROR>(arg), dpp_mov_i<MM_DPP_HALF_MIRROR>(cls));
    if (log2g >= 4) trop_better_cls(best, arg, cls, dpp_mov<MM_DPP_MIRROR>(best), dpp_mov_i<MM_DPP_MIRROR>(arg), dpp_mov_i<MM_DPP_MIRROR>(cls));
    if (log2g >= 5) trop_better_cls(best, arg, cls, __shfl_xor(best, 16), __shfl_xor(arg, 16), __shfl_xor(cls, 16));
    if (log2g >= 6) trop_better_cls(best, arg, cls, __shfl_xor(best, 32), __shfl_xor(arg, 32), __shfl_xor(cls, 32));
}

// ... and for the instances whose state indices fit 16 bits (NI = 8: every FSM of the batch has at most 65534 states): the pair
// (source, id) as ONE key source << 16 | id, compared unsigned -- the same order, a register and a DPP move per level less.
// 0xffffffff: no maximiser yet.
__device__ __forceinline__ void trop_better_key(float &best, unsigned &key, float v, unsigned k) {
    if (v > best || (v == best && v > MM_NINF && k < key)) {
        best = v;
        key = k;
    }
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_mov_u(unsigned v) { return (unsigned)dpp_mov_i<CTRL>((int)v); }
__device__ __forceinline__ void trop_grp_reduce_key(float &best, unsigned &key, int log2g) {
    if (log2g == 0) return;
    if (log2g >= 1) trop_better_key(best, key, dpp_mov<MM_DPP_XOR1>(best), dpp_mov_u<MM_DPP_XOR1>(key));
    if (log2g >= 2) trop_better_key(best, key, dpp_mov<MM_DPP_XOR2>(best), dpp_mov_u<MM_DPP_XOR2>(key));
    if (log2g >= 3) trop_better_key(best, key, dpp_mov<MM_DPP_HALF_MIRROR>(best), dpp_mov_u<MM_DPP_HALF_MIRROR>(key));
    if (log2g >= 4) trop_better_key(best, key, dpp_mov<MM_DPP_MIRROR>(best), dpp_mov_u<MM_DPP_MIRROR>(key));
    if (log2g >= 5) trop_better_key(best, key, __shfl_xor(best, 16), (unsigned)__shfl_xor((int)key, 16));
    if (log2g >= 6) trop_better_key(best, key, __shfl_xor(best, 32), (unsigned)__shfl_xor((int)key, 32));
}

// forward: rows 1..len of the back-pointers and of the classes (row r: frame r + 1) and the score.  grid = B workgroups (one
// utterance each), block = 64 * NW threads.
template <int NI, bool BIGV, int MODE>
__global__ void __launch_bounds__(1024) mm_classpath_fwd_kernel(RunParams p, ClassPathParams cp) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);
    constexpr bool CLS = MODE >= 1, SC = MODE == 2;
    constexpr bool KEY = CLS && NI == 8;  // (16-bit state indices: source and id travel as one key)
    const long long wsrow = u.s1p_prefix * (long long)(p.N + 1);
    int *wsBP = cp.ws_bp + wsrow;
    unsigned short *wsBC = cp.ws_bc + wsrow;
    if (len == 0) {  // no frame: no path
        if (tid == 0) p.score[b] = MM_NINF;
        return;
    }
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em;
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;   // (BIGV: see mm_log_kernel)
    int *bpbuf = reinterpret_cast<int *>(BIGV ? buf + 2 * S1p : lds + L.stage);  // [2][S1p]
    unsigned short *bcbuf = BIGV ? cp.ws_cbuf + (long long)b * cp.cbuf_stride : reinterpret_cast<unsigned short *>(lds + L.total);  // [2][S1p]
    float *ur = lds + classpath_lds_floats(BIGV ? 0 : S1p, P1p);  // [2][UR]
    const GraphDev gf = u.g[0];
    const unsigned short *plane = CLS ? cp.sc[b].plane[0] : nullptr;
    const int NC = cp.C, UR = cp.urow;
    const float *Ub = SC ? cp.U + (long long)b * cp.usb : nullptr;
    ItemRegs<NI> rg;
    ScoreIds<CLS ? NI : 0> si;

    stage_em(em + 1 * P1p, Vb, p.vsn, 1, len, P, tid, NT, 1.0f);
    for (int q = tid; q < 2 * S1p; q += NT) {
        buf[q] = MM_NINF;
        bpbuf[q] = -1;
        if constexpr (CLS) bcbuf[q] = (unsigned short)NC;
    }
    if constexpr (SC)
        for (int q = tid; q < 2 * UR; q += NT) ur[q] = 0.f;
    vsync();
    {   // frame 1: alpha_hat (+) lhs[:,1]; the phony final state starts empty
        float *a1 = buf + 1 * S1p;
        const float *e1 = em + 1 * P1p;
        for (int s = tid; s < S1; s += NT) a1[s] = (s < fstate ? u.init[s] : MM_NINF) + e1[u.s2p[s]];
        stage_em(em + 0 * P1p, Vb, p.vsn, 2, len, P, tid, NT, 1.0f);
        if constexpr (SC) stage_score(ur, Ub, cp.usn, cp.usc, 0, NC, tid, NT, 1.0f);  // transition 0 (step 2)
    }
    load_item_regs<NI>(rg, gf, wave, NW, lane);
    if constexpr (CLS) load_score_ids<NI>(si, gf, plane, NC, wave, NW, lane);
    float uvp = 0.f;
    if constexpr (SC) uvp = score_load_raw(Ub, cp.usn, cp.usc, 1, len - 1, NC, tid);
    vsync();
    for (int n = 2; n <= NF; ++n) {
        const float *ap = buf + ((n - 1) & 1) * S1p;
        float *an = buf + (n & 1) * S1p;
        int *bpn = bpbuf + (n & 1) * S1p;
        unsigned short *bcn = bcbuf + (n & 1) * S1p;
        const float *emn = em + (n & 1) * P1p;
        [[maybe_unused]] const float *urn = ur + (n & 1) * UR;  // transition n - 2
        // emissions of frame n+1: raw load now (every thread, clamped address: nothing waits on it), stored to LDS at the end of the step
        float evraw;
        {
            const int nn = n + 1 > p.N ? p.N : n + 1, qq = tid < P ? tid : P - 1;
            evraw = Vb[(long long)(nn - 1) * p.vsn + qq];
        }
        if constexpr (SC) {  // the scores of transition n - 1 (step n + 1) into the row step n - 1 has left, the next raw load
            if (n + 1 <= NF) stage_score_ahead(ur + ((n + 1) & 1) * UR, uvp, Ub, cp.usn, cp.usc, n - 1, NC, tid, NT, 1.0f);
            uvp = score_load_raw(Ub, cp.usn, cp.usc, n, len - 1, NC, tid);
        }
        if (n > 2) {  // back-pointers and classes of frame n-1 (row n-2): whole rows, coalesced
            const int4 *src = reinterpret_cast<const int4 *>(bpbuf + ((n - 1) & 1) * S1p);
            int4 *dst = reinterpret_cast<int4 *>(wsBP + (long long)(n - 2) * S1p);
            for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
            if constexpr (CLS) {
                const uint2 *csrc = reinterpret_cast<const uint2 *>(bcbuf + ((n - 1) & 1) * S1p);
                uint2 *cdst = reinterpret_cast<uint2 *>(wsBC + (long long)(n - 2) * S1p);
                for (int q = tid; q < (S1p >> 2); q += NT) cdst[q] = csrc[q];
            }
        }
        // (KEY: `arg` holds the key, `bk` nothing)
        auto arc = [&](float &best, int &arg, int &bk, float w, int c, unsigned id) {
            float x = w + ap[c];
            if constexpr (SC) x = x + urn[id];
            if constexpr (KEY) trop_better_key(best, reinterpret_cast<unsigned &>(arg), x, (unsigned)c << 16 | id);
            else if constexpr (CLS) trop_better_cls(best, arg, bk, x, c, (int)id);
            else trop_better(best, arg, x, c);
        };
        auto reduce = [&](float &best, int &arg, int &bk, int lg) {
            if constexpr (KEY) trop_grp_reduce_key(best, reinterpret_cast<unsigned &>(arg), lg);
            else if constexpr (CLS) trop_grp_reduce_cls(best, arg, bk, lg);
            else trop_grp_reduce(best, arg, lg);
        };
        auto finish = [&](float best, int arg, int bk, int row, int pdf) {
            an[row] = best + emn[pdf];
            if constexpr (KEY) {
                bpn[row] = arg == -1 ? -1 : (int)((unsigned)arg >> 16);
                bcn[row] = arg == -1 ? (unsigned short)NC : (unsigned short)((unsigned)arg & 0xffffu);
            } else {
                bpn[row] = arg;
                if constexpr (CLS) bcn[row] = (unsigned short)bk;
            }
        };
        static_for<0, NI>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const int meta = rg.meta[i];
            if (meta != 0) {
                const int R = meta & 0xff, lg = meta >> 8;
                float best = MM_NINF;
                int arg = -1, bk = NC;
                unsigned i01 = 0, i23 = 0, c01 = rg.c[i][0], c23 = rg.c[i][1];
                if constexpr (CLS) {
                    i01 = si.id[i][0];
                    i23 = si.id[i][1];
                    // (opaque per frame: unpacked or combined ahead of the time loop, the ids and indices of eight items would
                    // take twice their registers)
                    asm volatile("" : "+v"(i01), "+v"(i23), "+v"(c01), "+v"(c23));
                }
                const int c0 = c01 & 0xffffu, c1 = c01 >> 16;
                arc(best, arg, bk, rg.w[i][0], c0, i01 & 0xffffu);
                arc(best, arg, bk, rg.w[i][1], c1, i01 >> 16);
                if (R > 2) {
                    const int c2 = c23 & 0xffffu, c3 = c23 >> 16;
                    arc(best, arg, bk, rg.w[i][2], c2, i23 & 0xffffu);
                    arc(best, arg, bk, rg.w[i][3], c3, i23 >> 16);
                }
                reduce(best, arg, bk, lg);
                const unsigned row = rg.ri[i] & 0xffffu;
                if (row != 0xffffu && (lane & ((1 << lg) - 1)) == 0) finish(best, arg, bk, (int)row, (int)(rg.ri[i] >> 16));
            }
        });
        const int resident = NI * NW < gf.n_short ? NI * NW : gf.n_short;  // (known without touching memory)
        for (int it = wave; it < gf.n_items; it += NW) {
            if (it < resident) continue;
            const ItemMeta im = load_item(gf.items, it);
            const RowInfo ri = gf.rowinfo[(size_t)it * 64 + lane];
            const Slot *sp = gf.slots + (size_t)im.slot_row * 64 + lane;
            [[maybe_unused]] const unsigned short *ip = CLS ? plane + (size_t)im.slot_row * 64 + lane : nullptr;
            float best = MM_NINF;
            int arg = -1, bk = NC;
            for (int k = 0; k < im.R; ++k) {
                Slot s = load_slot(sp + k * 64);
                unsigned id = 0;
                if constexpr (CLS) id = ip[k * 64];
                arc(best, arg, bk, s.w, (int)s.col, id);
            }
            reduce(best, arg, bk, im.log2g);
            if (ri.row >= 0 && (lane & ((1 << im.log2g) - 1)) == 0) finish(best, arg, bk, ri.row, ri.pdf);
        }
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
    {   // back-pointers and classes of frame len + 1 (row len)
        const int4 *src = reinterpret_cast<const int4 *>(bpbuf + (NF & 1) * S1p);
        int4 *dst = reinterpret_cast<int4 *>(wsBP + (long long)len * S1p);
        for (int q = tid; q < (S1p >> 2); q += NT) dst[q] = src[q];
        if constexpr (CLS) {
            const uint2 *csrc = reinterpret_cast<const uint2 *>(bcbuf + (NF & 1) * S1p);
            uint2 *cdst = reinterpret_cast<uint2 *>(wsBC + (long long)len * S1p);
            for (int q = tid; q < (S1p >> 2); q += NT) cdst[q] = csrc[q];
        }
    }
    if (tid == 0) p.score[b] = buf[(NF & 1) * S1p + fstate];  // d_{len+1}(f)
}

// trace: path and classes.  grid = B workgroups, block = 256 threads.
__global__ void __launch_bounds__(256) mm_classpath_trace_kernel(RunParams p, ClassPathParams cp) {
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const UttDesc &u = p.utts[b];
    const int S1 = u.S1, S1p = u.S1p;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    const long long wsrow = u.s1p_prefix * (long long)(p.N + 1);
    const int *wsBP = cp.ws_bp + wsrow;
    const unsigned short *wsBC = cp.ws_bc + wsrow;
    int *path = p.path + (long long)b * p.path_stride_b;
    int *classes = cp.classes ? cp.classes + (long long)b * cp.csb : nullptr;
    if (tid == 0) {  // one lane follows the back-pointers from the phony final state of frame len + 1
        int s = p.score[b] > MM_NINF ? S1 - 1 : -1;  // (the forward kernel's: -inf without a frame or without a path)
        for (int n = len + 1; n >= 2; --n) {
            int i = -1, k = cp.C;
            if ((unsigned)s < (unsigned)S1) {
                const long long at = (long long)(n - 1) * S1p + s;  // frame n: row n - 1
                i = wsBP[at];
                if (classes) k = wsBC[at];
            }
            path[n - 2] = i;
            if (classes) classes[n - 2] = k < cp.C ? k : -1;
            s = i;
        }
    } else {
        for (int n = len + tid - 1; n < p.N; n += NT - 1) {
            path[n] = -1;
            if (classes) classes[n] = -1;
        }
    }
}

}  // namespace mm
