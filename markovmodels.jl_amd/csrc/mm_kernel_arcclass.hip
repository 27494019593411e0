// mm_kernel_arcclass.hip -- per-frame arc-class posteriors (Baum-Welch's xi_n summed over classes of arcs) on the item form.
// Included by mm_arcclass_tu.hip only.
//
// The forward half is mm_log_kernel<MODE_FB, NI, 1> as mm_launch_arcs runs it.  mm_arcclass_kernel then runs mm_arc_kernel's
// beta~ recursion over the backward (T_hat) item form -- the same normaliser M, the same kappa with the correction from the
// previous frame's posterior sum -- and at every frame n gives every CLASSIFIED entry k = (i -> j) its term
//     2^(alpha~_n[i] + w_ij + y_{n+1}[j] - M - kappa_n)  =  alpha_n(i) T_ij lhs_{n+1}(j) beta_{n+1}(j) / Z
// The classified entries of an utterance are ranked by (class, caller's entry index): class c owns the ranks
// [cptr[c], cptr[c + 1]).  Rank m has a record {row i, column j, weight} (ClassRec, in rank order) and one owning thread per
// frame (m = tid, tid + NT, ...), which stores the term at terms[n & 1][m]: no atomics, and nothing at all is done for an entry
// without a class -- the recursion does not know about classes.  (The records are read instead of the slots the recursion
// holds: one path for register-resident and streamed items and for the three instances, no rank registers -- DESIGN.md 4.28.)
// The class pass then sums each class's range with a fixed number of lanes in a fixed order and writes xi[b, c, n - 1].  The
// pass of frame n runs in iteration n - 1, behind the barrier that closes frame n, on the other half of the term row: it adds
// no barrier.  The term rows live in LDS behind the arc kernel's plan, or (ArcClassParams::terms_global) in the workspace: the
// barrier then carries the fences of the global vectors.  Frames t >= len, and every frame of an utterance without a path,
// are written by the kernel's first lines; it also writes ttl.
#pragma once
#include "mm_internal.h"
#include "mm_item_parts.hip"

namespace mm {

#define MM_CLASS_UNROLL 8  // records a thread of the term loop has in flight

// the sums of the classes of one frame: 1 << lgl lanes per class walk its ranks in a fixed order, a butterfly ends it
__device__ __forceinline__ void class_pass(const ClassDev &cd, const float *trow, float *xrow, long long xsc, int wave, int NW, int lane) {
    const int lgl = cd.lgl, per = 64 >> lgl, sub = lane & ((1 << lgl) - 1);
    for (int c0 = wave * per; c0 < cd.C; c0 += NW * per) {
        const int c = c0 + (lane >> lgl);
        float acc = 0.f;
        if (c < cd.C) {
            const int e1 = cd.cptr[c + 1], st = 1 << lgl;
            int m = cd.cptr[c] + sub;
            for (; m + 3 * st < e1; m += 4 * st) {  // (four loads in flight, added in the order of the plain loop: the same bits)
                const float t0 = trow[m], t1 = trow[m + st], t2 = trow[m + 2 * st], t3 = trow[m + 3 * st];
                acc += t0;
                acc += t1;
                acc += t2;
                acc += t3;
            }
            for (; m < e1; m += st) acc += trow[m];
        }
        acc = grp_sum_rt(acc, lgl);
        if (c < cd.C && sub == 0) xrow[c * xsc] = acc;
    }
}

template <int NI, bool BIGV>
__global__ void __launch_bounds__(512) mm_arcclass_kernel(RunParams p, ArcClassParams cp) {
    extern __shared__ float lds[];
    MM_ITEM_PROLOGUE(BIGV);
    const LdsPlan L = lds_plan(BIGV ? 0 : S1p, P1p, true);
    float *em = lds + L.em, *part = lds + L.part;
    float *psum = lds + L.total;  // [2][MM_MAX_WAVES] the waves' sums of the state posteriors of a frame (as mm_arc_kernel)
    float *buf = BIGV ? p.ws_big + (long long)b * p.big_stride : lds + L.buf;
    float *stage = BIGV ? buf + 2 * S1p : lds + L.stage;
    const GraphDev gb = u.g[1];
    const ClassDev cd = cp.cls[b];
    const bool tg = cp.terms_global != 0;
    float *terms = tg ? cp.terms + 2 * cd.term_off : psum + 2 * MM_MAX_WAVES;  // [2][cd.M]
    float *xb = cp.xi + (long long)b * cp.xsb;
    const double logZ2 = wsC[0];
    const bool ok = logZ2 > -1e300;
    if (cp.ttl && tid == 0) cp.ttl[b] = ok ? (float)(logZ2 * (double)MM_LN2) : MM_NINF;
    // frames beyond the utterance: only the phony self-loop is alive (no accepting path: nothing is)
    const int zfrom = ok ? len : 0;
    for (long long q = tid; q < (long long)(p.N - zfrom) * cd.C; q += NT) {
        const int c = (int)(q % cd.C);
        xb[(zfrom + q / cd.C) * cp.xsn + c * cp.xsc] = (ok && c == cd.cphony) ? 1.f : 0.f;
    }
    if (!ok || len < 1) return;

    for (int q = tid; q < 2 * S1p; q += NT) buf[q] = MM_NINF;
    vsync();
    if (tid == 0) buf[(NF & 1) * S1p + fstate] = 0.f;
    stage_em(em + (len & 1) * P1p, Vb, p.vsn, len, len, P, tid, NT, MM_LOG2E);
    copy_row(stage + (len & 1) * S1p, wsA + (long long)len * S1p, S1p >> 2, tid, NT);
    vsync();
    ItemRegs<NI> rg;
    load_item_regs<NI>(rg, gb, wave, NW, lane);
    double D = 0.0;
    const int n4 = S1p >> 2;
    float evp = 0.f;
    double Cn = wsC[len], Cpre = 0.0;
    auto prefetch = [&](int f) {  // frame f >= 1: emissions and C_f one step ahead
        evp = em_load_raw(Vb, p.vsn, f, p.N, P, tid);
        Cpre = wsC[f];
    };
    if (len >= 2) prefetch(len - 1);
    float corr = 0.f;  // log2 of the state posteriors' sum of frame n + 1 (1 in exact arithmetic)
    for (int n = len; n >= 1; --n) {
        const float *yp = buf + ((n + 1) & 1) * S1p;
        float *yn = buf + (n & 1) * S1p;
        const float *ast = stage + (n & 1) * S1p;  // alpha~ of frame n
        const float *emn = em + (n & 1) * P1p;
        const float M = (n == len) ? 0.f : part_max_dpp(part + ((n + 1) & 1) * MM_MAX_WAVES, NW, lane);
        D += (double)M;
        if (n < len) {
            float s = 0.f;  // (the waves' sums one after the other, as mm_arc_kernel adds them)
            for (int w = 0; w < NW; ++w) s += psum[((n + 1) & 1) * MM_MAX_WAVES + w];
            if (s > 0.f) corr += fast_log2(s);
        }
        const float kappa = (float)(logZ2 - Cn - D + (double)corr);
        const float sh = -M - kappa;
        if (n - 1 >= 1) {  // frame n-1 into the buffers frame n+1 has left (as mm_log_kernel's PASS 2)
            stage_em_ahead<em_value>(em + ((n - 1) & 1) * P1p, evp, Vb, p.vsn, n - 1, len, P, tid, NT, MM_LOG2E);
            stage_row<BIGV>(stage + ((n - 1) & 1) * S1p, wsA + (long long)(n - 1) * S1p, n4, tid, NT, wave, lane);
            Cn = Cpre;
            if (n - 2 >= 1) prefetch(n - 2);
        }
        // the classes of frame n + 1, from the half of the term row that frame's barrier closed
        if (n < len) class_pass(cd, terms + ((n + 1) & 1) * cd.M, xb + (long long)n * cp.xsn, cp.xsc, wave, NW, lane);
        // the terms of frame n: rank m by thread m mod NT
        // (MM_CLASS_UNROLL records in flight per thread: one at a time, a thread of a plan with every entry classified waits out
        // an L2 round trip per record)
        float *__restrict__ tn = terms + (n & 1) * cd.M;
        const ClassRec *__restrict__ recs = cd.recs;
        int m = tid;
        for (; m + (MM_CLASS_UNROLL - 1) * NT < cd.M; m += MM_CLASS_UNROLL * NT) {
            ClassRec r[MM_CLASS_UNROLL];
#pragma unroll
            for (int q = 0; q < MM_CLASS_UNROLL; ++q) r[q] = recs[m + q * NT];
#pragma unroll
            for (int q = 0; q < MM_CLASS_UNROLL; ++q) tn[m + q * NT] = fast_exp2(r[q].w + yp[r[q].col] + (ast[r[q].row] + sh));
        }
        for (; m < cd.M; m += NT) {
            const ClassRec r = recs[m];
            tn[m] = fast_exp2(r.w + yp[r.col] + (ast[r.row] + sh));
        }
        // the beta~ recursion; the leader lane of a row group: beta~_n, y_n = beta~_n + e_n, the state posterior (summed)
        float wm = MM_NINF, qs = 0.f;
        for_items<NI>(rg, gb, wave, NW, lane, yp, emn, [&](float v, int row, int, float e) {
            const float beta = v - M;
            qs += fast_exp2(ast[row] + beta - kappa);
            const float y = beta + e;
            yn[row] = y;
            wm = max_nc(wm, y);
        });
        part_put(part + (n & 1) * MM_MAX_WAVES, wave, lane, wm);
        qs = wave_sum(qs);
        if (lane == 0) psum[(n & 1) * MM_MAX_WAVES + wave] = qs;
        stage_row_wait<BIGV>();  // this wave's part of alpha~ of frame n - 1 is in LDS
        if constexpr (!BIGV) {  // (BIGV: vsync carries the fences)
            if (tg) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        vsync();
        if constexpr (!BIGV) {
            if (tg) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    class_pass(cd, terms + cd.M, xb, cp.xsc, wave, NW, lane);  // frame 1
}

}  // namespace mm
