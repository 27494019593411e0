// mm_item_parts.hip -- the parts the kernels of the item-form entries share (arcs, sample, cost, leaky, entropy, filter, window,
// segment, vitwindow): one definition each, included by those kernel files only.  Every part is what the kernels had
// written out, operation for operation: moving a kernel onto a part changes none of its results.  A kernel whose version of a
// part truly differs keeps its own code, with a comment saying why; no part takes a flag to cover such a case.
#pragma once
#include "mm_internal.h"
#include "mm_kernels.hip"

namespace mm {

// barrier of a workgroup whose vectors may live in global memory (FENCED): the stores before it are visible behind it
template <bool FENCED>
__device__ __forceinline__ void item_vsync() {
    if constexpr (FENCED) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if constexpr (FENCED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// The lines every kernel shares: one utterance per workgroup (RunParams p in scope), its sizes, its clamped length, the barrier,
// its emissions and its rows of the workspace.  The LDS plan and every further pointer stay with the kernel, below the macro.
#define MM_ITEM_PROLOGUE(FENCED)                                                                                  \
    const int b = blockIdx.x;                                                                                     \
    const UttDesc &u = p.utts[b];                                                                                 \
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;                                                \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = NT >> 6;                                      \
    [[maybe_unused]] const int S1 = u.S1, S1p = u.S1p, P1 = u.P1, P = P1 - 1, P1p = (P1 + 3) & ~3;                \
    [[maybe_unused]] const int fstate = S1 - 1;                                                                   \
    int len = p.lens ? p.lens[b] : p.N;                                                                           \
    len = len < 0 ? 0 : (len > p.N ? p.N : len);                                                                  \
    [[maybe_unused]] const int NF = len + 1;                                                                      \
    [[maybe_unused]] auto vsync = []() { item_vsync<FENCED>(); };                                                 \
    [[maybe_unused]] const float *Vb = p.V + (long long)b * p.vsb;                                                \
    [[maybe_unused]] float *wsA = p.ws_alpha + u.s1p_prefix * (long long)(p.N + 1);                               \
    [[maybe_unused]] double *wsC = p.ws_c + (long long)b * (p.N + 2)

// one row of n4 float4 from src to dst by all threads (coalesced): a row between the workspace and the vectors
__device__ __forceinline__ void copy_row(float *dst, const float *src, int n4, int tid, int NT) {
    const float4 *s = reinterpret_cast<const float4 *>(src);
    float4 *d = reinterpret_cast<float4 *>(dst);
    for (int q = tid; q < n4; q += NT) d[q] = s[q];
}
// one row of the workspace on its way to the stage rows while a frame is computed: by DMA into LDS (every wave its part; in LDS
// behind stage_row_wait and the barrier), BIGV: into the global vectors
template <bool BIGV>
__device__ __forceinline__ void stage_row(float *dst, const float *src, int n4, int tid, int NT, int wave, int lane) {
    if constexpr (BIGV) {
        copy_row(dst, src, n4, tid, NT);
    } else {
        const float4 *s = reinterpret_cast<const float4 *>(src);
        const unsigned d = lds_addr_of(dst);
        for (int q0 = wave * 64; q0 < n4; q0 += NT)
            if (q0 + lane < n4) dma_b128(s + q0 + lane, d + 16u * (unsigned)q0);
    }
}
// two rows on one walk, for the kernels that carry a second row beside alpha~ (two calls of stage_row cost their global-vector
// instances registers and a wave of occupancy)
__device__ __forceinline__ void copy_row_pair(float *dst0, const float *src0, float *dst1, const float *src1, int n4, int tid, int NT) {
    const float4 *s0 = reinterpret_cast<const float4 *>(src0), *s1 = reinterpret_cast<const float4 *>(src1);
    float4 *d0 = reinterpret_cast<float4 *>(dst0), *d1 = reinterpret_cast<float4 *>(dst1);
    for (int q = tid; q < n4; q += NT) {
        d0[q] = s0[q];
        d1[q] = s1[q];
    }
}
template <bool BIGV>
__device__ __forceinline__ void stage_row_pair(float *dst0, const float *src0, float *dst1, const float *src1, int n4, int tid, int NT, int wave,
                                               int lane) {
    if constexpr (BIGV) {
        copy_row_pair(dst0, src0, dst1, src1, n4, tid, NT);
    } else {
        const float4 *s0 = reinterpret_cast<const float4 *>(src0), *s1 = reinterpret_cast<const float4 *>(src1);
        const unsigned d0 = lds_addr_of(dst0), d1 = lds_addr_of(dst1);
        for (int q0 = wave * 64; q0 < n4; q0 += NT)
            if (q0 + lane < n4) {
                dma_b128(s0 + q0 + lane, d0 + 16u * (unsigned)q0);
                dma_b128(s1 + q0 + lane, d1 + 16u * (unsigned)q0);
            }
    }
}
// this wave's part of the rows stage_row brought is in LDS
template <bool BIGV>
__device__ __forceinline__ void stage_row_wait() {
    if constexpr (!BIGV) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// a frame's emissions as a kernel without the log2 scaling stages them: natural log (stage_em with scale 1)
__device__ __forceinline__ float em_value_nat(float raw, int n, int len, int P, int q) {
    if (q < P) return (n <= len) ? raw : MM_NINF;
    return (n <= len) ? MM_NINF : 0.f;
}
// the emissions of frame f one frame ahead: `raw` travelled in a register (em_load_raw), VALUE (em_value with scale MM_LOG2E,
// em_value_nat with scale 1) makes the staged entry of it; the pdfs beyond the block's threads are staged from memory
template <float (*VALUE)(float, int, int, int, int)>
__device__ __forceinline__ void stage_em_ahead(float *dst, float raw, const float *Vb, long long vsn, int f, int len, int P, int tid, int NT,
                                               float scale) {
    if (tid <= P) dst[tid] = VALUE(raw, f, len, P, tid);
    if (P >= NT) stage_em(dst + NT, Vb + NT, vsn, f, len, P - NT, tid, NT, scale);
}

// the sum of the waves' partial sums (lane < NW <= 16) in a fixed order, the same bits in every wave
__device__ __forceinline__ float part_sum(const float *ps, int NW, int lane) {
    float v = (lane < NW) ? ps[lane] : 0.f;
    v = grp_sum(v, 4);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// the largest emission of the real pdfs of a staged frame (0 for a frame without one), the same bits in every wave
__device__ __forceinline__ float frame_emax(const float *emn, int P, int lane) {
    float m = MM_NINF;
    for (int q = lane; q < P; q += 64) m = fmaxf(m, emn[q]);
    m = wave_max_rl(m);
    return (m > MM_NINF) ? m : 0.f;
}

// gamma of a frame (gp: its first element) from its per-pdf sums, over the sum of the first nsum of them: the frame adds up to 1
// whatever the rounding of the recursions left; a frame without mass gives zeros.  One wave.
__device__ __forceinline__ void finalise_gamma(const float *bf, int nsum, int P, int lane, float *gp, long long gsp) {
    float s = 0.f;
    for (int q = lane; q < nsum; q += 64) s += bf[q];
    s = wave_sum(s);
    const float inv = s > 0.f ? 1.f / s : 0.f;
    for (int q = lane; q < P; q += 64) gp[q * gsp] = bf[q] * inv;
}
// exact zeros on the frames from `from` (0-based) on of an utterance's output g (strides gsn, gsp)
__device__ __forceinline__ void zero_gamma_from(float *g, long long gsn, long long gsp, int from, int N, int P, int tid, int NT) {
    for (long long q = tid; q < (long long)(N - from) * P; q += NT) g[(from + q / P) * gsn + (q % P) * gsp] = 0.f;
}

// The pass over the pdf -> states lists (every state is in one list; the phony pdf's holds the final state): 8 lanes per pdf walk
// the pdf's states in pdf_rows in a fixed order, a 3-step DPP reduction ends it -- no atomics, the same bits on every run.
// c = per_pdf(pdf) once per pdf, per_row(row, c, acc) for each of its states adds to the NS sums acc; sum i of pdf goes to
// bn[i][pdf].  npdf: P1, or P where the phony pdf is left out.
template <int NS, class Pdf, class Row>
__device__ __forceinline__ void for_pdf_rows(const UttDesc &u, int npdf, int wave, int NW, int lane, float *const (&bn)[NS], Pdf &&per_pdf,
                                             Row &&per_row) {
    for (int p0 = wave * 8; p0 < npdf; p0 += NW * 8) {
        const int pdf = p0 + (lane >> 3);
        float acc[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = 0.f;
        if (pdf < npdf) {
            const auto c = per_pdf(pdf);
            const int e0 = u.pdf_ptr[pdf], e1 = u.pdf_ptr[pdf + 1];
            for (int k = e0 + (lane & 7); k < e1; k += 8) per_row(u.pdf_rows[k], c, acc);
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = grp_sum(acc[i], 3);
        if (pdf < npdf && (lane & 7) == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) bn[i][pdf] = acc[i];
        }
    }
}

}  // namespace mm
