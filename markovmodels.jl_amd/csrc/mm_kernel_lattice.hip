// mm_kernel_lattice.hip -- beam-pruned best-path lattices (mm_lattice_f32: for every utterance b and transition t the stored entries
// of T_hat that lie on a complete path within beam_b of the best path, compacted in entry order).  Included by mm_lattice_tu.hip
// only.  The tropical alpha and beta rows come from the export kernels as they stand; what is here is the pass over the arcs.
//
// mm_lattice_prune_kernel<LDS, WRITE>  one workgroup of 256 threads per cell (b, t).  It stages the two rows the arcs of the cell read,
//                            a(i) = alpha_{t+1}(i) and c(j) = lhs_{t+2}(j) + beta_{t+2}(j), in LDS (LDS = true: 2 * S1p floats) or
//                            gathers them from global memory (LDS = false: FSMs beyond the LDS, and under MM_BIGV), and streams the
//                            three arc planes (source, destination, weight) of the utterance's FSM: a thread takes 4 consecutive
//                            entries per iteration, one dwordx4 load per plane (the planes are 256-byte aligned; the tail of a
//                            plane is read entry by entry), the next iteration's loads issued ahead of this one's decisions; the
//                            rows are staged four states per thread and turn, so that their loads overlap.  lat_keep decides every entry -- the SAME function in the count pass
//                            (WRITE = false) and the write pass (WRITE = true), so both decide identically.  Compaction in entry
//                            order: per wave one ballot per entry slot and its mbcnt (the kept entries of the lower lanes), across
//                            the four waves a scan of the wave counts in LDS (double-buffered: one barrier per iteration), across
//                            iterations a running base.  WRITE = false: counts[b, t] = the base at the end.  WRITE = true: record
//                            offs[b * N + t] + rank, if below cap, receives the entry's index and score.
// mm_lattice_scan_kernel     one workgroup of 256 threads: the exclusive scan of the B * N counts (row-major, read through the
//                            caller's stride) into int64 offsets, chunks of 1024 cells walked in order, 4 consecutive cells per
//                            thread; offs[B * N] and *total = the sum.
// No atomics anywhere: a repeated call returns the same bits.  Three float adds and one subtraction per entry, in the header's
// grouping; nothing that can contract.  -inf + -inf is the only sum of infinities for finite or -inf inputs; a NaN (an input of
// +inf) fails both comparisons of lat_keep and is dropped.
#pragma once
#include "mm_internal.h"
#include "mm_kernels.hip"

namespace mm {

#define MM_LAT_NT 256  // threads of a workgroup of both kernels
#define MM_LAT_E 4     // consecutive entries per thread and iteration
#define MM_LAT_HEAD 64 // bytes of dynamic LDS in front of the rows: the wave counts [2][4] (and the rows stay 16-byte aligned)

// the through-score of one entry and whether it stays: x = (a + w) + c, s = x - best; `live`: the utterance has a path and a beam
// >= 0 (wave-uniform), `phony`: the entry is the phony self-loop
__device__ __forceinline__ bool lat_keep(float a, float w, float c, float best, float nbeam, bool live, bool phony, float &s) {
    const float x = (a + w) + c;
    s = x - best;
    return live && !phony && x > MM_NINF && s >= nbeam;
}

// lhs_n(j) of expand(V_b) for the 1-based frame n: the pdf's log-likelihood up to len, the phony pdf's 0 behind it
__device__ __forceinline__ float lat_lhs(const float *Vb, long long vsn, int n, int len, int pdf, int P) {
    if (pdf < P) return n <= len ? Vb[(long long)(n - 1) * vsn + pdf] : MM_NINF;
    return n <= len ? MM_NINF : 0.f;
}

// MM_LAT_E consecutive entries of one thread: one 16-byte load per plane (the planes start on 256 bytes and k is a multiple of 4);
// the last entries of a plane one by one, beyond it nothing is read and the entry is dropped like the phony self-loop
struct LatEntries {
    int src[MM_LAT_E], dst[MM_LAT_E];
    float w[MM_LAT_E];
};
__device__ __forceinline__ void lat_load(const LatticeDev &ld, int k, LatEntries &en) {
    typedef int i4 __attribute__((ext_vector_type(4)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    if (k + MM_LAT_E <= ld.nnz) {
        const i4 s4 = *reinterpret_cast<const i4 *>(ld.src + k), d4 = *reinterpret_cast<const i4 *>(ld.dst + k);
        const f4 w4 = *reinterpret_cast<const f4 *>(ld.w + k);
#pragma unroll
        for (int e = 0; e < MM_LAT_E; ++e) {
            en.src[e] = s4[e];
            en.dst[e] = d4[e];
            en.w[e] = w4[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < MM_LAT_E; ++e) {
            const bool in = k + e < ld.nnz;
            en.src[e] = in ? ld.src[k + e] : -1;
            en.dst[e] = in ? ld.dst[k + e] : 0;
            en.w[e] = in ? ld.w[k + e] : MM_NINF;
        }
    }
}

template <bool LDS, bool WRITE>
__global__ void __launch_bounds__(MM_LAT_NT) mm_lattice_prune_kernel(RunParams p, LatticeParams lp) {
    extern __shared__ __attribute__((aligned(16))) char lat_smem[];
    int *wcnt = reinterpret_cast<int *>(lat_smem);  // [2][4]
    float *arow = reinterpret_cast<float *>(lat_smem + MM_LAT_HEAD);
    const int cell = blockIdx.x, b = cell / p.N, t = cell - b * p.N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int len = p.lens ? p.lens[b] : p.N;
    len = len < 0 ? 0 : (len > p.N ? p.N : len);
    if (t >= len) {
        if (!WRITE && tid == 0) lp.counts[(long long)b * lp.csb + t] = 0;
        return;
    }
    const float best = lp.best[b], beam = lp.beam[b];
    const bool live = best > MM_NINF && beam >= 0.f;  // (a NaN beam compares false)
    if (!live) {
        if (!WRITE && tid == 0) lp.counts[(long long)b * lp.csb + t] = 0;
        return;
    }
    const float nbeam = -beam;
    const UttDesc &u = p.utts[b];
    const LatticeDev &ld = lp.arcs[b];
    const int S1 = u.S1, P = u.P1 - 1, nnz = ld.nnz;
    const float *A = lp.alpha + (long long)t * lp.row_stride + u.state_off;        // frame t + 1
    const float *Bt = lp.beta + (long long)(t + 1) * lp.row_stride + u.state_off;  // frame t + 2
    const float *Vb = p.V + (long long)b * p.vsb;
    float *crow = arow + u.S1p;
    LatEntries cur;  // (the first entries travel while the rows are staged)
    lat_load(ld, tid * MM_LAT_E, cur);
    if (LDS) {
        // four states per thread and turn: their loads are issued together, the emission gathers behind the pdfs together again
        for (int s0 = tid; s0 < S1; s0 += MM_LAT_NT * MM_LAT_E) {
            float av[MM_LAT_E], bv[MM_LAT_E];
            int pd[MM_LAT_E];
#pragma unroll
            for (int e = 0; e < MM_LAT_E; ++e) {
                const int s = s0 + e * MM_LAT_NT;
                const bool in = s < S1;
                av[e] = in ? A[s] : MM_NINF;
                bv[e] = in ? Bt[s] : MM_NINF;
                pd[e] = in ? u.s2p[s] : P;
            }
            float lv[MM_LAT_E];
#pragma unroll
            for (int e = 0; e < MM_LAT_E; ++e) lv[e] = lat_lhs(Vb, p.vsn, t + 2, len, pd[e], P);
#pragma unroll
            for (int e = 0; e < MM_LAT_E; ++e) {
                const int s = s0 + e * MM_LAT_NT;
                if (s < S1) {
                    arow[s] = av[e];
                    crow[s] = lv[e] + bv[e];
                }
            }
        }
    }
    __syncthreads();
    const long long off = WRITE ? lp.offs[cell] : 0;
    if (WRITE && off >= lp.cap) return;  // (every record of the cell lies at or behind cap: block-uniform)
    int base = 0;
    for (int k0 = 0, it = 0; k0 < nnz; k0 += MM_LAT_NT * MM_LAT_E, ++it) {
        const int k = k0 + tid * MM_LAT_E;
        LatEntries nxt;  // (the next turn's entries are on their way while this turn's are decided; behind the plane: nothing is read)
        lat_load(ld, k + MM_LAT_NT * MM_LAT_E, nxt);
        const int(&src)[MM_LAT_E] = cur.src;
        const int(&dst)[MM_LAT_E] = cur.dst;
        const float(&w)[MM_LAT_E] = cur.w;
        bool keep[MM_LAT_E];
        float sc[MM_LAT_E];
        int before = 0, wtotal = 0;
#pragma unroll
        for (int e = 0; e < MM_LAT_E; ++e) {
            const bool phony = src[e] < 0;
            const int i = phony ? 0 : src[e], j = dst[e];
            float a, c;
            if (LDS) {
                a = arow[i];
                c = crow[j];
            } else {
                a = A[i];
                c = lat_lhs(Vb, p.vsn, t + 2, len, u.s2p[j], P) + Bt[j];
            }
            keep[e] = lat_keep(a, w[e], c, best, nbeam, live, phony, sc[e]);
            const unsigned long long m = __ballot(keep[e]);
            before += __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            wtotal += __popcll(m);
        }
        int *wc = wcnt + (it & 1) * 4;
        if (lane == 0) wc[wave] = wtotal;
        __syncthreads();
        int wbase = 0, all = 0;
#pragma unroll
        for (int q = 0; q < MM_LAT_NT / 64; ++q) {
            const int n = wc[q];
            wbase += q < wave ? n : 0;
            all += n;
        }
        if (WRITE) {
            long long r = off + base + wbase + before;
#pragma unroll
            for (int e = 0; e < MM_LAT_E; ++e) {
                if (keep[e]) {
                    if (r < lp.cap) {
                        lp.arc[r] = k + e;
                        lp.score[r] = sc[e];
                    }
                    ++r;
                }
            }
        }
        base += all;
        cur = nxt;
    }
    if (!WRITE && tid == 0) lp.counts[(long long)b * lp.csb + t] = base;
}

__global__ void __launch_bounds__(MM_LAT_NT) mm_lattice_scan_kernel(const int *counts, long long csb, int B, int N, long long *offs, long long *total) {
    __shared__ long long wsum[MM_LAT_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long cells = (long long)B * N;
    long long run = 0;  // the sum of the chunks walked so far (every thread keeps the same value)
    for (long long c0 = 0; c0 < cells; c0 += MM_LAT_NT * 4) {
        const long long c = c0 + tid * 4;
        int v[4];
        long long mine = 0;
        long long row = c / N;  // (one division per thread and chunk: the four cells step from it)
        int col = int(c - row * N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = c + e < cells ? counts[row * csb + col] : 0;
            mine += v[e];
            if (++col == N) {
                col = 0;
                ++row;
            }
        }
        long long inc = mine;  // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long wbase = 0, all = 0;
#pragma unroll
        for (int q = 0; q < MM_LAT_NT / 64; ++q) {
            const long long n = wsum[q];
            wbase += q < wave ? n : 0;
            all += n;
        }
        long long o = run + wbase + inc - mine;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e < cells) offs[c + e] = o;
            o += v[e];
        }
        run += all;
        __syncthreads();  // (wsum is written again by the next chunk)
    }
    if (tid == 0) {
        offs[cells] = run;
        *total = run;
    }
}

}  // namespace mm
