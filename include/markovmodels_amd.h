/* markovmodels_amd.h -- C ABI of the MI355X-native forward-backward / Viterbi
 * engine that sits behind MarkovModels.jl's inference API.
 *
 * Every entry point names the reference interface (file:line under the
 * MarkovModels.jl tree) it replaces.  The reference seam is Julia multiple
 * dispatch on CuArray storage (src/fsm.jl:42-48, src/inference.jl:14-26,
 * src/linalg.jl:163,240,335); this library moves the seam one level up: one
 * call per `pdfposteriors` / `alpha-recursion` / `beta-recursion` instead of
 * four kernel launches per frame.
 *
 * Conventions
 *   - plain C, no C++/torch types; all functions return an int status
 *     (MM_OK = 0, negative = error) and record a message for mm_last_error().
 *   - "device pointer" = memory of the HIP device that was current when the
 *     handle was created; "host pointer" = ordinary memory.  Run calls are
 *     asynchronous on the given hipStream_t (passed as void*, NULL = default
 *     stream) and never synchronise the device.
 *   - the caller owns every in/out buffer; the library owns its handles and
 *     an internal workspace (the alpha store) that grows lazily and is freed
 *     with the batch.  ONE workspace per batch: run calls on the same batch
 *     must be issued on one stream (or otherwise ordered); calls on different
 *     batches are independent.  Growing the workspace frees the old one
 *     (hipFree synchronises): size it once with mm_batch_reserve() before
 *     capturing run calls in a hipGraph -- a run call that would have to grow
 *     the workspace while its stream is capturing fails with MM_ERR_INVALID
 *     instead of invalidating the pointers earlier captures baked in.
 *   - weights/likelihoods are natural-log values of the Log/Tropical
 *     semirings (zero(K) = -inf, one(K) = 0), bit-compatible with the
 *     reference's Array{K} storage.  The fast entries (mm_*_f32) take and return float32 like the reference's
 *     Float32 FSMs; inside, the linear-domain kernels carry float32 or -- for inputs beyond float32's exponent range --
 *     float64 values (mm_batch_set_exact_policy); the generic entry (mm_pdfposteriors_ex) and the linear algebra
 *     (mm_spmv / mm_spmm / mm_svdv) compute in the caller's float type.
 *   - the FSM is the reference's *extended* system (src/fsm.jl:19-28): S1 =
 *     S + 1 states, the last one being the phony final state (self loop of
 *     weight one); P1 = P + 1 pdfs, the last one being the phony pdf that
 *     only the final state emits (examples/prepare-lfmmi-graphs.jl:15-23).
 *   - state / pdf indices RETURNED by the library are 0-based.
 */
#ifndef MARKOVMODELS_AMD_H
#define MARKOVMODELS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ABI_VERSION 4 /* 2: mm_pdfposteriors_ex takes the rows of V_hat (P1); mm_batch_reserve_ex.  3: mm_spmv / mm_spmm / mm_svdv, mm_batch_set_exact_policy.  4: mm_batch_set_mark_policy, mm_batch_set_gamma_mode */

enum mm_status {
    MM_OK = 0,
    MM_ERR_INVALID = -1,     /* bad handle / argument */
    MM_ERR_DIM = -2,         /* the reference's DimensionMismatch (src/linalg.jl:166-167,242-244) */
    MM_ERR_HIP = -3,         /* a HIP runtime call failed */
    MM_ERR_UNSUPPORTED = -4, /* valid input the engine cannot run (e.g. graph too large for LDS) */
    MM_ERR_NOMEM = -5
};

enum mm_semiring { MM_LOG = 0, MM_TROPICAL = 1, MM_PROB = 2 }; /* Semirings.jl LogSemiring / TropicalSemiring / ProbSemiring */
enum mm_layout { MM_CSC = 0, MM_CSR = 1 };        /* how T_hat is handed over */

typedef struct mm_fsm_s *mm_fsm_t;     /* one compiled FSM   ~ CompiledFSM   (src/inference.jl:3-12)  */
typedef struct mm_batch_s *mm_batch_t; /* a batch of them    ~ batch()/rawunion (src/inference.jl:28-36, src/fsmops.jl:28-36) */

int mm_abi_version(void);
/* Message of the last error on the calling thread ("" if none). */
const char *mm_last_error(void);

/* compile(fsm, C_hat) (src/inference.jl:11-12) + adapt to the device
 * (src/inference.jl:14-26): takes the reference FSM fields as they are stored
 * on the host and builds the device-resident packed forms of T_hat' (forward)
 * and T_hat (backward).
 *   S1, nnz      size of T_hat (S1 x S1) and its stored entries
 *   layout       MM_CSC: ptr = colptr (S1+1), idx = rowval  -- SparseMatrixCSC as in src/fsm.jl:14
 *                MM_CSR: ptr = rowptr (S1+1), idx = colval  -- CuSparseMatrixCSR as in src/fsm.jl:45
 *   index_bytes  4 (Cint, src/linalg.jl:80) or 8 (Int64);  index_base 0 or 1 (Julia)
 *   val_bytes    4 (float) or 8 (double) for val / init_val
 *   init_idx/val the n_init stored entries of alpha_hat (src/fsm.jl:10)
 *   state2pdf    S1 entries (index_base based), the column of the single
 *                stored entry of each row of C_hat; the last must be P1-1
 * All pointers are host pointers and are not retained. */
int mm_fsm_create(int semiring, int64_t S1, int64_t nnz, int layout, int index_bytes, int index_base,
                  int val_bytes, const void *ptr, const void *idx, const void *val, int64_t n_init,
                  const void *init_idx, const void *init_val, const int32_t *state2pdf, int32_t P1,
                  mm_fsm_t *out);
/* `compile.(fsms, C_hats)` for a mini-batch of NEW graphs in one call (examples/test_cuda.jl:74-78 builds a fresh batch of
 * numerator graphs every training step): the same arguments as mm_fsm_create, one entry per graph (arrays of n pointers /
 * sizes; semiring, layout and the index / value types are shared).  The graphs are compiled on `threads` host threads
 * (<= 0: up to 16); small log-semiring graphs (the wave kernel's: <= 1023 states, <= 4096 arcs) get their kernel forms at
 * once, and the forms of ALL graphs go to the device as ONE allocation and ONE copy (a handle keeps its share alive:
 * destroy the handles in any order).  out: n handles, each as mm_fsm_create would have made it -- the same results bit for
 * bit; on error none is created.  (Without a HIP device the forms stay on the host until mm_batch_create, as after
 * mm_fsm_create.) */
int mm_fsm_create_many(int64_t n, int semiring, int layout, int index_bytes, int index_base, int val_bytes, const int64_t *S1,
                       const int64_t *nnz, const void *const *ptr, const void *const *idx, const void *const *val,
                       const int64_t *n_init, const void *const *init_idx, const void *const *init_val,
                       const int32_t *const *state2pdf, const int32_t *P1, int threads, mm_fsm_t *out);
int mm_fsm_destroy(mm_fsm_t fsm);
/* nstates + sizes (src/fsm.jl:84); any out pointer may be NULL.
 * packed_slots[d] = arc slots of the packed form, d = 0 forward, 1 backward. */
int mm_fsm_info(mm_fsm_t fsm, int64_t *S1, int64_t *nnz, int32_t *P1, int64_t packed_slots[2],
                int64_t packed_items[2]);

/* batch(cfsm...) (src/inference.jl:28-36) / rawunion(fsms...) (src/fsmops.jl:28-36):
 * B independent FSMs in one block-diagonal system.  Handles may repeat; when
 * all B are the same handle the graph is stored once (denominator case,
 * examples/test_cuda.jl:112).  The FSM handles must outlive the batch. */
int mm_batch_create(const mm_fsm_t *fsms, int64_t B, mm_batch_t *out);
int mm_batch_destroy(mm_batch_t batch);
/* Sum over the batch of S1 (rows of the block-diagonal system). */
int64_t mm_batch_total_states(mm_batch_t batch);
/* Names of the kernels a run entry launches for this batch (the engine picks them from the graphs' sizes and
 * shapes): entry 0 = mm_pdfposteriors_f32, 1 = mm_viterbi_f32 (on the row-lane form: mm_vit_kernel<N4,N2,NJ> +
 * mm_vit_backtrace_kernel<csr in LDS|global memory, R=frames per buffer of its ring>, else the item kernel), 2 = what the last mm_pdfposteriors_ex call on the batch launched
 * (the recursion kernel; for ProbSemiring FSMs in float32 with general state maps, the emission GEMM C_hat * V_hat on the matrix
 * cores before it), 3 = mm_alpharecursion_f32 / mm_betarecursion_f32, 4 = mm_arcposteriors_f32 (log batches only),
 * 5 = mm_samplepaths_f32 (log batches only), 6 = mm_expectedcost_f32 (log batches only), 7 = mm_leakyposteriors_f32 (log batches
 * only),
 * 8 = mm_pathentropy_f32 (log batches only): mm_entropy_fwd_kernel<NI,lds|global> + mm_entropy_bwd_kernel<...>.
 * 9 = mm_filterposteriors_f32 (log batches only): mm_filter_kernel<NI,lds|global>.
 * 10 = mm_windowposteriors_f32 (log batches only): mm_window_fwd_kernel<NI,lds|global> + mm_window_bwd_kernel<...>.
 * 11 = mm_viterbiwindow_f32 (tropical batches only): mm_vitwindow_fwd_kernel<NI,lds|global> + mm_vitwindow_trace_kernel<lds|global>.
 * 12 = mm_weightedposteriors_f32 (log batches only): mm_weights_kernel + mm_log_kernel<MODE_FB,NI,1> + mm_weighted_bwd_kernel<NI,lds|global>
 * + mm_weighted_scatter_kernel.
 * 13 = mm_segmentposteriors_f32 (log batches only): mm_window_fwd_kernel<NI,lds|global> + mm_segment_bwd_kernel<...>.
 * 14 = mm_arcclassposteriors_f32 (log batches only): mm_log_kernel<MODE_FB,NI,1> + mm_arcclass_kernel<NI,lds|global>; the text ends
 * in where the current class plan's term rows live ("terms in LDS" / "terms in global memory" / "no classes set"); ahead of that
 * ending, with a plan set, "class sums on L lanes": the lanes that sum one class in the class pass, the distinct values over the
 * batch's utterances in ascending order ("class sums on 8, 64 lanes").
 * 15 = mm_scoredposteriors_f32 (log batches only): mm_scored_fwd_kernel<NI,lds|global> + mm_scored_bwd_kernel<NI,lds|global>; the text
 * names the class cap and, for the current class plan within the cap, the term cap, the lanes per class and where the term rows
 * live (the endings of entry 14).
 * 16 = mm_classcost_f32 (log batches only): mm_classcost_fwd_kernel<NI,lds|global> + mm_classcost_bwd_kernel<NI,lds|global>; the text
 * names the class cap and says "exceed the cap" when the current class plan has more classes ("no classes set" without a plan).
 * 17 = mm_classpath_f32 (tropical batches only): mm_classpath_fwd_kernel<NI,lds|global> + mm_classpath_trace_kernel; the text names
 * the class cap and says "exceed the cap" when the plan of mm_batch_set_path_classes has more classes ("no classes set" without one).
 * 18 = mm_lattice_f32 (tropical batches only): the two recursions' instances (mm_tropical_kernel<NI,lds|global>,
 * mm_log_kernel<MODE_BETA,NI,lds|global,TROP>), mm_pick_final_kernel, mm_lattice_prune_kernel<lds|global,count>,
 * mm_lattice_scan_kernel and mm_lattice_prune_kernel<lds|global,write>.
 * 19 = mm_latticeposteriors_f32 (tropical batches only): mm_latpost_fb_kernel<threads> + mm_latpost_gamma_kernel<threads>; the text
 * names the state cap and says "exceed the cap" when the batch's largest FSM has more states.
 * 20 = mm_latticecost_f32 (tropical batches only): mm_latcost_fb_kernel<threads> + mm_latcost_grad_kernel<threads>; the text names
 * the bytes of LDS per state and the state cap, and says "exceed the cap" when the batch's largest FSM has more states.
 * 21 = mm_latticebest_f32 (tropical batches only): mm_latbest_kernel<threads>; the text names the bytes of LDS per state and the
 * state cap, and says "exceed the cap" when the batch's largest FSM has more states.
 * 22 = mm_latticesample_f32 (tropical batches only): mm_latsample_fwd_kernel<threads> + mm_latsample_kernel<threads>; the text names
 * the state cap and says "exceed the cap" when the batch's largest FSM has more states.
 * Informational (bench.py quotes it). */
int mm_batch_kernels(mm_batch_t batch, int entry, char *buf, size_t n);
/* Allocate the internal workspace for runs of up to N frames now (synchronises if it has to grow). */
int mm_batch_reserve(mm_batch_t batch, int64_t N);
/* Bytes of internal workspace a run with N frames needs (informational). */
size_t mm_batch_workspace_bytes(mm_batch_t batch, int64_t N);

/* pdfposteriors(fsm, V_hats, C_hats) (src/inference.jl:145-161), with
 * expand() (src/inference.jl:54-60) done inside:
 *   V      device, log-likelihoods of the P = P1-1 real pdfs; element (b, n, p)
 *          at V[b*v_stride_b + n*v_stride_n + p], n = 0..N-1
 *   lens   device int32[B] sequence lengths (<= N), or NULL for all N
 *   gamma  device, out: posterior PROBABILITIES exp(log gamma) like
 *          src/inference.jl:160; element (b, n, p) at
 *          gamma[b*g_stride_b + n*g_stride_n + p*g_stride_p]; frames n >= len_b
 *          are written as exact zeros.  (The reference returns a B x P x N
 *          column-major array: g_stride_b = 1, g_stride_p = B, g_stride_n = B*P.)
 *   ttl    device float[B], out: min over frames of the per-frame log
 *          normaliser (src/inference.jl:159) = log Z_b
 * An utterance with no accepting path (Z = 0) yields gamma = 0, ttl = -inf
 * (the reference yields NaN: src/inference.jl:158; guarded only in the dead
 * code at :198-200).
 * MM_PROB batches of Float32 FSMs (ProbSemiring{Float32}, non-negative weights): V holds LIKELIHOODS -- the semiring's values, like
 * the reference's Array{ProbSemiring} --, the library keeps a log-semiring twin of every such FSM (weights = their logarithms),
 * takes log V in one pass, runs the same fast kernels and returns ttl as the probability Z_b = exp(log Z_b) (0 if no path); gamma is
 * the same quotient in both semirings (:158-160).  Float64 ProbSemiring FSMs, general state maps, V_hat that expand() did not make:
 * mm_pdfposteriors_ex. */
/* Streams: the call is a chain of kernel launches on `stream` and nothing else -- no library-owned streams, no events, no
 * host synchronisation (the forward and the backward agents of an utterance are workgroups of ONE grid per phase); it can be
 * captured in a hipGraph once the workspace is sized (mm_batch_reserve).  Two batches driven from two caller streams do
 * not wait for each other. */
int mm_pdfposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n,
                         const int32_t *lens, int64_t N, float *gamma, int64_t g_stride_b, int64_t g_stride_n,
                         int64_t g_stride_p, float *ttl, void *stream);

/* Arc posteriors: the expected number of times each arc is taken (Baum-Welch's xi summed over the frames), and the expected
 * initial-state occupancy.  For utterance b, with the expanded emissions lhs = C_hat V_hat (expand() semantics, frames
 * 1..N+1, length len_b) and Z_b the value mm_pdfposteriors_f32 normalises by, for each stored entry k = (i -> j) of the
 * caller's T_hat, the phony-final column and the phony self-loop included:
 *
 *   c_b[k]    = sum_{n=1..N} alpha_n(i) * T_hat_ij * lhs_{n+1}(j) * beta_{n+1}(j) / Z_b        (linear, float32 out)
 *   init_b[m] = alpha_hat_i * lhs_1(i) * beta_1(i) / Z_b    for the m-th stored entry i of alpha_hat
 *
 * So the real arcs sum to len_b - 1, the final (omega) arcs to 1, the phony self-loop gets N - len_b, sum_k c_b[k] = N and
 * sum_m init_b[m] = 1 for every utterance that has a path; an utterance with no accepting path (len_b = 0 included) gets all
 * counts 0 and ttl = -inf.  c_b[k] = d log Z_b / d log T_hat_ij: the gradient of log Z with respect to the arc log-weights.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   counts       device, out: c_b[k] at counts[b*c_stride_b + k], k < nnz_b, in the order the caller gave T_hat's entries to
 *                mm_fsm_create (CSC or CSR, as its layout said); slots nnz_b <= k < c_stride_b are left untouched.
 *                c_stride_b < max_b nnz_b: MM_ERR_DIM.  NULL: MM_ERR_INVALID
 *   init_counts  device, out (NULL: not computed): init_b[m] at init_counts[b*i_stride_b + m], m < n_init_b, in init_idx order;
 *                i_stride_b < max_b n_init_b: MM_ERR_DIM
 *   ttl          device float[B], out (NULL: not written): log Z_b, the value mm_pdfposteriors_f32 returns
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on the item form of every FSM (any
 * size): the forward half of the item kernel, then a backward kernel that adds each arc's term to the sum of the one lane that
 * holds the arc -- no atomics, so the result is bit-identical from call to call.  The exact, mark and gamma policies and the
 * posterior floor do not apply to it.  Same stream contract as mm_pdfposteriors_f32: launches on `stream` only, no host
 * synchronisation; it can be captured in a hipGraph once a first call has made the batch's arc forms and sized the workspace. */
int mm_arcposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                         float *counts, int64_t c_stride_b, float *init_counts, int64_t i_stride_b, float *ttl, void *stream);

/* Posteriors with call-time arc weights and their full gradient.  The topology, the state maps and every compiled form of the
 * batch stay as they are; the arc log-weights and the initial log-weights of THIS call come as device tensors:
 *   W       device (NULL: the FSMs' own weights): W[b*w_stride_b + k], k < nnz_b, is the natural-log weight of the k-th stored entry
 *           of T_hat of utterance b's FSM, in the order the caller gave the entries to mm_fsm_create (the order `counts` uses).
 *           Finite, or -inf: the entry is absent for this call.  EVERY stored entry has a slot in both item forms whatever its own
 *           weight (an entry stored with -inf included), so W can set every entry but one: the phony self-loop (final -> final)
 *           is one(K) whatever W holds at its index -- expand() needs it to be.
 *           w_stride_b == 0: one weight vector for the whole batch (and ONE copy of the graph's weights on the device, not B) --
 *           allowed only when all B handles of the batch are the same FSM, else MM_ERR_INVALID; 0 < w_stride_b < max_b nnz_b, or a
 *           negative stride: MM_ERR_DIM
 *   W_init  device (NULL: the FSMs' own alpha_hat): W_init[b*wi_stride_b + m] is the weight of the m-th stored entry of alpha_hat,
 *           in init_idx order; wi_stride_b is checked like w_stride_b (against max_b n_init_b)
 *   gamma, ttl            what mm_pdfposteriors_f32 is defined to return for the batch whose FSMs hold these weights (ttl = log Z_b)
 *   counts, init_counts   what mm_arcposteriors_f32 is defined to return for that batch; slots nnz_b <= k < c_stride_b untouched
 * Each of the four outputs is optional (NULL); all four NULL: MM_ERR_INVALID.  gamma's strides are checked as
 * mm_expectedcost_f32 checks them, c_stride_b and i_stride_b as mm_arcposteriors_f32 does.  Consequently
 *   counts_b[k] = d log Z_b / d W_b[k],  init_counts_b[m] = d log Z_b / d W_init_b[m],  gamma_b = d log Z_b / d V_b,
 * and an entry at -inf has count 0.  Conventions of the arc entry: no accepting path under the call's weights (len_b = 0
 * included): gamma = 0, all counts 0, ttl = -inf; gamma of frames n >= len_b are exact zeros; the phony self-loop's count gets its
 * N - len_b; never a NaN for inputs that are finite or -inf.  The exact, mark and gamma policies and the posterior floor do not
 * apply.  What the arguments alone show is refused ahead of the batch.  MM_LOG batches only: Tropical and ProbSemiring batches
 * return MM_ERR_UNSUPPORTED.
 * The weights are read on the device, on `stream`, when the call runs: the call is a chain of launches on `stream` and nothing
 * else, deterministic (no atomics: the same bits on every run), and can be captured in a hipGraph once a first call has put the
 * forms on the device and sized the workspace (mm_batch_reserve does not cover it; a capture before that: MM_ERR_INVALID) -- a
 * replay after W was overwritten in place follows the new weights. */
int mm_weightedposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                              const float *W, int64_t w_stride_b, const float *W_init, int64_t wi_stride_b,
                              float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p,
                              float *counts, int64_t c_stride_b, float *init_counts, int64_t i_stride_b,
                              float *ttl, void *stream);

/* Posterior path sampling (forward filtering, backward sampling): nsamples state sequences per utterance, drawn from the
 * posterior over complete paths
 *   P(s_1 .. s_len | V) = alpha_hat(s_1) * prod_n lhs_n(s_n) * prod_n T_hat(s_n, s_n+1) * omega(s_len) / Z_b
 * (expand() semantics as mm_pdfposteriors_f32; omega = the column of the phony final state).  The forward half of the item kernel
 * runs ONCE per call; a second kernel walks the frames backwards and draws, given the state j of frame n + 1, the state i of
 * frame n with probability proportional to alpha_n(i) * T_hat_ij.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   nsamples     K >= 1 samples per utterance
 *   seed         any value: the key of the generator (see below)
 *   paths        device int32, out: the state (0-based, the caller's numbering) of sample k of utterance b at frame n at
 *                paths[b*path_stride_b + k*path_stride_k + n] for n < len_b, -1 for len_b <= n < N -- the convention of
 *                mm_viterbi_f32's path; the phony final state never appears.  An utterance without an accepting path
 *                (len_b = 0 included): all -1.  NULL: MM_ERR_INVALID; path_stride_k < N or
 *                path_stride_b < nsamples*path_stride_k: MM_ERR_DIM
 *   logprob      device float, out (NULL: not computed): logprob[b*lp_stride_b + k] = the natural-log posterior probability of
 *                the sampled STATE SEQUENCE, log alpha_hat(s_1) + sum log lhs + sum log T_hat + log omega(s_len) - log Z_b,
 *                accumulated in float64 along the chain; -inf for an utterance without a path.  Parallel entries of T_hat between
 *                the same two states count as ONE transition whose weight is their sum: both the draw and the reported
 *                probability are over state sequences.  lp_stride_b < nsamples: MM_ERR_DIM
 *   ttl          device float[B], out (NULL: not written): log Z_b, the value mm_pdfposteriors_f32 returns; -inf without a path
 * The random numbers.  The result is a function of (graphs, V, lens, N, seed) and of the indices (b, k) alone -- not of nsamples,
 * of the launch geometry, of the stream or of earlier calls: the first K' samples of a call with K > K' are the samples of a call
 * with K', and a repeated call returns the same bits.  The generator is counter based and has no state on the device:
 * Philox-4x32-10 with the 64 bits of `seed` as its key and (b, k, frame, chunk of 64 in-arcs) as its counter, its words turned
 * into uniforms strictly inside (0, 1).  The streams of different (b, k) are independent, and the key is the POSITION b in the
 * batch, not the utterance's content: two utterances with the same graph and emissions receive different samples, and an
 * utterance moved to another position of the batch receives other samples of the same distribution.  A state of probability zero
 * (alpha = 0, or an emission of -inf) is never drawn, whatever the uniform.
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on every log batch (any size) whatever
 * kernels mm_pdfposteriors_f32 picks for it.  Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host
 * synchronisation; it can be captured in a hipGraph once a first call has put the batch's item and sampling forms on the device
 * and sized the workspace (a capture before that returns MM_ERR_INVALID). */
int mm_samplepaths_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                       int64_t nsamples, int64_t seed, int32_t *paths, int64_t path_stride_b, int64_t path_stride_k,
                       float *logprob, int64_t lp_stride_b, float *ttl, void *stream);

/* Expected path cost under the path posterior and its gradient: any frame-decomposable Bayes risk; with
 * cost = -[pdf equals the reference alignment's pdf] over the denominator graph, lattice-free sMBR (Kanda et al., Interspeech 2018).
 * For utterance b with expanded emissions lhs = C_hat * expand(V_b) (frames 1..N+1, length len_b, exactly mm_pdfposteriors_f32's
 * semantics) and costs cost_b(n, p) for the len_b real frames and the P real pdfs (the phony pdf costs 0; frames beyond len_b
 * cost 0 and are NOT READ; the formulas count frames from 1 as the reference does, the arrays from 0 as V does):
 *
 *   A(pi)        = sum_{n=1..len_b} cost_b(n, pdf(s_n))                    for a complete state sequence pi = s_1 .. s_{N+1}
 *   risk_b       = sum_pi P(pi | V_b) * A(pi)
 *   grad_b(n,p)  = d risk_b / d V_b(n,p)    = sum_{j : pdf(j) = p} gamma_n(j) * (E[A | s_n = j] - risk_b)
 *   gamma_b(n,p) = d risk_b / d cost_b(n,p) = the pdf posterior, as mm_pdfposteriors_f32 returns it
 *
 * E[A | s_n = j] = r_n(j) + s_n(j) with the two conditional expectations
 *   r_1(j) = cost(1, pdf j)     r_n(j) = cost(n, pdf j) + sum_i P(s_{n-1}=i | s_n=j, V_{1..n}) * r_{n-1}(i),  P(i | j) ~ alpha_{n-1}(i) T_hat_ij
 *   s_{N+1}(.) = 0              s_n(i) = sum_j P(s_{n+1}=j | s_n=i, V) * (cost(n+1, pdf j) + s_{n+1}(j)),     P(j | i) ~ T_hat_ij lhs_{n+1}(j) beta_{n+1}(j)
 * Both are convex combinations plus an addition; a state no path reaches takes r = s = 0 (0/0 := 0); risk_b = r_{N+1}(final).
 * It follows that risk_b = sum_{n,p} gamma_b(n,p) * cost_b(n,p), that sum_p grad_b(n,p) = 0 for every frame, and that a cost that
 * does not depend on p (cost(n,p) = c_n) gives risk_b = sum_{n<len_b} c_n and grad = 0.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   cost         device, laid out like V: element (b, n, p) at cost[b*c_stride_b + n*c_stride_n + p], n < len_b only; must be
 *                finite there (a non-finite one makes that utterance's outputs unspecified and touches no other utterance).
 *                NULL: MM_ERR_INVALID; c_stride_n < P: MM_ERR_DIM
 *   risk         device float[B], out.  NULL: MM_ERR_INVALID
 *   grad         device, out: element (b, n, p) at grad[b*g_stride_b + n*g_stride_n + p*g_stride_p] (mm_pdfposteriors_f32's meaning
 *                of the three strides: the reference's column-major layout is g_stride_b = 1, g_stride_p = B, g_stride_n = B*P);
 *                frames n >= len_b are exact zeros.  NULL: MM_ERR_INVALID; strides that cannot hold B x N x P distinct elements
 *                (sorted by stride, each must reach past the extent of the one before): MM_ERR_DIM
 *   gamma        device, out with grad's strides (NULL: not written)
 *   ttl          device float[B], out (NULL: not written): log Z_b, the value mm_pdfposteriors_f32 returns
 * An utterance without an accepting path (len_b = 0 included) gets risk 0, grad 0, gamma 0, ttl = -inf.
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on the item form of every FSM (any size),
 * one workgroup per utterance: a forward kernel that carries r beside alpha~ (one 8-byte gather per arc), a backward kernel that
 * carries s beside beta~ and adds the per-pdf sums over fixed lists -- no atomics, so a repeated call returns the same bits.  r and
 * s are carried centred by per-frame float64 offsets, so the float32 values stay near zero whatever the length, and the frame's
 * posterior mean of E[A | s_n] - risk_b (zero by the law of total expectation) is taken out of grad, which removes the rounding the
 * states of a frame share.  The exact, mark
 * and gamma policies and the posterior floor do not apply.  Workspace: the alpha~ store of the item kernel and an r store of the
 * same size, float32 (sum_b S1p_b) x (N + 1) each (config 3 of bench.py at B = 256, N = 1500: 3.1 GB each), grown by the call.
 * Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host synchronisation; it can be captured in a hipGraph
 * once a first call has put the batch's item forms on the device and sized the workspace (a capture before that returns
 * MM_ERR_INVALID). */
int mm_expectedcost_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                        const float *cost, int64_t c_stride_b, int64_t c_stride_n,
                        float *risk, float *grad, float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p,
                        float *ttl, void *stream);

/* Pdf posteriors of the LEAKY HMM: the denominator forward-backward of LF-MMI training as the chain-model trainers run it (the
 * alpha_dash / beta_dash recursion of Kaldi's chain denominator computation, the `leaky` mode of PyChain), written for state
 * emissions.  After every frame a fraction eps of the total forward mass is re-injected into the initial states in the proportions
 * of the initial distribution, so a chunk that does not start or stay on a path from the graph's initial states keeps a finite
 * log Z and a gradient.  For one FSM in the extended system of src/fsm.jl:19-28 (S real states plus the phony final state, initial
 * vector alpha_hat, T_hat = [T omega; 0 1]), with pi(k) = alpha_hat(k) as the caller gave it (not renormalised, zero on the phony
 * state), u the indicator of the real states and eps >= 0 the leak coefficient, T_hat is replaced by
 *
 *   T_eps = (I + eps * u * pi') * T_hat        (semiring sums and products; log semiring: (+) = logaddexp, (*) = +)
 *
 * and everything else is mm_pdfposteriors_f32 unchanged: expand() semantics, lengths, gamma as probabilities normalised per frame,
 * ttl the minimum over the frames of the per-frame log normaliser.  In words: a path may, after any frame and from any real state,
 * jump with weight eps * pi(k) to initial state k; it then takes an ordinary arc of k, the final arc included.  The phony final state
 * never leaks.  eps = 0 is mm_pdfposteriors_f32 itself; log Z is non-decreasing in eps; d log Z_eps / d V(n,p) = gamma_eps(n,p), so
 * the LF-MMI gradient stays a difference of posteriors.  No S x S matrix is formed: with rho(j) = (+)_k pi(k) (*) T_hat(k,j) (one
 * constant per row, the phony final column included) and tot_n = (+)_{i real} alpha_n(i),
 *   alpha_1 = alpha_hat (*) lhs_1
 *   alpha_n(j) = lhs_n(j) (*) [ (+)_i alpha_{n-1}(i) T_hat(i,j)  (+)  eps (*) tot_{n-1} (*) rho(j) ]
 *   z_n(i) = (+)_j T_hat(i,j) lhs_{n+1}(j) beta_{n+1}(j)        c_n = (+)_k pi(k) z_n(k)
 *   beta_n(i) = z_n(i) (+) eps (*) c_n  for real i,   beta_n(final) = z_n(final)        gamma_n(j) ~ alpha_n(j) beta_n(j)
 *   V, lens, N, gamma, strides, ttl   exactly as mm_pdfposteriors_f32: frames n >= len_b are exact zeros; an utterance with no
 *                path even with the leak (len_b = 0, or a frame whose emissions are all -inf) gets gamma = 0 and ttl = -inf.
 *                gamma or ttl NULL: MM_ERR_INVALID; strides that cannot hold B x N x P distinct elements: MM_ERR_DIM
 *   leak         the linear coefficient eps (coefficients in use range from 1e-5 to 0.1); 0 is allowed; negative or non-finite:
 *                MM_ERR_INVALID
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on the item form of every FSM of every log
 * batch (any size, shared or distinct graphs, each with its own pi and rho), one workgroup per utterance, whatever kernels
 * mm_pdfposteriors_f32 picks for the batch: a forward kernel with the leak term in the row epilogue, a backward kernel that forms
 * beta = z (+) eps c between its two barriers and adds the per-pdf sums over fixed lists -- no atomics, so a repeated call returns
 * the same bits.  Like mm_pdfposteriors_f32 the result does not depend on the level of V (a constant added to every emission of a
 * frame changes gamma not at all and ttl by that constant): the float32 sums behind tot and c are taken relative to the frame's
 * largest emission.  A frame in which every live state's own emission lies more than 110 nats below the frame's largest loses its
 * leak (the unleaked result there, never a NaN).  The exact, mark and gamma policies and the posterior floor do not apply.  Workspace: the alpha~ store of the item
 * kernel, grown by the call.  Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host synchronisation; it can be
 * captured in a hipGraph once a first call has put the batch's item forms and leak rows (rho) on the device and sized the workspace
 * (a capture before that returns MM_ERR_INVALID). */
int mm_leakyposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                           float leak, float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p, float *ttl,
                           void *stream);

/* Entropy of the posterior over complete paths and its gradient in the emissions: the objective of semi-supervised sequence
 * training (negative conditional entropy over the denominator graph, for untranscribed audio), the entropy regulariser of LF-MMI /
 * CTC-style losses, a per-utterance confidence figure.  For utterance b the extended system is that of src/fsm.jl:19-28 with
 * lhs = C_hat * expand(V_b), frames 1..N+1 and length len_b -- exactly mm_pdfposteriors_f32's semantics; a path is a complete
 * state sequence pi = s_1 .. s_{N+1} and P(pi) = w(pi) / Z_b its posterior:
 *
 *   H_b          = - sum_pi P(pi) ln P(pi)                                                                   (nats; >= 0)
 *   Hf_1(j) = 0     Hf_n(j) = sum_i P(i | j) (Hf_{n-1}(i) - ln P(i | j)),  P(i | j) ~ alpha_{n-1}(i) T_hat_ij     (the entropy of the prefix given s_n = j)
 *   Hb_{N+1}(.) = 0 Hb_n(i) = sum_j P(j | i) (Hb_{n+1}(j) - ln P(j | i)),  P(j | i) ~ T_hat_ij lhs_{n+1}(j) beta_{n+1}(j)  (... of the suffix given s_n = i)
 *   H_b          = Hf_{N+1}(final)
 *   grad_b(n,p)  = d H_b / d V_b(n,p) = sum_{j : pdf(j) = p} q_n(j) * (Hf_n(j) + Hb_n(j) - ln q_n(j) - H_b),   q_n(j) the state posterior
 *
 * (the entropy semiring: Hernando et al. 2005, Li & Eisner 2009).  0 * ln 0 := 0; a state no path reaches carries Hf = Hb = 0.
 * It follows that sum_p grad_b(n,p) = 0 for every frame, that a constant added to all emissions of a frame changes neither H nor
 * grad, that a graph with a single path of positive weight gives H = 0 and grad = 0, and that paths of equal weight give
 * H = ln(number of paths).  The paths are sequences of stored entries of T_hat: parallel entries between the same two states,
 * which the reference's sparse() combines and its FSMs therefore never hold, would count as distinct transitions.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   entropy      device float[B], out: H_b.  NULL: MM_ERR_INVALID
 *   grad         device, out (NULL: not written): element (b, n, p) at grad[b*g_stride_b + n*g_stride_n + p*g_stride_p], the three
 *                strides as mm_expectedcost_f32's; frames n >= len_b are exact zeros.  Strides that cannot hold B x N x P distinct
 *                elements: MM_ERR_DIM (not looked at when grad and gamma are both NULL)
 *   gamma        device, out with grad's strides (NULL: not written): the pdf posterior, as mm_pdfposteriors_f32 returns it
 *   ttl          device float[B], out (NULL: not written): log Z_b, the value mm_pdfposteriors_f32 returns
 * grad == NULL and gamma == NULL is allowed and runs the forward kernel alone: entropy and ttl, bit for bit those of the full
 * call, with no frame kept in the workspace (confidence scoring).
 * An utterance without an accepting path (len_b = 0 included) gets entropy 0, grad 0, gamma 0, ttl = -inf; len_b = 1 gives the
 * entropy of the choice of the single state.
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on the item form of every FSM (any size),
 * one workgroup per utterance: a forward kernel that carries Hf beside alpha~ (one 8-byte gather per arc; the conditional
 * probabilities are the terms of the row's log-sum-exp), a backward kernel that carries Hb beside beta~ and adds the per-pdf sums
 * over fixed lists -- no atomics, so a repeated call returns the same bits.  Hf and Hb are carried centred by per-frame float64
 * offsets, so the float32 values stay near zero whatever the length, and the frame's posterior mean of the bracket (zero by the
 * chain rule of entropy) is taken out of grad.  The exact, mark and gamma policies and the posterior floor do not apply.
 * Workspace: the alpha~ store of the item kernel and an Hf store of the same size, float32 (sum_b S1p_b) x (N + 1) each, grown by
 * the call; for a value-only call the Hf store is not allocated.  Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host
 * synchronisation; it can be captured in a hipGraph once a first call has put the batch's item forms on the device and sized the
 * workspace (a capture before that returns MM_ERR_INVALID). */
int mm_pathentropy_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                       float *entropy, float *grad, float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p,
                       float *ttl, void *stream);

/* Forward filtering posteriors with a carried state: the causal quantities of a log batch -- what online confidence, keyword /
 * filler spotting, HMM-smoothed activity detection and endpointing run on -- and the way to run a recursion over audio in chunks.
 * Every other posterior of this header is a smoothing quantity and needs the whole utterance.  For utterance b the extended system
 * is that of src/fsm.jl:19-28 (S real states and the phony final state f, T_hat = [T omega; 0 1]) with lhs = C_hat * expand(V_b)
 * and length len = len_b, exactly as mm_pdfposteriors_f32 uses it; frames counted from 1 here and from 0 in the arrays:
 *
 *   start(j)     = alpha_hat(j)  (state_in == NULL)   or   exp(state_in_b(j))   for real j;   start(f) = 0
 *   a_1(j)       = start(j) lhs_1(j)
 *   a_n(j)       = lhs_n(j) sum_i a_{n-1}(i) T_hat(i,j)                  n = 2..len     (a_n(f) = 0: the phony pdf is -inf there)
 *   l_n          = ln sum_j a_n(j),   l_0 := 0
 *   incr(n)      = l_n - l_{n-1}                                         ln P(V_n | V_1..n-1) given the start vector
 *   filt(n,p)    = sum_{j : pdf(j) = p} a_n(j) / sum_j a_n(j)            the filtering posterior; rows sum to 1
 *   state_out(j) = ln sum_i a_len(i) T_hat(i,j) - l_len                  for ALL j of the extended system, j = f included
 *   ttl          = l_len + state_out(f)                                  = log Z_b when state_in == NULL
 *
 * state_out is the one-step prediction before the next emission, normalised by the mass alive at the last frame; its final entry
 * is the log of the fraction of that mass the final weights accept.  It follows that sum_n incr(n) + state_out(f) is the log Z
 * mm_pdfposteriors_f32 normalises by; that CHUNKING IS EXACT -- a call on frames 1..L1 and a second call on frames L1+1..L with
 * state_in = the first call's state_out give, concatenated, the filt and incr of the single call, and log Z = the sum of incr over
 * all chunks + state_out(f) of the last chunk --; that filt(n,.) and incr(n) do not depend on V at frames after n; that on a graph
 * whose final weights are the same for every real state filt(len,.) is the smoothing posterior gamma(len,.) (on other graphs it is
 * not); and that a constant added to all emissions of a frame changes filt not at all and incr of that frame by that constant.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   state_in     device float[mm_batch_total_states], natural log: element (b, s) at state_offset_b + s (one column of
 *                mm_alpharecursion_f32's layout).  NULL: the FSMs' own initial vectors.  The entry of the phony final state is ignored
 *   state_out    device, out, same layout (NULL: not written).  state_in == state_out is allowed: a workgroup reads its segment
 *                before it writes it
 *   filt         device, out (NULL: not computed): element (b, n, p) at filt[b*f_stride_b + n*f_stride_n + p*f_stride_p],
 *                probabilities; the strides as mm_leakyposteriors_f32's (the reference's column-major B x P x N layout included).
 *                Strides that cannot hold B x N x P distinct elements: MM_ERR_DIM
 *   incr         device, out (NULL: not written): element (b, n) at incr[b*i_stride_b + n].  i_stride_b < N: MM_ERR_DIM
 *   ttl          device float[B], out (NULL: not written)
 * All four outputs NULL: MM_ERR_INVALID.  Conventions: frames n >= len_b of filt and incr are exact zeros.  len_b = 0 gives
 * filt = 0, incr = 0, ttl = -inf and state_out = a copy of state_in -- with state_in == NULL: ln alpha_hat, the vector NULL stands
 * for (how a caller obtains a reset vector).  An utterance whose alive mass becomes zero at frame d <= len_b (a frame of all -inf,
 * a start vector without a live state) keeps its values of the frames before d; from d on filt = 0 and incr = -inf, ttl = -inf and
 * state_out = -inf everywhere.  Nothing is NaN.
 * MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.  Runs on the item form of every FSM of every log
 * batch (any size, shared or distinct graphs), one workgroup per utterance, whatever kernels mm_pdfposteriors_f32 picks for the
 * batch: ONE kernel, the forward step of the item kernel; behind each step's barrier the per-pdf sums of the finished frame are
 * taken over fixed lists relative to that frame's own maximum -- no atomics, so a repeated call returns the same bits, and filt
 * does not depend on the level of V.  No frame is kept: the call uses no workspace, whatever N.  The exact, mark and gamma policies
 * and the posterior floor do not apply.  Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host
 * synchronisation; it can be captured in a hipGraph once a first call has put the batch's item forms on the device (a capture
 * before that returns MM_ERR_INVALID). */
int mm_filterposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                            const float *state_in, float *state_out,
                            float *filt, int64_t f_stride_b, int64_t f_stride_n, int64_t f_stride_p,
                            float *incr, int64_t i_stride_b, float *ttl, void *stream);

/* Fixed-lag smoothing posteriors: the forward-backward of a log batch over a WINDOW of the audio, which starts from a carried vector
 * instead of the FSM's initial vector and ends open (beta = 1 on every real state: the audio goes on) or on the final weights.
 * What lies between mm_filterposteriors_f32 (causal, nothing of the future) and the smoothing entries (the whole utterance):
 * P(pdf_n | V_1..n+L) for online alignment, keyword spotting, endpointing and confidence, and the forward-backward of training on
 * long recordings cut into windows (ttl = ln P(window | carried start), d ttl / d V = gamma, the next window continues from
 * state_out where mm_leakyposteriors_f32 restarts from the initial distribution).  For utterance b the extended system and
 * lhs = C_hat * expand(V_b) are exactly those of mm_filterposteriors_f32, len = len_b; frames counted from 1 here and from 0 in the
 * arrays, f the phony final state:
 *
 *   start(j)     = alpha_hat(j)  (state_in == NULL)   or   exp(state_in_b(j))   for real j;   start(f) = 0
 *   a_1(j)       = start(j) lhs_1(j);   a_n(j) = lhs_n(j) sum_i a_{n-1}(i) T_hat(i,j)     n = 2..len      (the filter's a_n)
 *   l_n          = ln sum_j a_n(j),   l_0 := 0
 *   b_len(i)     = 1                   (closed_b == 0: the audio goes on behind the window)
 *   b_len(i)     = T_hat(i, f)         (closed_b != 0: the audio ends at frame len; the final weights)
 *   b_n(i)       = sum_{j real} T_hat(i,j) lhs_{n+1}(j) b_{n+1}(j)                         n < len
 *   gamma(n,p)   = sum_{j : pdf(j) = p} a_n(j) b_n(j) / sum_j a_n(j) b_n(j)                rows sum to 1
 *   ttl          = ln sum_j a_len(j) b_len(j)      open: = l_len = ln P(V_1..len | start); closed and state_in == NULL: = log Z_b
 *   c            = commit_b clamped to [0, len]    (commit == NULL: c = len)
 *   state_out(j) = ln sum_i a_c(i) T_hat(i,j) - l_c     for ALL j, f included: the filter's state_out after c frames
 *   lcommit      = l_c
 *
 *   V, lens, N   as mm_pdfposteriors_f32
 *   state_in, state_out   layout and aliasing rule of mm_filterposteriors_f32: they may be one buffer.  state_out NULL: not written
 *   closed       device int32[B]; NULL: every utterance is open
 *   commit       device int32[B]; NULL: c = len
 *   lcommit      device float[B], out (NULL: not written)
 *   gamma        device, out: element (b, n, p) at gamma[b*g_stride_b + n*g_stride_n + p*g_stride_p]; the strides as
 *                mm_leakyposteriors_f32's.  NULL: MM_ERR_INVALID.  Strides that cannot hold B x N x P distinct elements: MM_ERR_DIM
 *   ttl          device float[B], out (NULL: not written)
 * Argument errors that need no device are reported before the NULL-batch check.  MM_LOG batches only: Tropical and ProbSemiring
 * batches return MM_ERR_UNSUPPORTED.
 * Conventions: frames n >= len of gamma are exact zeros.  len = 0 gives gamma = 0, ttl = -inf, lcommit = 0 and state_out = a copy
 * of the start vector (state_in == NULL: ln alpha_hat).  c = 0 with len > 0 also gives a copy of the start vector and lcommit = 0.
 * A window of zero total mass -- the alive mass dies at some frame d <= len, or the window is closed and the final weights accept
 * none of it -- gives gamma = 0 in all its frames and ttl = -inf; its state_out and lcommit are still the prefix's values when every
 * frame up to c is alive, else -inf.  Nothing is NaN.
 * Consequences: (a) closed with state_in == NULL: gamma and ttl are those of mm_pdfposteriors_f32.  (b) open: gamma(len,.) =
 * filt(len,.) of mm_filterposteriors_f32, ttl = the sum of its incr, and with c = len state_out is its state_out.  (c) RE-WINDOWING
 * IS EXACT: a window over frames 1..M with commit c and a second window over frames c+1..M with state_in = the first window's
 * state_out and the same closed: the second has the first's gamma on frames c+1..M, and its ttl = the first's ttl - the first's
 * lcommit.  (d) a constant added to every emission of a frame changes gamma not at all and ttl by that constant.  (e) d ttl /
 * d V(n,p) = gamma(n,p).  (f) gamma(n,.) of an open window does not depend on frames after len.  (g) no atomics: a repeated call
 * returns the same bits.
 * Runs on the item form of every FSM of every log batch, one workgroup per utterance: mm_window_fwd_kernel (the filter kernel's
 * step; the frame's largest emission lives in the float64 offset, every alpha~ row is stored) and mm_window_bwd_kernel (per-pdf
 * sums over fixed lists, each frame normalised by its own sum).  The exact, mark and gamma policies and the posterior floor do not
 * apply.  Workspace: the alpha~ store of the item kernel, float32 (sum_b S1p_b) x (N + 1), grown by the call.  Stream contract of
 * mm_arcposteriors_f32: launches on `stream` only, no host synchronisation; it can be captured in a hipGraph once a first call has
 * put the batch's item forms on the device and sized the workspace (a capture before that returns MM_ERR_INVALID). */
int mm_windowposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                            const float *state_in, const int32_t *closed, const int32_t *commit, float *state_out, float *lcommit,
                            float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p, float *ttl, void *stream);

/* Segment posteriors: the forward-backward of a log batch over a SEGMENT of the audio, which starts from a carried vector like a
 * window of mm_windowposteriors_f32 and ends open, on the final weights or on a carried END vector -- and hands back the end vector
 * of the segment before it.  What the window entry cannot do: end on what comes after it.  With it the exact smoothing posteriors
 * of a long recording -- the gamma of mm_pdfposteriors_f32, the LF-MMI gradient -- take the workspace of ONE chunk, whatever the
 * length of the audio: pass 1 is mm_filterposteriors_f32 over the chunks (no frame kept; the start state of every chunk saved),
 * pass 2 this entry over the chunks in reverse, each from its saved state, ending on the vector the chunk behind it returned.
 * The extended system, lhs, start, a_n and l_n are exactly mm_windowposteriors_f32's; frames counted from 1 here and from 0 in the
 * arrays, f the phony final state:
 *
 *   b_len(i)     = 1                     end_mode_b == 0                                          (open)
 *   b_len(i)     = T_hat(i, f)           end_mode_b != 0 and (end_mode_b != 2 or end_in == NULL)  (the final weights)
 *   b_len(i)     = exp(end_in_b(i))      end_mode_b == 2 and end_in != NULL                       (carried), real i; f's entry is not read
 *   b_n(i)       = sum_{j real} T_hat(i,j) lhs_{n+1}(j) b_{n+1}(j)                         n < len
 *   gamma(n,p)   = sum_{j : pdf(j) = p} a_n(j) b_n(j) / sum_j a_n(j) b_n(j)
 *   ttl          = ln sum_j a_len(j) b_len(j)
 *   b_0(i)       = sum_{j real} T_hat(i,j) lhs_1(j) b_1(j)      for ALL i of the extended system (b_0(f) = 0)
 *   lend         = ln max_i b_0(i)
 *   end_out(i)   = ln b_0(i) - lend      the largest entry is 0; the entry of f is -inf
 *
 *   V, lens, N, state_in, gamma and its strides, ttl   as mm_windowposteriors_f32
 *   end_mode     device int32[B]; NULL: every utterance is open
 *   end_in, end_out   layout of state_in / state_out (natural log, element (b, s) at state_offset_b + s).  They may be one buffer: a
 *                workgroup reads its segment before it writes it.  end_out NULL: not written
 *   lend         device float[B], out (NULL: not written)
 * gamma NULL: MM_ERR_INVALID; strides that cannot hold B x N x P distinct elements: MM_ERR_DIM; both are reported before the
 * NULL-batch check.  MM_LOG batches only: Tropical and ProbSemiring batches return MM_ERR_UNSUPPORTED.
 * Conventions (nothing is NaN): frames n >= len of gamma are exact zeros.  len = 0 gives gamma = 0, ttl = -inf, and end_out = the
 * end vector the segment was given: carried -- a copy of end_in as given, its final entry included, lend = 0; open -- 0 on the real
 * states and -inf on f, lend = 0; final -- ln T_hat(i, f) - its maximum, lend = that maximum (no final weight at all: all -inf and
 * lend = -inf).  A segment without mass -- the alive mass dies at a frame <= len, a start or end vector has no live state, or the
 * total is zero -- gives gamma = 0, ttl = -inf, end_out = -inf everywhere and lend = -inf: a dead utterance propagates backwards
 * through the chunks.
 * Consequences: (a) with end_in == NULL gamma and ttl are those of mm_windowposteriors_f32 with closed = end_mode.  (b) CHAINING IS
 * EXACT: segment A on frames 1..L1, segment B on frames L1+1..L started from the filter's state_out after L1 frames, with any end;
 * A with end_mode = 2 and end_in = B's end_out.  Then A has, on its frames, the gamma of the one call over 1..L with B's end, B has
 * that gamma on its own frames, and ttl_A + lend_B = the one call's ttl.  (c) a constant added to all emissions of a frame changes
 * gamma and end_out not at all, ttl and lend by that constant.  (d) a constant added to end_in_b changes ttl and lend by it (b_0 is
 * linear in b_len) and nothing else.  (e) d ttl / d V(n,p) = gamma(n,p).  (f) end_out and lend do not depend on state_in, as long as the segment has mass.
 * (g) no atomics: a repeated call returns the same bits.
 * Runs on the item form of every FSM of every log batch, one workgroup per utterance: mm_window_fwd_kernel as the window entry
 * launches it, then mm_segment_bwd_kernel (the window's backward loop; a carried end's total from the stored alpha~ row of frame len
 * and the end vector; one more item pass behind frame 1 for end_out and lend).  Workspace: the window entry's, the alpha~ store for
 * N frames.  Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host synchronisation; it can be captured in a
 * hipGraph once a first call has put the batch's item forms on the device and sized the workspace (a capture before that returns
 * MM_ERR_INVALID). */
int mm_segmentposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                             const float *state_in, const int32_t *end_mode, const float *end_in, float *end_out, float *lend,
                             float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p, float *ttl, void *stream);

/* Per-frame arc-class posteriors: Baum-Welch's xi_n (L. E. Baum et al., "A maximization technique occurring in the statistical
 * analysis of probabilistic functions of Markov chains", 1970; Rabiner 1989, eq. 37), summed over classes of arcs instead of over
 * the frames.  mm_batch_set_arc_classes gives every stored entry k = (i_k -> j_k) of an FSM's T_hat -- the phony-final column and
 * the phony self-loop included, in the order mm_arcposteriors_f32 reports them -- a class cls[k] in {-1, 0, ..., C-1}; -1: not
 * counted.  For utterance b of length len, frames 1-based inside the formula, t = 0 .. N-1:
 *
 *   xi[b, c, t] = sum_{k : cls[k] = c}  alpha_{t+1}(i_k) * T_hat_{i_k j_k} * lhs_{t+2}(j_k) * beta_{t+2}(j_k) / Z_b
 *
 * with Z_b the normaliser of mm_pdfposteriors_f32.  So: for t < len-1 the terms are real arcs; at t = len-1 they are the arcs into
 * the phony final state; for t >= len only the phony self-loop is alive -- its class, if it has one, gets exactly 1.0f and every
 * other class exactly 0.0f.  If every entry has a class, sum_c xi[b, c, t] = 1 for every t < N.  sum_t xi[b, c, t] = the sum of
 * mm_arcposteriors_f32's counts over the entries of class c.  With cls[k] = the pdf of the source state i_k, xi[b, p, t] =
 * gamma[b, p, t] for t < len; with cls[k] = the pdf of the destination j_k (the phony pdf = P, so C = P + 1), xi[b, p, t] =
 * gamma[b, p, t+1] for t+1 < len, and class P holds the final arcs at t = len-1 and the phony loop behind it.  An utterance with
 * no accepting path gets xi = 0 everywhere and ttl = -inf; len = 0 with a path: every frame is the phony loop's (as the counts of
 * mm_arcposteriors_f32).  No gradient of xi is offered (it is second order).
 *
 * mm_batch_set_arc_classes: host arrays, not retained.  offsets NULL: one array of nnz ids for a batch of ONE shared FSM; else
 * offsets[B + 1] into cls, utterance b's nnz_b ids at cls[offsets[b]] (a wrong slice length: MM_ERR_DIM).  C < 1, an id outside
 * [-1, C), a batch of several FSMs without offsets: MM_ERR_INVALID.  Host work only: the classified entries are ranked by (class,
 * entry index) per distinct (FSM, class array); the first mm_arcclassposteriors_f32 call behind it puts the plan on the device in
 * one allocation and one copy (never during a stream capture: MM_ERR_INVALID).  Calling it again replaces the plan.
 * mm_batch_arc_class_info: cap = the most classified entries of one utterance whose per-frame terms the kernel keeps in LDS for
 * this batch (beyond it they live in the workspace), max_M = the most any utterance of the current plan has (-1: no plan), C.
 *
 *   V, lens, N   as mm_pdfposteriors_f32
 *   xi           device, out: element (b, c, t) at xi[b*x_stride_b + t*x_stride_n + c*x_stride_c]; strides that cannot hold
 *                B x N x C elements: MM_ERR_DIM.  NULL: MM_ERR_INVALID
 *   ttl          device float[B], out (NULL: not written): log Z_b
 * MM_LOG batches only (others: MM_ERR_UNSUPPORTED); no classes set: MM_ERR_INVALID.  Runs on the item form of every FSM: the
 * forward half of the item kernel, then mm_arcclass_kernel: the beta~ recursion of the arc entry with its per-frame correction,
 * one owning thread per classified entry and frame, class sums in a fixed order -- no atomics, a repeated call returns the same
 * bits, and relabelling the classes permutes the rows of xi bit for bit.  Stream contract of mm_arcposteriors_f32: launches on
 * `stream` only; it can be captured in a hipGraph once a first call has put the plan on the device and sized the workspace. */
int mm_batch_set_arc_classes(mm_batch_t batch, const int32_t *cls, const int64_t *offsets, int32_t C);
int mm_batch_arc_class_info(mm_batch_t batch, int64_t *cap, int64_t *max_M, int32_t *C);
int mm_arcclassposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                              float *xi, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_c, float *ttl, void *stream);

/* Posteriors with per-frame arc-class scores and their gradient.  Under the class plan of mm_batch_set_arc_classes, a complete
 * path of utterance b (length len; frames 1-based inside the formula, t 0-based as in mm_arcclassposteriors_f32) weighs
 *
 *   alpha_hat(s_1) * prod_n lhs_n(s_n) * prod_{t=0}^{len-1} T_hat[k_t] * exp(U[b, t, cls(k_t)])
 *
 * with k_t the stored entry taken from frame t+1 to frame t+2 (t = len-1: the arc into the phony final state); Z_b(U) is the sum
 * over the paths.  An entry of class -1 contributes exp(0); parallel entries between the same two states are scored one by one;
 * the phony self-loop stays one(K) whatever its class holds (as under mm_weightedposteriors_f32).  U is finite or -inf (-inf
 * removes the class at that transition); rows t >= len are never read.  For finite or -inf inputs no output is ever NaN.
 *
 *   V, lens, N   as mm_pdfposteriors_f32
 *   U            device, element (b, t, c) at U[b*u_stride_b + t*u_stride_n + c*u_stride_c], natural log; strides that cannot hold
 *                B x N x C elements: MM_ERR_DIM.  NULL: all zeros (no scores)
 *   gamma        device, out (NULL: not computed): d log Z_b / d V -- what mm_pdfposteriors_f32 would return if the scores were
 *                part of the graph; frames n >= len are exact zeros.  Strides checked as mm_weightedposteriors_f32 checks them
 *   xi           device, out (NULL: not computed), laid out as mm_arcclassposteriors_f32's: xi by class under Z_b(U).  For t < len
 *                it is d log Z_b / d U[b, t, c]; for t >= len and for an utterance without a path the conventions of
 *                mm_arcclassposteriors_f32 hold (the phony loop's class exactly 1.0f, the others exactly 0.0f; no path: 0)
 *   ttl          device float[B], out (NULL: not written): log Z_b(U); -inf without a path
 * gamma, xi and ttl all NULL: MM_ERR_INVALID.  With U NULL xi and ttl are those of mm_arcclassposteriors_f32 and gamma that of
 * mm_pdfposteriors_f32, from ONE forward pass; with U constant in t (U[b, t, c] = u_c) the result is that of
 * mm_weightedposteriors_f32 with W[k] = w_k + u_{cls[k]}.
 * MM_LOG batches only (others: MM_ERR_UNSUPPORTED); no classes set, or a first call during a stream capture: MM_ERR_INVALID; more
 * classes than mm_batch_score_class_cap reports -- the classes whose two score rows fit the LDS beside the kernel's plan --:
 * MM_ERR_UNSUPPORTED, the message names the cap.  Runs on the item form of every FSM: mm_scored_fwd_kernel (the item kernel's
 * forward loop, every arc adding its class's entry of the transition's score row, staged in LDS one step ahead), then
 * mm_scored_bwd_kernel (the loop of mm_arcclass_kernel with the score in the beta~ recursion and in every term, and a per-pdf pass
 * in a fixed order for gamma).  The class ids travel in a plane of 16-bit ids parallel to the slots of each item form, built with
 * the class plan and replaced with it.  Stream contract of the arc entries: launches on `stream` only; no atomics, the same bits on
 * every run; capturable in a hipGraph after a first call has put the plan on the device and sized the workspace; a replay after U
 * was overwritten in place follows the new scores. */
int mm_scoredposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                            const float *U, int64_t u_stride_b, int64_t u_stride_n, int64_t u_stride_c,
                            float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p,
                            float *xi, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_c, float *ttl, void *stream);
int mm_batch_score_class_cap(mm_batch_t batch, int64_t *cap);

/* Expected arc-class cost under the path posterior and its gradient: a Bayes risk whose costs sit on the arcs -- with
 * A = -[class equals the reference's class at that transition] over the denominator graph, lattice-free MPE / MWE (a phone or a
 * word is right or wrong where its arc is entered); insertion and length penalties; an expected number of boundaries.  Under the
 * class plan of mm_batch_set_arc_classes, for utterance b of length len, with class costs A[b, t, c], t = 0 .. len-1, on the
 * transition index of mm_arcclassposteriors_f32 (entry k_t leads from frame t+1 to frame t+2, frames 1-based inside the formulas;
 * t = len-1: the arc into the phony final state) and optional pdf costs D[b, n, p] that mean exactly what mm_expectedcost_f32's
 * cost means:
 *
 *   A(pi)        = sum_{n=1..len} D(n, pdf(s_n))  +  sum_{t=0..len-1} A(t, cls(k_t))
 *   risk_b       = sum_pi P(pi | V_b) * A(pi)
 *   grad_b(n,p)  = d risk_b / d V_b(n,p) = sum_{j : pdf(j) = p} gamma_n(j) * (r_n(j) + s_n(j) - risk_b)
 *
 *   r_1(j) = D(1, pdf j)
 *   r_n(j) = D(n, pdf j) + sum_{k into j} P(k | s_n=j, V_1..n) * (r_{n-1}(i_k) + A(n-2, cls k)),     P(k | j) ~ alpha_{n-1}(i_k) T_hat[k]
 *   s_{N+1} = 0
 *   s_n(i) = sum_{k out of i} P(k | s_n=i, V) * (A(n-1, cls k) + D(n+1, pdf j_k) + s_{n+1}(j_k)),    P(k | i) ~ T_hat[k] lhs_{n+1}(j_k) beta_{n+1}(j_k)
 *   risk_b = r_{N+1}(final)
 *
 * Conventions (the scored entry's wherever both share a case): an entry of class -1 costs 0; the phony self-loop costs 0 whatever
 * class it holds; parallel entries between the same two states are costed one by one, each with its own class; rows t >= len of A
 * and n >= len of D are NEVER READ; A and D must be finite where they are read (a non-finite value leaves that utterance's outputs
 * unspecified and touches no other utterance); an utterance without an accepting path (len = 0 included) gets risk 0, grad 0,
 * gamma 0 and ttl = -inf; nothing is NaN for finite costs and finite or -inf emissions.
 * Identities: with A = 0 the outputs are those of mm_expectedcost_f32 on D; with cls[k] = the pdf of the source state i_k,
 * A[b, t, p] = D'[b, t, p] and D NULL they are those of mm_expectedcost_f32 on D'; risk_b = sum_{n,p} gamma_b(n,p) D_b(n,p) +
 * sum_{t<len,c} xi_b(c,t) A_b(t,c) with xi of mm_arcclassposteriors_f32; with every entry classified and A[b, t, c] = a_t,
 * risk_b = sum_{t<len} a_t and grad = 0; sum_p grad_b(n,p) = 0 for every frame.  d risk_b / d A[b, t, c] = xi_b(c, t) and
 * d risk_b / d D = gamma: the first is what mm_arcclassposteriors_f32 returns and is not an output here.
 *   V, lens, N   as mm_pdfposteriors_f32
 *   A            device, element (b, t, c) at A[b*a_stride_b + t*a_stride_n + c*a_stride_c]; strides that cannot hold B x N x C
 *                elements: MM_ERR_DIM (as mm_scoredposteriors_f32 checks U).  NULL: MM_ERR_INVALID
 *   D            device, as mm_expectedcost_f32's cost (d_stride_n < P: MM_ERR_DIM).  NULL: zeros
 *   risk, grad   device, out, required (NULL: MM_ERR_INVALID); grad's strides as mm_expectedcost_f32's, frames n >= len exact zeros
 *   gamma, ttl   device, out, optional (NULL: not written): meaning and stride rules of mm_expectedcost_f32
 * MM_LOG batches only (others: MM_ERR_UNSUPPORTED); no class plan: MM_ERR_INVALID; more classes than mm_batch_cost_class_cap
 * reports -- the largest C whose two cost rows of C + 1 floats (padded to 4) fit the LDS behind the cost kernels' plan, at most
 * 65 534 --: MM_ERR_UNSUPPORTED, the message names the cap.  Runs on the item form of every FSM, one workgroup per utterance:
 * mm_classcost_fwd_kernel and mm_classcost_bwd_kernel, the loops of mm_expectedcost_f32's kernels in which every arc adds its
 * class's entry of the transition's cost row (staged in LDS one step ahead, not scaled) to the gathered second operand; the class
 * ids travel in the 16-bit planes of mm_scoredposteriors_f32.  r and s are carried centred as in mm_expectedcost_f32, the class
 * term with them.  Workspace: mm_expectedcost_f32's -- the alpha~ store and an r store of the same size, float32
 * (sum_b S1p_b) x (N + 1) each --, grown by the call: mm_batch_workspace_bytes and mm_batch_reserve do NOT cover it (they size
 * mm_pdfposteriors_f32's workspace), so before a capture a first call with the same N is required.  Stream contract of the arc entries: launches on `stream` only; no host
 * synchronisation; no atomics, so a repeated call returns the same bits; capturable in a hipGraph after a first call has put the
 * class planes on the device and sized the workspace; a first call during a capture returns MM_ERR_INVALID. */
int mm_classcost_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                     const float *A, int64_t a_stride_b, int64_t a_stride_n, int64_t a_stride_c,
                     const float *D, int64_t d_stride_b, int64_t d_stride_n,
                     float *risk, float *grad, float *gamma, int64_t g_stride_b, int64_t g_stride_n, int64_t g_stride_p,
                     float *ttl, void *stream);
int mm_batch_cost_class_cap(mm_batch_t batch, int64_t *cap);

/* alpha-recursion(alpha_hat, T_hat', C_hat*V_hat) (src/inference.jl:62-74) as
 * called from pdfposteriors (:150-152): out is the reference's state_A, a
 * (sum S1) x (N+1) column-major matrix: element (b, n, s) at
 * out[n*out_stride_n + state_offset_b + s] with state_offset_b the running sum
 * of S1 over the batch.  Values are natural-log (un-normalised).
 * One shared graph in the pair form (the batches of mm_fbp_kernel, up to 250 pdfs) runs phase A of the pair kernels over all
 * N + 1 frames -- two utterances per workgroup, linear domain -- and one layout pass; utterances whose values leave float32's
 * range (sharp emissions) and every other batch run the item kernel (log domain, one workgroup per utterance).  While the last
 * finished export of the direction handed more than half of its utterances to the item kernel, the next one starts there
 * (every 32nd call tries the linear-domain kernels again; the count is read from pinned memory without synchronising; never
 * during stream capture): the two paths agree within the parity bar, not in the last bits -- mm_batch_set_exact_policy pins the
 * choice (MM_EXACT_F32_FIRST: the linear-domain kernels first, always; MM_EXACT_F64_FIRST: the item kernel alone). */
int mm_alpharecursion_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n,
                          const int32_t *lens, int64_t N, float *out, int64_t out_stride_n, void *stream);
/* beta-recursion(T_hat, C_hat*V_hat) (src/inference.jl:99-110); same layout (state_B).  Log and Tropical
 * batches (the latter is what maxstateposteriors -- docs/src/inference.md:5 -- combines with the tropical alpha). */
int mm_betarecursion_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n,
                         const int32_t *lens, int64_t N, float *out, int64_t out_stride_n, void *stream);

/* maxstateposteriors (documented docs/src/inference.md:5, absent from src/ at this commit: src/MarkovModels.jl:56-57;
 * historical use test/test_algorithms.jl:279-281): the max-marginals of the tropical semiring,
 * mu = alpha (*) beta (/) best -- for every state and frame the weight of the best complete path through it relative
 * to the best path overall (0 on a best path, -inf where no complete path passes, -inf everywhere if the utterance
 * has no path).  MM_TROPICAL batches.  out: device, the layout of mm_alpharecursion_f32 (element (b, n, s) at
 * out[n*out_stride_n + state_offset_b + s], n = 0..N).  Computed on the device: tropical alpha and beta recursions
 * and the combination. */
int mm_maxstateposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n,
                              const int32_t *lens, int64_t N, float *out, int64_t out_stride_n, void *stream);

/* bestpath (documented docs/src/inference.md:5-6, absent from src/ at this
 * commit: src/MarkovModels.jl:56-57; historical use examples/demo.ipynb cell 23).
 * Tropical alpha-recursion (src/inference.jl:62-74 with K = TropicalSemiring)
 * plus back-pointers and an on-device back-trace.  The batch must have been
 * built from MM_TROPICAL FSMs.
 *   path   device int32, element (b, n) at path[b*path_stride_b + n]: 0-based
 *          state at frame n < len_b, -1 for n >= len_b or when no path exists
 *   score  device float[B]: weight of the best path (-inf if none)
 *   bp     optional device int32 (NULL to use internal storage): back-pointers,
 *          element (b, n, s) at bp[n*bp_stride_n + state_offset_b + s], n = 0..N;
 *          bp = lowest source state among the maximisers, -1 if none. */
int mm_viterbi_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens,
                   int64_t N, int32_t *path, int64_t path_stride_b, float *score, int32_t *bp,
                   int64_t bp_stride_n, void *stream);

/* Windowed best paths: the Viterbi recursion of a tropical batch over a WINDOW of the audio, which starts from a carried vector
 * instead of the FSM's initial vector and ends open (on the best real state: the audio goes on) or in the phony final state -- and
 * the CONVERGENCE POINT, the last frame through which every surviving path passes: the path up to it can never change, whatever
 * audio follows.  The tropical counterpart of mm_windowposteriors_f32 for online alignment, keyword spotting, endpointing on the
 * best path and live captioning, where mm_viterbi_f32 would re-run the whole prefix at every chunk.  For utterance b the extended
 * system, lhs = C_hat * expand(V_b) and len = len_b are exactly those of mm_viterbi_f32; natural log; frames counted from 1 here
 * and from 0 in the arrays, f the phony final state:
 *
 *   start(j)   = alpha_hat(j) (state_in == NULL)  or  state_in_b(j)   for real j;  start(f) = -inf
 *   d_1(j)     = start(j) + lhs_1(j)
 *   d_n(j)     = (max_i d_{n-1}(i) + T_hat(i,j)) + lhs_n(j),  bp_n(j) = the LOWEST i among the maximisers (-1 if the max is -inf)
 *   e(i)       = d_len(i)                     closed_b == 0 (the audio goes on)
 *   e(i)       = d_len(i) + T_hat(i,f)        closed_b != 0 (the audio ends at frame len)
 *   score      = max_i e(i);  s_len = the lowest maximiser;  s_n = bp_{n+1}(s_{n+1});   path(n) = s_n, 0-based, -1 for n >= len
 *   A_len      = { real i : e(i) > -inf };   A_n = { bp_{n+1}(j) : j in A_{n+1} }      the states surviving paths pass at frame n
 *   converged  = the largest n in 1..len with |A_n| = 1;  0 if there is none
 *   c          = clamp(commit_b, 0, len)   (commit == NULL: len when commit_converged == 0, else 0);
 *                commit_converged != 0:  c = max(c, converged)
 *   m_c        = max_{j real} d_c(j)
 *   state_out(j) = (max_i d_c(i) + T_hat(i,j)) - m_c      for ALL j, f included
 *   mcommit    = m_c;   ncommit = c
 *
 *   V, lens, N   as mm_viterbi_f32
 *   state_in, state_out   layout and aliasing rule of mm_filterposteriors_f32: they may be one buffer.  state_out NULL: not written
 *   closed       device int32[B]; NULL: every utterance is open
 *   commit       device int32[B]; NULL: see c above
 *   mcommit      device float[B], ncommit, converged device int32[B], out (each NULL: not written)
 *   path, score  as mm_viterbi_f32's.  NULL: MM_ERR_INVALID.  path_stride_b < N: MM_ERR_DIM
 * Argument errors that need no device are reported before the NULL-batch check.  MM_TROPICAL batches only: Log and ProbSemiring
 * batches return MM_ERR_UNSUPPORTED.
 * Arithmetic: the float32 operations of mm_viterbi_f32's item kernel in the same order -- one add per arc, a max, one add of the
 * emission -- and one subtraction for state_out.  No multiply, nothing that can contract.
 * Conventions: len = 0 gives path all -1, score = -inf, converged = 0, ncommit = 0, mcommit = 0 and state_out = a copy of the start
 * vector (state_in == NULL: alpha_hat).  c = 0 with len > 0 gives the same copy and mcommit = 0.  A window without a path (score =
 * -inf) has path all -1 and converged = 0; its state_out and mcommit are still the prefix's values when m_c > -inf, else -inf
 * everywhere.  Nothing is NaN.
 * Consequences: (a) closed with state_in == NULL: path and score are those of mm_viterbi_f32, bit for bit.  (b) FINALITY: an open
 * window of len frames and any longer window from the same start, open or closed, that has a path: the two paths agree on frames
 * 1..converged, bit for bit (the forward pass is causal and the back-pointers of the first len frames are identical).  (c)
 * RE-WINDOWING: a window over frames 1..M with commit c and a second window over frames c+1..M with state_in = the first window's
 * state_out and the same closed: in exact arithmetic the second has the first's path on frames c+1..M and its score = the first's
 * score - mcommit; in float32 this holds bit for bit whenever every sum is exactly representable (weights and emissions that are
 * multiples of 1/16 of moderate size, say).  When c <= converged, the committed frames of successive windows concatenate to the
 * best path of the whole audio.  (d) a constant added to every emission of a frame changes no path and no converged, and moves
 * score by that constant.  (e) no atomics whose order matters: a repeated call returns the same bits.
 * Runs on the item form of every FSM of every tropical batch, one workgroup per utterance: mm_vitwindow_fwd_kernel<NI,lds|global>
 * (mm_viterbi_f32's item kernel from the carried start; per frame it stores the back-pointer row, the row of PRE-EMISSION maxima
 * -- state_out of whatever commit frame the second kernel arrives at is that row minus m_c, so no arc pass is repeated -- and the
 * frame's maximum over the real states) and mm_vitwindow_trace_kernel (the best path by one lane; the surviving set as byte flags,
 * propagated through the back-pointer rows until one state is left: O((len - converged) * S) work).  Workspace, grown by the call
 * and covered by mm_batch_workspace_bytes: int32 and float32 rows (sum_b S1p_b) x (N + 1) each, float32 B x (N + 2), int32 B.
 * Stream contract of mm_arcposteriors_f32: launches on `stream` only, no host synchronisation; it can be captured in a hipGraph
 * once a first call has put the batch's item forms on the device and sized the workspace (a capture before that returns
 * MM_ERR_INVALID). */
int mm_viterbiwindow_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                         const float *state_in, const int32_t *closed, const int32_t *commit, int commit_converged, float *state_out,
                         float *mcommit, int32_t *ncommit, int32_t *path, int64_t path_stride_b, float *score, int32_t *converged,
                         void *stream);

/* Best paths that report arc classes, under per-frame arc-class scores: the tropical twin of mm_scoredposteriors_f32.  What a
 * decoder or an aligner hands on is the sequence of labels with their times -- words, phones, transition-ids, boundaries: things
 * that sit on ARCS -- and the states do not determine it, because parallel entries between the same two states are allowed and the
 * back-pointers of mm_viterbi_f32 keep the source state alone.  A plan (mm_batch_set_path_classes) gives every stored entry
 * k = (i_k -> j_k) of an FSM's T_hat -- the phony-final column and the phony self-loop included, in the order mm_arcposteriors_f32
 * reports them -- a class cls[k] in {-1, 0, ..., C-1}.  For utterance b of length len, frames 1-based in the formulas and t 0-based
 * as in mm_arcclassposteriors_f32, f the phony final state:
 *
 *   d_1(j)  = alpha_hat(j) + lhs_1(j)
 *   x_n(k)  = (T_hat[k] + d_{n-1}(i_k)) + U[b, n-2, cls k]     one float32 add, then one more; class -1 and the
 *                                                              phony self-loop: no second add.  U == NULL: no second add at all
 *   d_n(j)  = (max_{k into j} x_n(k)) + lhs_n(j)                n = 2 .. len+1
 *   bp_n(j) = source state, bc_n(j) = class of THE maximiser: the lowest source state; among parallel maximisers from that
 *             state the lowest class id, with -1 ordered behind every class.  (-1, -1) if the max is -inf
 *   score   = d_{len+1}(f);  s_{len+1} = f;  s_n = bp_{n+1}(s_{n+1});  path(n-1) = s_n;
 *   classes(t) = bc_{t+2}(s_{t+2}),  t = 0 .. len-1      (t = len-1: the arc into the phony final state)
 *
 * path[b, n] for n >= len and classes[b, t] for t >= len are -1.  An utterance without a path (len = 0 included) has path and classes
 * all -1 and score = -inf.  U is finite or -inf; rows t >= len of U are never read; nothing is NaN.  Float adds and a max only,
 * nothing that can contract; natural log throughout (the score row is staged unscaled, as the tropical kernels stage emissions);
 * no atomics: a repeated call returns the same bits.
 * Consequences: (a) with U NULL, path and score are mm_viterbi_f32's, bit for bit, whatever the plan.  (b) With U[b, t, c] = u_c,
 * path and score are those of mm_viterbi_f32 on the FSM with weights w_k + u_cls[k] -- bit for bit wherever every sum is exact
 * (weights, scores and emissions that are multiples of 1/16 of moderate size).  (c) U = -inf at (t, c) removes the class from that
 * transition: classes[b, t] != c, or the utterance has no path.  (d) score = the float32 sum along the returned path in the
 * recursion's order (exact on such a grid).  (e) Relabelling the classes by an order-preserving map changes `classes` by that map
 * and nothing else.
 *
 * mm_batch_set_path_classes: MM_TROPICAL batches only (others: MM_ERR_UNSUPPORTED; mm_batch_set_arc_classes keeps refusing tropical
 * batches).  Arguments and error codes of mm_batch_set_arc_classes; C > 65534: MM_ERR_UNSUPPORTED.  Host work only: it builds the
 * 16-bit class plane of the forward item form of every distinct (FSM, class array) -- an unclassified entry, the phony self-loop
 * and every padding slot carry the id C --; the first mm_classpath_f32 call behind it puts the planes on the device in one
 * allocation and one copy (never during a stream capture: MM_ERR_INVALID).  Calling it again replaces the plan.
 * mm_batch_path_class_info: C = the classes of the current plan (0: none), cap = the largest C whose two score rows fit the LDS
 * behind the forward kernel's plan (either pointer may be NULL).
 *
 *   V, lens, N   as mm_viterbi_f32
 *   U            device, element (b, t, c) at U[b*u_stride_b + t*u_stride_n + c*u_stride_c], natural log; strides checked as
 *                mm_scoredposteriors_f32 checks them (MM_ERR_DIM).  NULL: no scores
 *   path, score  as mm_viterbi_f32's.  NULL: MM_ERR_INVALID.  path_stride_b < N: MM_ERR_DIM
 *   classes      device int32, out, element (b, t) at classes[b*classes_stride_b + t]; classes_stride_b < N: MM_ERR_DIM.  NULL: not
 *                written -- a plan is then required only if U is given
 * U or classes without a plan: MM_ERR_INVALID.  U with more classes than the cap: MM_ERR_UNSUPPORTED, the message names the cap.
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * Runs on the item form of every FSM, one workgroup per utterance: mm_classpath_fwd_kernel<NI,lds|global> (mm_viterbiwindow_f32's
 * step from the FSM's own start; the score row of a transition is C + 1 floats in LDS, double-buffered and fetched one step ahead,
 * its slot [C] holds 0; the maximiser's class travels with its source through the lane and group reduction; per frame the
 * back-pointer row and a 16-bit class row leave for the workspace) and mm_classpath_trace_kernel (one lane per utterance follows
 * the back-pointers from f).  Workspace, grown by the call and NOT covered by mm_batch_workspace_bytes (mm_batch_reserve does not
 * size it: a first call does): int32 and 16-bit rows (sum_b S1p_b) x (N + 1) each.  Stream contract of the arc entries: launches
 * on `stream` only, no host synchronisation; capturable in a hipGraph after a first call has put the item forms and the planes on
 * the device and sized the workspace (a capture before that returns MM_ERR_INVALID); a replay after U was overwritten in place
 * follows the new scores. */
int mm_batch_set_path_classes(mm_batch_t batch, const int32_t *cls, const int64_t *offsets, int32_t C);
int mm_batch_path_class_info(mm_batch_t batch, int32_t *C, int64_t *cap);
int mm_classpath_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                     const float *U, int64_t u_stride_b, int64_t u_stride_n, int64_t u_stride_c, int32_t *path, int64_t path_stride_b,
                     int32_t *classes, int64_t classes_stride_b, float *score, void *stream);

/* Beam-pruned best-path lattices (MM_TROPICAL batches): for every utterance and transition, the stored entries of T_hat that lie on
 * some complete path whose weight is within beam_b of the best path's, with their through-scores -- the pruned hypothesis space that
 * N-best lists, confidences, rescoring by a second model and lattice-based training read off on the host.  Conventions of
 * mm_classpath_f32: lhs = C_hat . expand(V_b), frames 1-based in the formulas, transition t 0-based between frames t+1 and t+2
 * (t = len-1: the arc into the phony final state f), the stored entries k = (i_k -> j_k) in the order mm_arcposteriors_f32 reports
 * them (parallel entries between two states are entries of their own).
 *
 *   alpha_n, beta_n   the tropical recursions mm_alpharecursion_f32 / mm_betarecursion_f32 export (beta_n excludes frame n's emission)
 *   best    = alpha_{N+1}(f)                                                       (mm_viterbi_f32's score)
 *   x_t(k)  = (alpha_{t+1}(i_k) + T_hat[k]) + (lhs_{t+2}(j_k) + beta_{t+2}(j_k))   three float32 adds, in this grouping
 *   s_t(k)  = x_t(k) - best                                                        one float32 subtraction
 *   keep (t, k)  iff  t < len,  k is not the phony self-loop,  best > -inf,  beam_b >= 0,  x_t(k) > -inf,  s_t(k) >= -beam_b
 *
 * The records of all (b, t) are concatenated in row-major (b, t) order, within one (b, t) sorted by ascending k; record r holds
 * arc[r] = k and score[r] = s_t(k).  The first record of (b, t) is the exclusive prefix sum of `counts` (the entry returns no
 * offsets: a cumsum of counts gives them).  An utterance without a path (len = 0 included) has all counts 0 and best = -inf; a
 * negative or NaN beam keeps nothing, +inf keeps every arc with a finite through-score; nothing is NaN.  No atomics: a repeated
 * call returns the same bits.
 * Where every sum is exact -- weights, emissions and beams that are multiples of 1/16 of moderate size -- every kept / dropped
 * decision and every score is exact.  Otherwise s carries the float32 rounding of the sums behind it, about
 * (N + 3) * 2^-24 * max|alpha|: an arc whose true score lies that close to -beam may fall on either side, and a beam of 0 is then
 * NOT meaningful (the arcs of the best path itself score a rounding error below or above 0).
 * Consequences: (a) the arcs mm_classpath_f32 / mm_viterbi_f32 take are kept for any beam >= 0, with score 0, on exact inputs.
 * (b) beam = 0 on exact inputs keeps exactly the arcs of all tied best paths.  (c) The kept sets are nested in the beam.  (d) For
 * every state j and frame n = t+2 with mu_n(j) >= -beam, mu being mm_maxstateposteriors_f32's, the maximum of s_t(k) over the kept
 * arcs into j equals mu_n(j) (exactly on exact inputs).  (e) The result does not depend on cap: with cap < total the first cap
 * records are those of the full call.
 *
 *   V, lens, N   as mm_viterbi_f32
 *   beam         device float[B], natural log.  NULL: MM_ERR_INVALID
 *   counts       device int32, out, element (b, t) at counts[b*counts_stride_b + t]: the kept arcs of transition t, 0 for t >= len.
 *                Always written.  NULL: MM_ERR_INVALID.  counts_stride_b < N: MM_ERR_DIM
 *   total        device int64[1], out: the sum of counts.  Always written.  NULL: MM_ERR_INVALID
 *   best         device float[B], out.  NULL: not written
 *   arc, score   device int32 / float32, out, `cap` records each (cap: a host value).  Records r >= cap are not written and nothing
 *                at or behind arc[cap] / score[cap] is touched.  arc == NULL with cap == 0 is the count-only call; arc and score
 *                are both given or both NULL, cap >= 0, and cap == 0 with arc NULL: MM_ERR_INVALID otherwise
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * Order of a call: the two recursions (mm_tropical_kernel, mm_log_kernel<MODE_BETA, .., TROP>, as mm_maxstateposteriors_f32 runs
 * them), mm_pick_final_kernel, then mm_lattice_prune_kernel<lds|global, count> (one workgroup of 256 threads per (b, t): the rows
 * alpha_{t+1} and lhs_{t+2} + beta_{t+2} staged in LDS, or gathered from global memory where 2 S1p floats exceed it; the arc table
 * -- source, destination and weight planes of every distinct FSM in the caller's entry order -- streamed in 16-byte loads; compaction
 * in entry order by ballot and mbcnt per wave, a scan of the wave counts, a running base), mm_lattice_scan_kernel (offsets and
 * total, one workgroup, fixed order) and the same prune kernel in its write mode, skipped for the count-only call.  Both modes
 * decide by one predicate function.
 * Workspace, grown by the call and NOT covered by mm_batch_workspace_bytes (mm_batch_reserve does not size it: a first call does):
 * two float32 rows (sum_b S1_b) x (N + 1), int64 [B*N + 1], float32 [B].  Stream contract of the arc entries: launches on `stream`
 * only, no host synchronisation; capturable in a hipGraph after a first call has put the item forms and the arc table on the device
 * (one allocation, one copy) and sized the workspace (a capture before that returns MM_ERR_INVALID); a replay after V and beam were
 * overwritten in place follows them. */
int mm_lattice_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                   const float *beam, int32_t *counts, int64_t counts_stride_b, int64_t *total, float *best, int32_t *arc,
                   float *score, int64_t cap, void *stream);

/* Lattice posteriors (MM_TROPICAL batches): the log-semiring forward-backward over the records of a lattice of mm_lattice_f32 (or a
 * subset of one), under THIS call's emissions V -- a second model's, or the first one's at another acoustic scale -- and an optional
 * extra score per record (a language-model or pronunciation rescoring, a boosting term).  One call for the whole batch returns the
 * log posterior of every record (arc confidences; what posterior pruning and MBR decoding over the lattice read), the lattice's
 * log-sum per utterance and the pdf occupancies, its gradient against V: lattice-based MMI as an autograd function.
 * Conventions of mm_lattice_f32: the stored entries k = (i_k -> j_k) of T_hat in the caller's order, transitions t 0-based
 * (t = len-1: the arcs into the phony final state f), record r of cell (b, t) is arc[r] = k with offsets[b*N + t] <= r <
 * offsets[b*N + t + 1]; pdf(s) a state's pdf; frames 0-based below.  A lattice path of utterance b is one record r_0 .. r_{len-1}
 * per transition with j(r_t) = i(r_{t+1}) and j(r_{len-1}) = f; it weighs
 *
 *   W(path) = alpha_hat(i(r_0)) + V[b, 0, pdf(i(r_0))]
 *           + sum_{t < len-1} ( T_hat[arc[r_t]] + extra[r_t] + V[b, t+1, pdf(j(r_t))] )
 *           + T_hat[arc[r_{len-1}]] + extra[r_{len-1}]
 *   logz[b]        = log sum_path exp W(path)                        (-inf: no path; len = 0 included)
 *   post[r]        = log sum_{path through r} exp W(path) - logz[b]  (<= 0; -inf: no path through r, or logz = -inf)
 *   gamma[b, n, p] = sum_{r in cell (b, n), pdf(i(r)) = p} exp(post[r])   for n < len, 0 for n >= len and where logz = -inf
 *
 * alpha_hat and T_hat are the weights the tropical batch holds; extra == NULL means 0.  gamma = d logz / d V, exp(post) =
 * d logz / d extra; for every t < len of an utterance with a path the posteriors of the cell sum to 1.  Nothing is NaN for inputs
 * that are finite or -inf.  Where every cell holds one record and the inputs are multiples of 1/16 -- a beam of 0 with a unique best
 * path, extra NULL, the lattice's own V -- post is exactly 0, gamma exactly 0 / 1 and logz mm_lattice_f32's best, bit for bit.
 *
 *   V, lens, N   as mm_lattice_f32; lens and N are those of the lattice call that produced `offsets`
 *   offsets      device int64[B*N + 1], the exclusive prefix sum of the lattice's counts in row-major (b, t) order.  NULL: MM_ERR_INVALID
 *   arc          device int32[nrec].  Within a cell the records ascend in k, as mm_lattice_f32 writes them; a subset of a lattice
 *                keeps that.  NULL with nrec > 0: MM_ERR_INVALID
 *   nrec         a host value >= 0: the records arc / extra / post hold.  Negative: MM_ERR_INVALID
 *   extra        device float32[nrec], or NULL
 *   post         device float32[nrec], out.  NULL with nrec > 0: MM_ERR_INVALID
 *   logz         device float32[B], out.  NULL: MM_ERR_INVALID
 *   gamma        device float32, out, or NULL (not computed): element (b, n, p) at gamma[b*gamma_stride_b + n*gamma_stride_n + p], all N
 *                rows of every utterance written.  gamma_stride_n < P or gamma_stride_b < N*gamma_stride_n: MM_ERR_DIM
 * Memory safety does not depend on the contents of the device arrays: a record whose k is outside [0, nnz_b) or is the phony
 * self-loop is dead (its post is -inf and it contributes nothing); records at or behind nrec are never read or written (a lattice cut
 * by mm_lattice_f32's cap goes in as it is: the result is that of the truncated lattice); offsets that decrease, are negative or reach
 * behind nrec are clamped into [0, nrec] and made non-decreasing; lens are clamped into [0, N].  The records of cells at or behind
 * len receive -inf; records no cell covers are not written.
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * The state vectors live in LDS, 16 bytes per state: an FSM of more than about 10 200 states (padded) returns MM_ERR_UNSUPPORTED
 * with the limit in the message; mm_batch_kernels(.., 19, ..) names it.
 * Order of a call: mm_latpost_fb_kernel (one workgroup per utterance, serial over its transitions; per step three passes over the
 * records of the cell: gather source, destination and weight through arc[r] from mm_lattice_f32's arc table, the emission of the
 * destination and extra[r]; per target state an integer LDS maximum on an order-preserving code of the float, then the sum of
 * exp(x - max) in 64-bit fixed point, rint(. * 2^40), by 64-bit integer LDS adds; the vectors relative to a per-step maximum that
 * is accumulated in double.  The forward value of a record is kept in post[r]; the backward pass overwrites it with
 * y_r - LSE_cell(y), the cell's own log-sum -- logz is never subtracted from anything), then, when gamma is given,
 * mm_latpost_gamma_kernel (one workgroup per (b, n): exp(post) by the source's pdf, the same fixed-point adds).  Integer maxima and
 * integer sums do not depend on the order of arrival: a repeated call returns the same bits.  The terms a sum loses lie below 2^-41
 * of its largest.  The work of a step is proportional to the records of its cell, not to the graph.
 * No workspace.  Stream contract of the arc entries: launches on `stream` only, no host synchronisation; capturable in a hipGraph
 * after a first call of this entry or of mm_lattice_f32 has put the item forms and the arc table on the device (a capture before
 * that returns MM_ERR_INVALID); a replay after V, extra, offsets or arc were overwritten in place follows them. */
int mm_latticeposteriors_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                             const int64_t *offsets, const int32_t *arc, int64_t nrec, const float *extra, float *post, float *logz,
                             float *gamma, int64_t gamma_stride_b, int64_t gamma_stride_n, void *stream);

/* Lattice expected cost (MM_TROPICAL batches): the expectation of a cost that adds up along a path, over the paths of a lattice of
 * mm_lattice_f32 weighed as mm_latticeposteriors_f32 weighs them, and its gradient -- the lattice form of mm_expectedcost_f32.  With
 * cost[r] minus the phone or word accuracy of the record it is MPE / MWE (Povey 2003), with minus [pdf of the record's source = the
 * alignment's pdf] state-level MBR; the loss of MBR decoding over a lattice is the same expectation.  Records, cells, offsets, arc,
 * extra, W(path), post, logz and gamma are exactly those of mm_latticeposteriors_f32, i(r) / j(r) the source / destination of a record:
 *
 *   A(path)      = sum_{t < len} cost[r_t]                                   one record per transition, as in W(path)
 *   risk[b]      = sum_path exp(W(path) - logz[b]) * A(path)
 *   diff[r]      = exp(post[r]) * (E[A | path through r] - risk[b])          = d risk / d extra[r]   (Povey's gamma^MPE of the arc)
 *   grad[b,n,p]  = sum_{r in cell (b, n), pdf(i(r)) = p} diff[r]             = d risk / d V[b,n,p];  exact 0 for n >= len
 *   d risk / d cost[r] = exp(post[r])
 *   E[A | through r] = ca_t(i(r)) + cost[r] + cb_{t+1}(j(r))
 *     ca_0(.) = 0        ca_{t+1}(j) = sum_{r in cell t, j(r) = j} exp(x_r - a_{t+1}(j)) * (ca_t(i(r)) + cost[r])
 *     cb_len(f) = 0      cb_t(i)     = sum_{r in cell t, i(r) = i} exp(z_r - b_t(i))     * (cost[r] + cb_{t+1}(j(r)))
 *   risk[b] = ca_len(f)
 *
 * x_r and z_r are the forward and backward values of a record in mm_latticeposteriors_f32's recursions (a_t(i(r)) resp. b_{t+1}(j(r))
 * plus the record's own weight); both sums are convex combinations plus an addition.  Identities: post, logz and gamma are bit for bit
 * those of mm_latticeposteriors_f32 on the same inputs; every cell's diff sums to 0 and every row of grad sums to 0; risk =
 * sum_r exp(post[r]) cost[r]; a cost that is constant within each cell (c_t) gives risk = sum_{t < len} c_t and diff = grad = 0;
 * where every cell holds one record and the costs are multiples of 1/16, risk is the exact sum and diff and grad are exactly 0.
 *
 *   batch .. extra   as mm_latticeposteriors_f32
 *   cost         device float32[nrec]; finite on the live records of cells t < len (a non-finite cost leaves that utterance's outputs
 *                unspecified and touches no other utterance).  NULL with nrec > 0: MM_ERR_INVALID
 *   risk         device float32[B], out.  NULL: MM_ERR_INVALID
 *   diff         device float32[nrec], out.  NULL with nrec > 0: MM_ERR_INVALID
 *   post, logz   as mm_latticeposteriors_f32, required
 *   grad, gamma  device float32, out, each or both NULL (not computed): element (b, n, p) at [b*stride_b + n*stride_n + p] of either,
 *                one pair of strides for both, all N rows of every utterance written.  stride_n < P or stride_b < N*stride_n: MM_ERR_DIM
 * An utterance without a path (len = 0 included) gets risk 0, diff 0, grad 0, gamma 0 and logz -inf.  Dead records and the records of
 * cells at or behind len get diff 0 and post -inf; records no cell covers are not written.  Nothing is NaN for inputs that are finite
 * or -inf.  Memory safety does not depend on the contents of the device arrays, by mm_latticeposteriors_f32's checks: dead records,
 * clamped and monotone offsets, lens clamped into [0, N].
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * The state vectors live in LDS, 28 bytes per state (the 16 of the posteriors, a signed 64-bit cost sum and a float): an FSM of more
 * than about 5 800 states (padded) returns MM_ERR_UNSUPPORTED with the limit in the message; mm_batch_kernels(.., 20, ..) names it.
 * Order of a call: mm_latcost_fb_kernel -- mm_latpost_fb_kernel's code with the cost part compiled in: the same three passes per step.
 * A state's ca (forward; cb backward) is kept relative to the largest value of the step that finished it, and forward those maxima
 * accumulate in a double that ends as the risk, so the float32 values stay near zero however long the utterance is.  Per step the
 * block's maximum vmax of |v_r|, v_r = centred ca(i(r)) + cost[r], is taken beside the first pass; the second adds
 * rint(exp(x_r - max) * (v_r / vmax) * 2^40) as a signed 64-bit integer per target state; the thread that finishes a state sets its
 * value to (cost sum / sum) * vmax.  diff[r] holds v_r between the passes.  Backward, u_r = v_r + centred cb(j(r)) is the cost of
 * the paths through r up to a constant of the cell; the cell's posterior mean u_bar of u is summed in the same fixed point and
 * diff[r] = exp(post[r]) * (u_r - u_bar), so no offset of the forward pass is needed.  Then, when grad or gamma is given,
 * mm_latcost_grad_kernel (one workgroup per (b, n): diff by the source's pdf as signed fixed point relative to the cell's largest
 * |diff|, exp(post) as mm_latpost_gamma_kernel sums it).  Integer maxima and integer sums: a repeated call returns the same bits in
 * every output.  No workspace.  Stream contract and graph capture: those of mm_latticeposteriors_f32 (a first call of this entry
 * counts); a replay after V, extra, cost, offsets or arc were overwritten in place follows them. */
int mm_latticecost_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                       const int64_t *offsets, const int32_t *arc, int64_t nrec, const float *extra, const float *cost, float *risk,
                       float *diff, float *post, float *logz, float *grad, float *gamma, int64_t stride_b, int64_t stride_n, void *stream);

/* Lattice best paths (MM_TROPICAL batches): the tropical twin of mm_latticeposteriors_f32 -- over the records of a lattice of
 * mm_lattice_f32 (or a subset of one), under THIS call's emissions V and an optional extra score per record, the weight of the best
 * path, how far below it the best path through every record lies, and the best path itself as records and as states.  It is the step
 * behind a rescoring: the new one-best, the through-scores that re-prune the lattice to a narrower beam under the new scores, the
 * target of a perceptron or max-margin loss.  Unlike the route over a lattice's graph it keeps parallel entries apart (it says WHICH
 * record won) and takes a score per record.  Records, cells, offsets, arc, extra, dead records and W(path) are exactly those of
 * mm_latticeposteriors_f32, i(r) / j(r) the source / destination of a record, f the phony final state.  In float32, in this
 * grouping -- adds, one subtraction and a maximum, so nothing can contract:
 *
 *   wz_r        = (T_hat[arc[r]] + extra[r]) + e_{t+2}(j(r))     e_n(j): V[b, n-1, pdf(j)] for n <= len, 0 for j = f behind len,
 *                                                                -inf otherwise; extra NULL: + 0
 *   a_0(s)      = alpha_hat(s) + e_1(s)
 *   f_r         = a_t(i(r)) + wz_r                               r in cell t
 *   a_{t+1}(j)  = max_{r in cell t, j(r) = j} f_r
 *   best[b]     = a_len(f)                                       (-inf: no path, len = 0 included)
 *   b_len(f) = 0;   b_t(i) = max_{r in cell t, i(r) = i} (wz_r + b_{t+1}(j(r)))
 *   score[r]    = (f_r + b_{t+1}(j(r))) - best[b]                -inf: no path through r, r dead, best = -inf, cell at or behind len
 *   r_{len-1}   = the LOWEST live r of cell len-1 with j(r) = f and f_r = best
 *   r_t         = the LOWEST live r of cell t with j(r) = i(r_{t+1}) and f_r = a_{t+1}(i(r_{t+1}))
 *   rec[b, t]   = r_t, an index into arc;  path[b, t] = i(r_t), mm_viterbi_f32's convention (the 0-based state at frame t);
 *                 both -1 for t >= len and for an utterance without a path
 *
 * The maximum and the equality are those of the floats' order with -0 below +0.  Consequences: (a) best is bit for bit the float32
 * sum along the returned path in the recursion's order, a_0(path[b, 0]) then + wz of rec[b, 0], rec[b, 1], .., for any input: the
 * maximum only selects among computed values.  (b) With extra NULL, the lattice's own V and exact inputs (multiples of 1/16 of
 * moderate size) best and score are mm_lattice_f32's, bit for bit.  (c) On such inputs score[rec[b, t]] == 0 and every cell t < len
 * of an utterance with a path has maximum 0.  (d) Where the best path is unique, path is mm_viterbi_f32's.  (e) extra[r] = -inf
 * removes record r: rec never names it, or the utterance has no path.  (f) best <= logz of mm_latticeposteriors_f32 on the same
 * inputs.  Nothing is NaN for inputs that are finite or -inf.  Integer maxima: a repeated call returns the same bits.
 *
 *   batch .. extra   as mm_latticeposteriors_f32
 *   best         device float32[B], out.  NULL: MM_ERR_INVALID
 *   score        device float32[nrec], out.  NULL with nrec > 0: MM_ERR_INVALID.  Between the passes it holds f_r
 *   rec          device int64, out, or NULL (not computed): element (b, t) at rec[b*rec_stride_b + t], all N of every utterance
 *                written.  rec_stride_b < N: MM_ERR_DIM
 *   path         device int32, out, or NULL (not computed): element (b, t) at path[b*path_stride_b + t], likewise.
 *                path_stride_b < N: MM_ERR_DIM
 * Memory safety does not depend on the contents of the device arrays, by mm_latticeposteriors_f32's checks: a record whose entry is
 * outside [0, nnz_b) or is the phony self-loop is dead, cells are clamped into [0, nrec] and made non-decreasing, lens into [0, N];
 * records no cell covers are not written.
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * The state vectors live in LDS, 12 bytes per state: an FSM of more than about 13 600 states (padded) returns MM_ERR_UNSUPPORTED
 * with the limit in the message; mm_batch_kernels(.., 21, ..) names it.
 * Order of a call: mm_latbest_kernel alone (one workgroup per utterance, serial over its transitions, mm_latpost_fb_kernel's
 * organisation with one pass and one barrier per step: three state vectors rotate -- read, accumulate by integer LDS maximum on the
 * order-preserving code of the float, empty.  The forward pass parks f_r in score[r]; the backward pass overwrites it, and carries
 * the trace: per step the 64-bit maximum of (code of f_r, 2^32 - 1 - place in the cell) over the records into the path's current
 * state, by a wave reduction and one LDS atomic, so no back-pointer is ever stored; a doctored cell of 2^32 records or more falls
 * back to an exact 64-bit minimum).  The work of a step is proportional to the records of its cell, not to the graph.
 * No workspace.  Stream contract and graph capture: those of mm_latticeposteriors_f32 (a first call of any lattice entry puts the
 * item forms and the arc table on the device); a replay after V, extra, offsets or arc were overwritten in place follows them. */
int mm_latticebest_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                       const int64_t *offsets, const int32_t *arc, int64_t nrec, const float *extra, float *best, float *score,
                       int64_t *rec, int64_t rec_stride_b, int32_t *path, int64_t path_stride_b, void *stream);

/* Lattice path sampling (MM_TROPICAL batches): nsamples lattice paths per utterance, drawn independently from the posterior of a
 * lattice of mm_lattice_f32 (or a subset of one) under THIS call's emissions V and an optional extra score per record.  It is what a
 * loss needs whose cost does NOT add up along a path -- the expected word error rate, an edit distance (Shannon, "Optimizing expected
 * word error rate via sampling for speech recognition", Interspeech 2017; Prabhavalkar et al., "Minimum word error rate training for
 * attention-based sequence-to-sequence models", ICASSP 2018) -- and sampled minimum-Bayes-risk decoding, and diverse pseudo-labels.
 * Unlike mm_samplepaths_f32 it draws RECORD sequences: parallel entries between two states are separate outcomes, and every record
 * has its own score.  Records, cells, offsets, arc, extra, dead records, lens, W(path) and logz are exactly those of
 * mm_latticeposteriors_f32, i(r) / j(r) the source / destination of a record, f the phony final state:
 *
 *   P(sample k of utterance b = path) = exp(W(path) - logz[b])          path = r_0 .. r_{len-1}, one record per transition
 *   x_r         = a_t(i(r)) + wz_r - c_t                                 r in cell t: the value mm_latticeposteriors_f32's forward pass
 *                                                                        has for the record, wz_r = (T_hat[arc[r]] + extra[r]) + e_{t+2}(j(r))
 *                                                                        in float32, c_t ONE constant per cell (the pass's running offset)
 *   u_r         = unit_open(first word of Philox-4x32-10(key = seed's low and high 32 bits; counter = (b, k, t, place of r in its cell)))
 *                 unit_open(w) = ((w >> 9) + 1/2) / 2^23, mm_samplepaths_f32's generator and its split of the seed
 *   g_r         = -logf(-logf(u_r))                                      a Gumbel variate, float32, the accurate logarithm
 *   key_r       = x_r + g_r                                              float32
 *   cur_{len-1} = f;   r_t = the live record r of cell t with j(r) = cur_t and x_r > -inf whose key_r is greatest, among equal keys the
 *                 one at the LOWEST place of the cell;   cur_{t-1} = i(r_t)
 *   rec[b, k, t]  = r_t, an index into arc;   path[b, k, t] = i(r_t), mm_viterbi_f32's convention (the 0-based state at frame t)
 *   logprob[b, k] = W(path) - logz[b],  W in float64: the float32 wz of r_{len-1}, r_{len-2}, .., r_0 added in that order, then the
 *                   float32 alpha_hat(i(r_0)) + V[b, 0, pdf(i(r_0))]; the difference with logz[b] in float64, rounded once
 *
 * The maximum of x_r + Gumbel noise over the records into a state is a draw with probability proportional to exp(x_r) (the Gumbel-max
 * trick); exp(x_r) over the records into cur_t is the posterior of r_t given the rest of the path behind it, and c_t, common to the
 * cell, cancels.  Consequences: (a) a sample is a function of (lattice, V, extra, lens, seed, b, k) alone: not of nsamples, the
 * thread count, the stream or earlier calls; the first K' samples of a call with nsamples > K' are the samples of a call with K'; a
 * repeated call returns the same bits.  (b) The counter holds the POSITION b, not the utterance's content: two equal utterances of a
 * batch get different samples.  (c) A record with x_r = -inf is never drawn, whatever u: a dead record, extra[r] = -inf, a record
 * with no path into its source.  (d) A chosen record has a finite x_r, hence a finite-x record into its source one cell earlier: a
 * chain of an utterance with a path never dies.  (e) Discretisation: u takes 2^23 values, so g takes 2^23 values in about
 * [-2.81, 16.64]; the Gumbel mass outside that range is about 6e-8 on either side, which bounds the bias of a decision's
 * probabilities at that order, beside the float32 rounding of x and g.  (f) Where every cell holds one live record -- a beam of 0 with
 * a unique best path -- every sample is that path, and on inputs that are multiples of 1/16 logprob is exactly 0.  (g) The key's low
 * word holds 2^32 - 1 - place: a record at place >= 2^32 - 1 of a doctored cell of that many records is passed over, never drawn;
 * should that leave a sample without a candidate, its remaining entries are -1 and its logprob -inf.
 *
 *   batch .. extra   as mm_latticeposteriors_f32
 *   nsamples     a host value >= 1 (MM_ERR_INVALID otherwise); more than 64 * 65535: MM_ERR_UNSUPPORTED
 *   seed         any value; its low and high 32 bits are the generator's key
 *   fwd          device float32[nrec], out: a per-record buffer of the caller's.  NULL with nrec > 0: MM_ERR_INVALID.  On return fwd[r]
 *                = x_r, that is the record's forward value up to one constant per cell; -inf for a dead record, a record with no path
 *                into its source, the records of cells at or behind len and every record of an utterance without a path
 *   rec          device int64, out, or NULL: element (b, k, t) at rec[b*rec_stride_b + k*rec_stride_k + t].  rec_stride_k < N or
 *                rec_stride_b < nsamples*rec_stride_k: MM_ERR_DIM
 *   path         device int32, out, or NULL: element (b, k, t) at path[b*path_stride_b + k*path_stride_k + t]; the same rule for its
 *                strides.  rec and path both NULL: MM_ERR_INVALID.  All N entries of every (b, k) are written: -1 for t >= len, and
 *                everywhere for an utterance without a path
 *   logprob      device float32, out, or NULL (not computed): element (b, k) at logprob[b*lp_stride_b + k]; -inf without a path.
 *                lp_stride_b < nsamples: MM_ERR_DIM
 *   logz         device float32[B], out: mm_latticeposteriors_f32's logz, bit for bit.  NULL: MM_ERR_INVALID
 * Memory safety does not depend on the contents of the device arrays, by mm_latticeposteriors_f32's checks: a record whose entry is
 * outside [0, nnz_b) or is the phony self-loop is dead, cells are clamped into [0, nrec] and made non-decreasing, lens into [0, N];
 * records no cell covers are not written.
 * Log and ProbSemiring batches: MM_ERR_UNSUPPORTED.  Argument errors that need no device are reported before the NULL-batch check.
 * The state vectors of the forward pass live in LDS, 16 bytes per state: an FSM of more than about 10 200 states (padded) returns
 * MM_ERR_UNSUPPORTED with the limit in the message; mm_batch_kernels(.., 22, ..) names it.
 * Order of a call: mm_latsample_fwd_kernel (mm_latpost_fb_kernel's forward pass, the same code: it ends behind logz), then
 * mm_latsample_kernel on a grid of (B, ceil(nsamples / 64)): a workgroup draws 64 samples of one utterance, serial over the
 * transitions backwards.  LDS holds a 64-bit mask per state -- bit q: sample q of the chunk sits there -- and two alternating sets of
 * 64 key slots.  Per step every thread takes records of the cell, reads the mask of the destination and, for every set bit with a
 * finite fwd[r], maximises the 64-bit (order-preserving code of key_r, 2^32 - 1 - place) in that sample's slot by an integer LDS
 * atomic; behind a barrier lane q of the first wave reads its winner, stores rec / path, adds wz to its float64 weight and moves
 * its bit to the source's mask; a second barrier ends the step.  Integer maxima do not depend on the order of arrival.  The work of a
 * step is the records of its cell plus the candidates of at most 64 states.
 * No workspace.  Stream contract and graph capture: those of mm_latticeposteriors_f32 (a first call of any lattice entry puts the
 * item forms and the arc table on the device); a replay after V, extra, offsets or arc were overwritten in place follows them. */
int mm_latticesample_f32(mm_batch_t batch, const float *V, int64_t v_stride_b, int64_t v_stride_n, const int32_t *lens, int64_t N,
                         const int64_t *offsets, const int32_t *arc, int64_t nrec, const float *extra,
                         int64_t nsamples, int64_t seed, float *fwd,
                         int64_t *rec, int64_t rec_stride_b, int64_t rec_stride_k,
                         int32_t *path, int64_t path_stride_b, int64_t path_stride_k,
                         float *logprob, int64_t lp_stride_b, float *logz, void *stream);

/* totalsum(alpha, T, omega, n) / totalcumsum(alpha, T, omega, n) (src/algorithms.jl:8-29;
 * totalweightsum(fsm, n) = totalcumsum, :36), one value per FSM of the batch, in the batch's semiring
 * (Log or Tropical):  v_1 = alpha, v_k = T' v_{k-1};
 *   cumulative = 0:  out[b] = omega . v_n            cumulative != 0:  out[b] = (+)_{k=1..n} omega . v_k
 * Runs the emission-free alpha-recursion on the extended system (the phony final state's self loop of
 * weight one is the accumulator) for n + 1 frames.  n >= 1; out: device float[B], natural log. */
int mm_totalsum_f32(mm_batch_t batch, int64_t n, int cumulative, float *out, void *stream);

/* ---- the generic entry: pdfposteriors(fsm, V_hats, C_hats) as the reference declares it (src/inference.jl:145-161) ----
 * Any semiring the FSMs were created with (MM_LOG, MM_TROPICAL, MM_PROB: the function is generic in K), float32 or
 * float64 (FSM{LogSemiring{Float64}} is what the reference's tests build: test/test_fsms.jl:3-7), any sparse state map
 * C_hat (not only the one-hot map of examples/prepare-lfmmi-graphs.jl:15-23), any (P+1) x (N+1) matrices V_hat (not
 * only those expand() makes).  Correctness first: a plain kernel that materialises alpha and beta like the reference.
 * Asynchronous on `stream` like every run call: its workspace (alpha and beta, 2 x N1 x sum S1 elements) and the
 * utterance descriptors live with the batch, grown lazily (growing synchronises; refused while the stream is capturing:
 * size them with mm_batch_reserve_ex first), so a steady-state call allocates nothing, waits for nothing and can be
 * captured in a hipGraph.  The fast kernels are behind mm_pdfposteriors_f32.
 *   maps     NULL (every FSM's own one-hot state map), or B handles (NULL entries: the FSM's own)
 *   val_bytes 4 / 8: the type of Vhat, gamma, ttl
 *   P1       rows of every V_hat_b (P + 1).  Must equal the number of pdfs of the state map in force for every utterance
 *            (src/inference.jl:146-150: vcat(V_hats...) against blockdiag(C_hats...)'); MM_ERR_DIM otherwise -- e.g. a
 *            P x N matrix that expand() (:54-60) was not applied to
 *   Vhat     device; element (b, n, p) of V_hat_b at Vhat[b*v_stride_b + n*v_stride_n + p], n = 0..N1-1 (N1 = N + 1 columns),
 *            p = 0..P1-1 (P1 = P + 1 rows: the last is the phony pdf); values in the semiring's own domain
 *   gamma    device, out: element (b, n, p), n < N1 - 1, p < P1 - 1 (the reference drops the last row and column, :160);
 *            exp() of the quotient for MM_LOG / MM_TROPICAL, the quotient itself for MM_PROB
 *   ttl      device [B], out: the minimum over ALL N1 columns of the per-column sum (:159), in the semiring's domain
 * Z = 0 yields gamma = 0 and ttl = zero(K) (the reference: 0/0). */
typedef struct mm_statemap_s *mm_statemap_t;
/* C_hat (S1 x P1) as CSR: rowptr[S1+1], colidx / val [nnz]; host pointers, not retained. */
int mm_statemap_create(int semiring, int64_t S1, int32_t P1, int64_t nnz, int index_bytes, int index_base, int val_bytes,
                       const void *rowptr, const void *colidx, const void *val, mm_statemap_t *out);
int mm_statemap_destroy(mm_statemap_t map);
int mm_pdfposteriors_ex(mm_batch_t batch, const mm_statemap_t *maps, int val_bytes, int32_t P1, const void *Vhat,
                        int64_t v_stride_b, int64_t v_stride_n, int64_t N1, void *gamma, int64_t g_stride_b, int64_t g_stride_n,
                        int64_t g_stride_p, void *ttl, void *stream);
/* Allocate the generic entry's workspace for calls with val_bytes-sized values and up to N1 = N + 1 columns now
 * (synchronises if it has to grow): call before capturing mm_pdfposteriors_ex in a hipGraph. */
int mm_batch_reserve_ex(mm_batch_t batch, int val_bytes, int64_t N1);

/* Deterministic mode (default off).  Every kernel but one reduces in a fixed order; the general ("item") kernel -- the
 * path of small deep graphs such as LF-MMI numerators -- adds a pdf's state posteriors with LDS float atomics, so the
 * last bits of its gamma can differ between runs.  on != 0 makes it sum over per-pdf state lists in a fixed order
 * instead (one more workgroup barrier per frame: ~20 % slower on such graphs).  The reference has no such switch: its
 * CPU path is deterministic, its CUDA path (src/linalg.jl:213-233) reduces in warp-shuffle order, also fixed. */
int mm_batch_set_deterministic(mm_batch_t batch, int on);

/* Posterior floor of the fast (linear-domain) kernels, default 1e-30.  Those kernels keep float32 products, so terms more
 * than ~126 log2 below their frame's scale drop out; an utterance is accepted from them only if every posterior that can
 * have been lost that way is below the floor (otherwise the exact kernels compute it again, mm_batch_last_redo_count).
 * With sharp emissions (a trained acoustic model: the forward and the backward mass of a frame sit on different states)
 * the default sends every utterance to the exact kernels -- 3 to 6 times the time of a call.  A caller to whom posteriors
 * below, say, 1e-12 are zero (LF-MMI gradients) says so here: results then differ from the reference's by less than the
 * floor in any posterior (those below it may come out as 0), log Z is unaffected beyond 1e-4 relative as before, and
 * inputs up to ~6 sigma of logit spread stay on the fast kernels.  floor in [1e-30, 1e-6]; the log-domain kernels (wave,
 * item, generic) are exact and ignore it.  The reference has no such switch (one algorithm, log domain throughout).
 * Caveat of the DEFAULT floor: the acceptance test bounds every dropped TERM, i.e. an absolute error
 * of K * 7.9e-31 for a pdf of K states -- the 1e-4 relative bar on log gamma holds by construction for posteriors above
 * ~1e-26; between 1e-30 and 1e-26 a posterior of an ACCEPTED utterance can be low by about a per cent (seen once in ~1000
 * fuzzer comparisons: 1.436e-30 computed as 1.423e-30).  mm_batch_set_exact_policy(batch, MM_EXACT_F64_FIRST) removes the
 * float32 kernels from the path altogether. */
int mm_batch_set_posterior_floor(mm_batch_t batch, float floor);

/* How many utterances of the LAST mm_pdfposteriors_f32 call on this batch the fast (linear-domain) kernels handed to
 * the exact kernels ("flag and redo": a value left the range in which float32 products are exact enough; results are
 * the log semiring's either way, only the time differs -- a redone utterance is computed twice).  Reads the marks the
 * call left in the batch's workspace: synchronises `stream` (the stream of that call), nothing on the hot path.
 * *n = 0 for batches that run on the exact kernels only, or before the first call.  The reference has no such
 * path (src/inference.jl:145-161 runs one algorithm for every input); this is an observability hook. */
int mm_batch_last_redo_count(mm_batch_t batch, void *stream, int64_t *n);
/* ... and how many of THOSE the float64 exact kernels (mm_kernel_dpair.hip: the first stop of a marked utterance of a
 * shared-graph batch) handed on to the log-domain kernels: values beyond the double's range that carry mass -- normally 0. */
int mm_batch_last_fallback_count(mm_batch_t batch, void *stream, int64_t *n);
/* 1 if the last mm_pdfposteriors_f32 call on this batch skipped the float32 kernels and ran the float64 exact kernels on
 * the whole batch (the engine does that while more than a quarter of the utterances of the last finished call were
 * beyond the float32 kernels -- a sharp acoustic model; mm_batch_last_redo_count then reports the whole batch), else 0.
 * No synchronisation.  Observability only: results are the same either way. */
int mm_batch_last_exact_first(mm_batch_t batch);
/* Team kernels (graphs beyond one compute unit): out[0] = workgroups of the float32 team kernels' phase-A launches, since the last
 * call of this function, that found their whole team on ONE XCD (they exchange rows by plain stores through that XCD's L2; the
 * others by write-through stores), out[1] = all such workgroups.  The kernels count from the FIRST call of this function on (which
 * returns zeros): a batch nobody asks carries no measurement atomics.  Synchronises the device; a measurement aid (bench.py). */
int mm_batch_team_xcd_stats(mm_batch_t batch, int out[2]);

/* Which linear-domain kernels a shared-graph batch starts with (the batches of the pair / split pair kernels; others ignore it).
 *   MM_EXACT_AUTO (default)  float32 first; float64 first while the last FINISHED call left utterances marked and that costs
 *                            no more rounds of workgroups.  The engine reads that call's count from pinned host memory without
 *                            synchronising, so WHICH kernels a pipelined caller's next call launches depends on host / device
 *                            timing (results are within the parity bar either way; the last bits of gamma and the time are not
 *                            reproducible from run to run), and a hipGraph capture freezes the choice current at capture time.
 *   MM_EXACT_F32_FIRST       always float32 first, marked utterances redone by the float64 kernels: the launches of a call
 *                            are a function of the call alone
 *   MM_EXACT_F64_FIRST       always the float64 kernels on the whole batch (a trained acoustic model's sharp outputs)
 * With a fixed policy two identical call sequences give bit-identical results.  During stream capture MM_EXACT_AUTO behaves
 * as MM_EXACT_F32_FIRST (a captured graph must not bake in the state of an unrelated earlier call).  The reference has no
 * such switch (src/inference.jl:145-161: one algorithm for every input). */
enum mm_exact_policy { MM_EXACT_AUTO = 0, MM_EXACT_F32_FIRST = 1, MM_EXACT_F64_FIRST = 2 };
int mm_batch_set_exact_policy(mm_batch_t batch, int policy);

/* What a RANGE MARK of the float32 linear-domain kernels means (the batches of the pair / split pair kernels; others ignore it).
 * Those kernels mark an utterance when a value of a state vector left the range in which float32 products keep every term.
 *   MM_MARKS_DECIDE (default)  the finish kernel clears the mark when two criteria say that nothing that matters was lost (the
 *                              frames' log Z agree within 2e-4 log2; every term that can have been dropped is below the posterior
 *                              floor): the reference's own benchmark graph marks every utterance after ~55 frames -- its
 *                              initial-context states decay out of the float range -- and none of those marks carries mass.
 *                              Contract: log gamma within 1e-4 relative for posteriors above ~1e-24, an ABSOLUTE error below
 *                              ~1e-27 for smaller ones (a flushed value of a recursion takes its descendants along: a posterior
 *                              of 8.5e-29 has been seen computed as 0 on a 5-frame utterance; DESIGN.md section 3,
 *                              tests/test_gpu_exact.py::test_fuzzer_findings_pin_the_parity_contract).
 *   MM_MARKS_KEEP              a range mark always stays: the exact kernels (float64 / wide-exponent values, 1022 log2 of range)
 *                              compute every utterance whose float32 vectors left the range, whatever the criteria say.  The
 *                              1e-4 relative bar on log gamma then holds down to 1e-30 like SURVEY section 8(d) states it; costs a
 *                              second pass on inputs that raise marks (the reference's WSJ denominator: 2.03 instead of 1.76 ms;
 *                              config 3 on the benchmark's inputs raises none: unchanged).
 * Per batch, takes effect at the next call; the reference has no such switch (src/inference.jl:145-161: one algorithm, log
 * domain, every input). */
enum mm_mark_policy { MM_MARKS_DECIDE = 0, MM_MARKS_KEEP = 1 };
int mm_batch_set_mark_policy(mm_batch_t batch, int policy);

/* What mm_pdfposteriors_f32 does with the posteriors, for the caller's step right behind the path (examples/test_cuda.jl:140-152:
 * the LF-MMI gradient gamma_den - gamma_num, formed by the reference in a separate broadcast over two B x P x N arrays):
 *   accumulate = 0, scale = 1 (default)   gamma_out  = gamma, frames n >= len_b zeroed
 *   accumulate = 0, scale = s             gamma_out  = s * gamma
 *   accumulate = 1, scale = s             gamma_out += s * gamma (frames n >= len_b left as they are): the numerator call with
 *                                         s = -1 on the buffer the denominator call has just written leaves the gradient there,
 *                                         no third pass.  Every element receives exactly one float add per call (a no-return
 *                                         atomic): the result does not depend on any order.
 * Supported by batches of the wave kernel (every graph <= 1023 states and <= 4096 arc slots per direction, any batch: LF-MMI
 * numerators; mm_batch_kernels says which kernel a batch runs); MM_ERR_UNSUPPORTED for the others (their float32 kernels may hand
 * an utterance to the exact kernels, whose result must REPLACE the first: the caller subtracts in a pass of its own).  Per batch,
 * takes effect at the next call. */
int mm_batch_set_gamma_mode(mm_batch_t batch, int accumulate, float scale);

/* ---- the reference's semiring linear algebra on caller-owned device arrays (src/linalg.jl) ------------------------------
 * Generic in K like the reference: semiring in {MM_LOG, MM_TROPICAL, MM_PROB}, val_bytes 4 (Float32) / 8 (Float64) for
 * every value array of a call.  A is a CuSparseMatrixCSR{K} (src/linalg.jl:80: Cint indices): rowptr[rows + 1],
 * colval[nnz], nzval[nnz], index_base 1 as Julia stores them (0 accepted).  All pointers are DEVICE pointers; the calls
 * are asynchronous on `stream`; sizes are checked like the reference's @boundscheck (MM_ERR_DIM = DimensionMismatch).
 * Values are in the semiring's own domain (natural log for Log / Tropical, zero(K) = -inf). */

/* LinearAlgebra.mul!(c, A, b) (src/linalg.jl:163-184; kernel _cukernel_mul_smdv! :213-233, warp_reduce :204-211):
 * c[r] = (+)_k nzval[k] (*) b[colval[k]] over row r.  b_len / c_len: the lengths of b and c (checked against cols / rows).
 * An A without stored entries leaves c untouched (`if length(A.nzVal) > 0`, :169). */
int mm_spmv(int semiring, int val_bytes, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colval,
            int index_base, const void *nzval, const void *b, int64_t b_len, void *c, int64_t c_len, void *stream);
/* LinearAlgebra.mul!(C, A, B, alpha, beta) (src/linalg.jl:240-262; kernel _cukernel_mul_smdm! :268-280):
 * C = (beta (*) C) (+) A (*) B with B (b_rows x b_cols) and C (c_rows x c_cols) column-major with leading dimensions ldb /
 * ldc.  beta = 0: C is overwritten (fill!(C, zero(K)), :247 -- what the 3-argument mul! passes); beta = 1: accumulated into;
 * any other beta: rmul!(C, beta) first (:247), beta a value of K's domain.  alpha is ignored like in the reference. */
int mm_spmm(int semiring, int val_bytes, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colval,
            int index_base, const void *nzval, const void *B, int64_t b_rows, int64_t b_cols, int64_t ldb, void *C, int64_t c_rows,
            int64_t c_cols, int64_t ldc, double beta, void *stream);
/* Sparse vector (.) dense vector broadcast, _copyto!(f, dest, x::CuSparseVector, y) (src/linalg.jl:294-315; kernel :320-328):
 * dest = zero(K) everywhere, then dest[nzind[i]] = f(nzval[i], y[nzind[i]]), f = (*) for op 0 (elmul!, :290), (/) for op 1
 * (eldiv!, :292).  n = length of x, y (y_len) and dest (dest_len). */
int mm_svdv(int semiring, int val_bytes, int op, int64_t n, int64_t nnz, const int32_t *nzind, int index_base, const void *nzval,
            const void *y, int64_t y_len, void *dest, int64_t dest_len, void *stream);

/* ---- multi-GPU boundary (one process per GPU, RCCL over xGMI) -------------------------------------------------
 * The batch is block diagonal (src/fsmops.jl:28-36, src/inference.jl:28-36): utterances shard over the ranks with no
 * collective on the data path.  The only exchange is the total log-likelihood the LF-MMI loss consumes
 * (examples/test_cuda.jl:140-152 sums ttl_num / ttl_den over the utterances), offered here over RCCL so that a host
 * binding without torch.distributed (julia/MarkovModelsAMD.jl) has it too.
 * comm: an ncclComm_t of the calling process.  The library does not link RCCL and never opens one of its own (an
 * ncclComm_t belongs to the RCCL build that made it): it resolves ncclAllReduce / ncclAllGather in the library handed
 * over with mm_set_rccl, else among the process's global symbols.  Both calls are asynchronous on `stream`;
 * MM_ERR_UNSUPPORTED if RCCL is not visible, MM_ERR_HIP if RCCL fails. */

/* dl_handle: what dlopen() returned for the RCCL `comm` was made with (PyTorch loads its bundled librccl.so with local
 * visibility; Libdl.dlopen in Julia likewise), or NULL to go back to the process's global symbols. */
int mm_set_rccl(void *dl_handle);

/* sum (device double[1]) = sum over ALL ranks of sum_b ttl[b], b < B_local (device float[B_local], the ttl output of
 * mm_pdfposteriors_f32), accumulated in float64: a one-block reduction and a one-element all-reduce. */
int mm_allreduce_logz(void *comm, const float *ttl, int64_t B_local, double *sum, void *stream);

/* all (device float[world * B_max]) = the ttl vectors of all ranks, rank r at all + r * B_max.  Every rank passes
 * the same B_max >= its B_local and a ttl buffer of B_max floats (pad with -inf: ranks may hold shards of different
 * sizes). */
int mm_allgather_ttl(void *comm, const float *ttl, int64_t B_max, float *all, void *stream);

/* Test aid (host only, no GPU): evaluate one semiring product out = M (x) in
 * THROUGH THE PACKED FORM the kernels consume, direction 0: M = T_hat'
 * (forward), 1: M = T_hat (backward).  in/out: host float[S1], natural log.
 * argmax (may be NULL): for MM_TROPICAL the back-pointer per row. */
int mm_debug_packed_product(mm_fsm_t fsm, int direction, const float *in, float *out, int32_t *argmax);

/* Test aid (host only, no GPU): the same product evaluated THROUGH THE QUAD FORM of the fast
 * pdfposteriors kernel (internal renumbering, quads of 4 arcs laid out for KQ quads per lane, per-lane
 * running sums, row totals from the lane partials), in the linear domain relative to max(in) like the
 * kernel does.  MM_LOG FSMs only.  stats (may be NULL) receives {quads, lanes, modelled LDS cycles per
 * gather instruction with arcs in CSR order, the same after the bank-aware placement}. */
int mm_debug_quad_product(mm_fsm_t fsm, int direction, int KQ, const float *in, float *out, double stats[4]);

/* Test aid (host only, no GPU): where the quad form for KQ quads per lane puts every row.  order[S1]: internal position ->
 * state of the direction's numbering; recs[4 * S1]: per position the row record the kernel reads, {qe, i1, pdf, i2} -- 2 + the
 * row's last quad (0: a row without arcs), 2 + its first lane-end quad before that (or 0), its pdf, 2 + the second lane end (0:
 * none, 1: more than two -- the long walk i1, i1 + KQ, ... < qe).  MM_LOG FSMs only. */
int mm_debug_quad_layout(mm_fsm_t fsm, int direction, int KQ, int32_t *order, uint16_t *recs);

/* Test aid (host only, no GPU): the same product evaluated THROUGH THE ROW-LANE FORM of the row kernels (mm_rows.h:
 * rows sorted by size and dealt to the compute waves as segments, arcs in per-lane register slots, group sums,
 * internal numbering = finishing order), in the linear domain relative to max(in) like the kernels do.  MM_LOG FSMs
 * only.  stats (may be NULL) receives {arc slots per lane (KA), compute waves, segments, real arcs / arc slots,
 * cost of the most loaded wave, of the least loaded one, modelled LDS cycles per gather instruction with arcs in
 * CSR order, the same after the bank-aware placement}.  Returns MM_ERR_UNSUPPORTED if the FSM does not fit the form. */
int mm_debug_row_product(mm_fsm_t fsm, int direction, const float *in, float *out, double stats[8]);
/* The same with the packer's options: flags bit 0 = the pair form of the pair kernels (8-byte positions, its cost model),
 * bits 1-2 = copies of the linear vector the arcs may read (0: the form's default, 1, 2), bit 3 = the second copy
 * scrambles the low five position bits with the next five instead of rotating by half the banks. */
int mm_debug_row_product_ex(mm_fsm_t fsm, int direction, int flags, const float *in, float *out, double stats[8]);

/* Test aid (host only, no GPU): the product evaluated THROUGH THE SPLIT FORMS of the team kernels (mm_rows.h
 * make_rows_split: the rows cut into H sets, one row-lane form per set whose arcs read the whole team's vector).
 * stats (may be NULL) receives {arc slots per lane, positions of the team's vector, segments, real arcs / arc slots,
 * cost of the most / least loaded wave, modelled LDS cycles per gather before / after the bank-aware placement}. */
int mm_debug_split_product(mm_fsm_t fsm, int H, int direction, const float *in, float *out, double stats[8]);

/* Test aid (host only, no GPU): the pdf-major table of the pair form of `direction` (mm_rows.h RowGraph::pdftab: what the
 * pair kernels' phase B sums the posteriors through), packed like mm_debug_row_product_ex packs the pair forms, both directions,
 * the forward form's partner fields filled.  rows receives the number of rows S1; tab [S1] the table (8 * own position |
 * (8 * position in the other direction's numbering) << 16, rows in pdf-major order); pdfse [2 * (P + 1)] the (first, end) of
 * each pdf's range; slots [S1][2] the two slot-table words of every lane that finishes a row, in the order of the slot table
 * (word 1's high half, / 8, is the row's place in tab).  The forms are packed afresh from the FSM's unpruned matrices by the same
 * make_rows / set_partner code as the forms a batch uploads (those are packed from the pruned matrices): the same construction,
 * not the very table a kernel reads. */
int mm_debug_pair_pdftab(mm_fsm_t fsm, int direction, int64_t *rows, uint32_t *tab, uint16_t *pdfse, uint32_t *slots);

/* Test aid (host only, no GPU): the product evaluated THROUGH THE WAVE FORM of the wave kernel (one wave per direction:
 * segments of 64 / g rows, at most 4 arcs per lane and segment, log2 weights, lane-group log-sum-exp).  stats (may be
 * NULL) receives {arc slots per lane, segments, real arcs / arc slots, modelled LDS cycles per gather}.
 * MM_ERR_UNSUPPORTED if the FSM does not fit the form (more than 16 segments). */
int mm_debug_wave_product(mm_fsm_t fsm, int direction, const float *in, float *out, double stats[4]);

/* Test aid (host only, no GPU): the product evaluated THROUGH THE STREAM FORM of the stream kernels (mm_stream.hip: rows sorted
 * by length and cut into segments of 64, one lane per row, rows of more than 128 arcs on a whole wave; 8-byte arc records
 * {LDS address of the source, high dword of the weight's double}; float64 accumulation) exactly as a workgroup walks it.
 * MM_LOG FSMs of up to 16 370 states and 1024 pdfs (MM_ERR_UNSUPPORTED otherwise).  stats (may be NULL) receives {arc slots per
 * lane summed over the 15 waves, segments, real arcs / arc slots, arc slots of the most loaded wave}. */
int mm_debug_stream_product(mm_fsm_t fsm, int direction, const float *in, float *out, double stats[4]);
/* ... through the forms of a TEAM of H = 1, 2 or 4 workgroups (round 6: the rows of a direction dealt to H sets, one record stream per
 * set and wave, the sets' regions of the vector padded to multiples of 4 positions): the same product, set by set. */
int mm_debug_stream_team_product(mm_fsm_t fsm, int H, int direction, const float *in, float *out, double stats[4]);

/* Test aid (host only, no GPU): the static bound the fast kernels use to recognise dead rows without a walk --
 * the fewest arcs from an initial state to every state (direction 0) or from every state to the phony final
 * state (direction 1), on the pruned graph; -1 = unreachable (such states are dropped).  out: host int32[S1].
 * alpha_n[s] (resp. beta_n[s]) is zero(K) whenever n - 1 (resp. len + 1 - n) is smaller.  MM_LOG FSMs only. */
int mm_debug_reach_distance(mm_fsm_t fsm, int direction, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* MARKOVMODELS_AMD_H */
