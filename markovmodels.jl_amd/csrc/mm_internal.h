// mm_internal.h -- what the translation units of the engine share on the host side (not part of the C ABI).
// mm_engine.hip holds the C ABI, the handles and the item / quad / row kernels; kernel families with many template
// instances live in translation units of their own (compiled in parallel, see Makefile) behind plain launch functions.
// Every launch with dynamic LDS, in all of them, goes through mm_launch below and asks MM_LDS_MAX what fits; the four
// translation units of the pair family share their geometry, team placement and launch sequence (end of mm_kernel_pairs.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/markovmodels_amd.h"

namespace mm {

struct RunParams;  // mm_kernels.hip

// records the message mm_last_error() returns on this thread; returns `code`
int mm_fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::mm::mm_fail(MM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

#define MM_LDS_MAX (size_t(160 * 1024))  // LDS bytes of a compute unit: what one workgroup can ask for
// The one launch: raises the kernel's dynamic-LDS limit to lds_bytes (on every launch: nothing is remembered), launches, and
// returns MM_OK or the mm_fail of the HIP error.  (lds_bytes 0: a kernel without dynamic LDS has no limit to raise)
// (static: an instance per translation unit, none among the library's dynamic symbols)
template <typename... P, typename... A>
static int mm_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const A &...args) {
    if (lds_bytes) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes)));
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

// The instances of an item-form entry's kernels: NI = 8 register-resident items per wave with the state vectors in LDS or in global
// memory (bigv), NI = 0 (FSMs of more than 65534 states) with global vectors only.  f(ItemInstance<NI, BIGV>{}) launches the
// entry's kernels of the instance; no instance: MM_ERR_UNSUPPORTED in the entry's name.
template <int NI_, bool BIGV_>
struct ItemInstance {
    static constexpr int NI = NI_;
    static constexpr bool BIGV = BIGV_;
};
template <class F>
static int item_instance(const char *entry, int NI, bool bigv, F &&f) {
    if (NI == 8) return bigv ? f(ItemInstance<8, true>{}) : f(ItemInstance<8, false>{});
    if (NI == 0 && bigv) return f(ItemInstance<0, true>{});
    return mm_fail(MM_ERR_UNSUPPORTED, std::string(entry) + ": no instance for this geometry");
}

#define MM_ROW_RS 8192  // LDS bytes of one copy of the linear vector (row kernels) / half a pair vector (pair kernels)
#define MM_PAIR_KA 44   // arc slots per lane of the pair kernels
// pdfs (+ 1) of the pair / split pair / float64 pair kernels: passes of 64 lanes of their service waves (the NJ of the instances),
// and the floats of one slot of per-pdf partial sums a team publishes (PairLay::XPS, mm_kernel_pairs.hip)
#define MM_PAIR_P1MAX 506
#define MM_PAIR_SPLIT_Q10 512  // (mm_engine.hip: RunParams::split_q10 of the pair kernels)
// (teams of 8 have no LDS for the arrays of 512 pdfs: 5 passes, 314 pdfs)
inline int mm_pair_nj(int P1, int H = 1) { return P1 <= 128 ? 2 : (P1 <= 250 ? 4 : (H == 8 ? (P1 <= 314 ? 5 : 0) : (P1 <= MM_PAIR_P1MAX ? 8 : 0))); }
inline int mm_pair_xps(int P1, int H = 1) { const int nj = mm_pair_nj(P1, H); return nj <= 4 ? 512 : 128 * nj; }
// split pair kernels (teams of H workgroups per utterance pair and direction): bytes of half a pair vector, arc slots per
// lane, compute waves (+ a service wave and an exchange wave)
#define MM_SPLIT_RS 12288
#define MM_SPLIT_RSH 13312  // LDS bytes of the rows ONE workgroup of a team finishes (the sets are balanced by arcs: their row
                            // counts differ by a few per cent; 1663 rows leave 51 slot rows of LDS in phase B)
// teams of 4: the team's vector of pairs is 32 KB (up to 4094 states), a workgroup finishes a quarter of the rows
#define MM_SPLIT4_RS 16384
#define MM_SPLIT4_RSH 9216
// teams of 8: 47.5 KB (up to ~6050 states), an eighth of the rows each (a multiple of 1 KB: the partner rows come in 1 KB DMAs);
// what the LDS of a compute unit holds next to two such vectors
#define MM_SPLIT8_RS 24320
#define MM_SPLIT8_RSH 6144
// (the geometry of a team of H: template arguments of the team kernels of mm_split_tu.hip, mm_dpair_tu.hip and mm_wpair_tu.hip)
constexpr int mm_split_rs(int H) { return H == 8 ? MM_SPLIT8_RS : (H == 4 ? MM_SPLIT4_RS : MM_SPLIT_RS); }
constexpr int mm_split_ka(int) { return 36; }  // arc slots per lane, whatever the team
constexpr int mm_split_rsh(int H) { return H == 8 ? MM_SPLIT8_RSH : (H == 4 ? MM_SPLIT4_RSH : MM_SPLIT_RSH); }
#define MM_SPLIT_NWC 14

// ---- generic path (mm_generic.hip): any semiring, float32 or float64, any C_hat / V_hat
struct FsmGenView {   // host copies of one FSM in double, natural units; [0]: CSR of T_hat' (forward), [1]: of T_hat (backward)
    int semiring = 0;
    int64_t S1 = 0;
    int32_t P1 = 0;
    const int64_t *ptr[2] = {nullptr, nullptr};
    const int32_t *col[2] = {nullptr, nullptr};
    const double *val[2] = {nullptr, nullptr};
    const double *init = nullptr;   // dense alpha_hat [S1]
    const int32_t *s2p = nullptr;   // the FSM's one-hot state map [S1]
    void *dev[2] = {nullptr, nullptr};  // device copies made by the generic path (float32, float64); freed by mm_generic_free
};
FsmGenView *mm_fsm_gen_view(mm_fsm_t f);
// what the generic entry keeps with the batch between calls (owned and freed by the batch): the alpha / beta workspace,
// the utterance descriptors on the device and the host image they were uploaded from (a call with the same FSMs, maps
// and float type uploads nothing)
struct GenScratch {
    void *ws = nullptr;
    size_t ws_bytes = 0;
    void *d_utts = nullptr;
    size_t utts_bytes = 0;
    std::vector<char> host;  // what d_utts holds
    std::string last_kernels;  // what the last call of the generic entry launched (mm_batch_kernels, entry 2)
};
GenScratch *mm_batch_gen_scratch(mm_batch_t h);
int mm_batch_gen_view(mm_batch_t h, int64_t *B, const mm_fsm_t **fsms, int *semiring, int *device);
void mm_generic_free(void *dev);

// ---- pair kernels (mm_pairs_tu.hip)
struct PairLaunch {
    int64_t B = 0;
    int nwc = 1, slotrows = 0, max_P1 = 0, pair_ka = 0, H = 1;
    bool small = false;  // every FSM has at most 127 states: the instance whose service wave copies and scans one row of 64 float4
};
// whether a launch runs the small-graph instances (mm_launch_pairs, mm_launch_pair_export, and what mm_batch_kernels says)
inline bool pair_small_instances(const PairLaunch &pl) { return pl.H == 1 && pl.small && pl.max_P1 <= 128; }
int mm_launch_pairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0);
// alpha / beta export on the pair kernels (phase A of one direction over all frames + a layout pass): dir 0 alpha, 1 beta
bool mm_pair_export_fits(const PairLaunch &pl);
int mm_launch_pair_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t s0);
size_t mm_pair_lds_bytes(int phase, int nslotrows, int max_P1);
size_t mm_pair_hand_bytes();
// ---- the float64 exact pair kernels (mm_dpair_tu.hip): one utterance per workgroup, for the utterances marked in p.redo
int mm_launch_dpairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0);
// ---- the wide-exponent pair kernels (mm_wpair_tu.hip): two utterances per workgroup with a float64's range, whole batches only
// (every utterance marked in p.redo): what a call that goes to the exact kernels FIRST runs when the batch fits
bool mm_wpair_fits(const PairLaunch &pl);
int mm_launch_wpairs(const PairLaunch &pl, const RunParams &p, hipStream_t s0);
// ---- split pair kernels (mm_split_tu.hip): teams of pl.H workgroups
int mm_launch_split(const PairLaunch &pl, const RunParams &p, hipStream_t s0);
size_t mm_split_lds_bytes(int H, int phase, int nslotrows, int max_P1);
bool mm_split_export_fits(const PairLaunch &pl);  // alpha / beta export on the team kernels: teams of 2 and 4, up to 128 pdfs
int mm_launch_split_export(const PairLaunch &pl, const RunParams &p, int dir, hipStream_t s0);  // (0: no instance for that many pdfs)


// ---- wave kernel (mm_wave_tu.hip)
#define MM_WAVE_RS 4352  // LDS bytes of one state vector of the wave kernel
#define MM_WAVE_WAVES 4  // waves per agent (direction) of the wave kernel
struct WaveLaunch {
    int64_t B = 0;
    int nseg = 0, max_P1 = 0, n_cus = 256;
};
int mm_launch_wave(const WaveLaunch &wl, const RunParams &p, hipStream_t stream);

// ---- lane kernel (mm_lane_tu.hip): graphs of up to 64 states and 64 pdfs, one wave per direction
size_t mm_lane_dev_bytes();
void mm_lane_dev_fill(void *dst, const double *w0, const double *w1, const float *init, const float *fin, const int *s2p, const int *pdf_ptr,
                      const int *pdf_states, int S, int P, int ident);
int mm_launch_lane(int64_t B, int max_S, const RunParams &p, hipStream_t stream);

// ---- stream kernels (mm_stream.hip): graphs beyond every register-resident form -- the arcs streamed from L2 as 8-byte records,
// the vector in LDS as wide-exponent 32-bit values, one utterance per workgroup, forward launch then backward launch
struct StreamForm;
size_t mm_stream_lds_bytes(int S1, int P1);
// NJ of mm_stream_kernel<NJ, H>: 64-lane passes over the P1 = P + 1 pdfs of a batch.  One owner of the arithmetic: the launcher, the
// LDS layout and mm_batch_kernels all ask here.
int mm_stream_nj(int P1);
// (H: workgroups of a team per utterance and direction -- 1, 2 or 4; the rows of a direction dealt to H sets)
int mm_stream_build(int64_t S1, int32_t P1, const int64_t *const rowptr[2], const int32_t *const col[2], const float *const val[2],
                    const float *init, const int32_t *s2p, bool upload, int H, StreamForm **out);  // *out NULL: does not fit
void mm_stream_free(StreamForm *f);
const void *mm_stream_dev(const StreamForm *f);
void mm_stream_eval(const StreamForm *f, int d, const float *in, float *out, double stats[4]);
int mm_stream_pick_h(int64_t B, int n_cus);
size_t mm_stream_slot(int max_S1);
size_t mm_stream_extra_bytes(int64_t B, int64_t total_s1p, int64_t N, size_t off[4], int H, int max_S1);
size_t mm_stream_exchange_bytes(int64_t B, int H, int max_S1);
int mm_launch_stream(int64_t B, int n_cus, int max_S1, int max_P1, int H, const RunParams &p, hipStream_t st);

// ---- Viterbi on the row-lane form (mm_vit_tu.hip)
struct VitLaunch {
    int64_t B = 0;
    int n4 = 0, n2 = 0, max_P1 = 0, max_S1p = 0, max_arcs = 0, bp_row = 0;  // n4 x n2: wide / narrow positions per wave
};
// What mm_launch_viterbi launches for a batch: the forward instance mm_vit_kernel<n4,n2,nj> and the back-trace's plan -- csrl: the
// graph's row pointers and sources sit in LDS next to the ring (mm_vit_backtrace_kernel<true>), R: frames per buffer of the ring,
// lds: the back-trace's dynamic LDS bytes.  One owner of the arithmetic: the launcher and mm_batch_kernels both ask here.
struct VitPlan {
    int nj = 0, R = 0;
    bool csrl = false;
    size_t lds = 0;
};
int mm_vit_plan(const VitLaunch &vl, VitPlan *pl);  // MM_ERR_UNSUPPORTED: no instance, or no room for one row of back-pointers
int mm_launch_viterbi(const VitLaunch &vl, const RunParams &p, hipStream_t stream);

// ---- quad kernels (mm_quad_tu.hip)
struct QuadLaunch {
    int64_t B = 0;
    int kq = 0, nw = 1, max_S1p = 0;
    size_t lds = 0;
};
int mm_launch_quad_pass(int pass, const QuadLaunch &ql, const RunParams &p, hipStream_t stream);

// ---- arc posteriors (mm_arcs_tu.hip: mm_log_kernel's forward half, then mm_arc_kernel and mm_arc_scatter_kernel on the item form)
struct ArcDev {  // one utterance's arc form (mm_engine.hip ensure_arc_forms)
    const int *k2slot;       // [nnz] caller entry -> slot (slot row * 64 + lane) of the backward item form; -1: none
    const int *init_states;  // [n_init] the states of alpha_hat in the caller's init_idx order
    long long slot_off;      // this utterance's first slot in ArcParams::acc
    int nnz, n_init;
    int kphony;  // caller entry of the phony self-loop (final -> final), -1: none
    int pad;
};
struct ArcParams {
    const ArcDev *arcs;  // [B]
    double *acc;         // [sum of the utterances' backward slots] per-slot sums
    float *post1;        // [sum S1p] state posteriors of frame 1
    float *counts;
    long long csb;
    float *init_counts;  // NULL: not asked for
    long long isb;
    float *ttl;          // NULL: not asked for
};
// LDS bytes of mm_arc_kernel behind the item kernel's plan: the per-wave posterior sums of two frames
#define MM_ARC_LDS_EXTRA (2 * MM_MAX_WAVES * sizeof(float))
// NI: register-resident items per wave (8, or 0 for FSMs of more than 65534 states); bigv: the state vectors in global memory
int mm_launch_arcs(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const ArcParams &ap, hipStream_t stream);

// ---- per-frame arc-class posteriors (mm_arcclass_tu.hip: mm_log_kernel's forward half, then mm_arcclass_kernel on the item form)
struct alignas(16) ClassRec {  // one classified entry i -> j, at its rank (sorted by class, then by the caller's entry index)
    int row, col;              // i, j
    float w;                   // log2 T_hat_ij, the weight of the entry's slot of the backward item form
    int k;                     // the caller's entry
};
struct ClassDev {  // one utterance's class plan (mm_engine.hip mm_batch_set_arc_classes)
    const ClassRec *recs;  // [M]
    const int *cptr;       // [C + 1] class c owns the ranks [cptr[c], cptr[c + 1])
    long long term_off;    // the ranks of the utterances before this one (its rows in ArcClassParams::terms start at 2 * term_off)
    int M, C;
    int cphony;  // class of the phony self-loop (final -> final), -1: none
    int lgl;     // log2 of the lanes that sum one class: 0, 3 or 6 by the plan's mean class size
};
struct ArcClassParams {
    const ClassDev *cls;  // [B]
    float *terms;         // per utterance [2][M] in the workspace; read when terms_global
    int terms_global;     // 0: the term rows live in LDS behind the arc kernel's plan
    float *xi;
    long long xsb, xsn, xsc;
    float *ttl;  // NULL: not asked for
};
// lds_bytes: the item kernel's plan, as mm_launch_arcs; term_lds: bytes of the term rows in LDS (0: they are global)
int mm_launch_arcclass(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, size_t term_lds, const RunParams &p, const ArcClassParams &cp,
                       hipStream_t stream);

// ---- posteriors with per-frame arc-class scores (mm_scored_tu.hip: mm_scored_fwd_kernel, mm_scored_bwd_kernel on the item form)
struct ScoredDev {  // one utterance's class planes (mm_engine.hip build_score_planes, with the class plan)
    const unsigned short *plane[2];  // [slots of the forward / backward item form] class id of the slot's entry; C: none
    const unsigned short *rcls;      // [M] the class of every rank of ClassDev::recs
};
struct ScoredParams {
    const ClassDev *cls;  // [B]
    const ScoredDev *sc;  // [B]
    const float *U;       // [b * usb + t * usn + c * usc], rows t < len_b only; NULL: no scores
    long long usb, usn, usc;
    int C;                // classes of the plan
    int urow;             // floats of one score row in LDS: C + 1 rounded up to a multiple of 4
    float *terms;         // as ArcClassParams
    int terms_global;
    float *xi;            // NULL: not asked for
    long long xsb, xsn, xsc;
    float *ttl;           // NULL: not asked for
};
// floats of one score row in LDS for a plan of C classes
inline int mm_scored_urow(int64_t C) { return int((C + 1 + 3) & ~int64_t(3)); }
// lds_bytes: the arc kernel's size (the item kernel's plan + MM_ARC_LDS_EXTRA) + the two score rows, of both kernels; term_lds: bytes
// of the term rows the backward kernel keeps in LDS behind them (0: they are global).  gamma (NULL: not asked for) goes where
// RunParams says.
int mm_launch_scored(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, size_t term_lds, const RunParams &p, const ScoredParams &sp,
                     hipStream_t stream);

// ---- posterior path sampling (mm_sample_tu.hip: mm_log_kernel's forward half, then mm_sample_kernel on the sampling form)
#define MM_SAMPLE_NW 8  // waves of a workgroup of mm_sample_kernel that run chains (+ one that stages the alpha~ rows)
#define MM_SAMPLE_CW 8  // the most chains one wave carries in registers (1, 2, 4 or 8: mm_sample_tu.hip sample_cw)
struct SampleRec {  // one in-arc i -> j of the sampling form, in the list of its destination j (parallel entries merged)
    int32_t src;    // i
    float w;        // log2 T_hat_ij
    int32_t start;  // the in-list of i: where the walk goes on when i is drawn (no second dependent load per frame)
    int32_t deg;
};
struct SampleDev {  // one FSM's sampling form (mm_engine.hip ensure_sample_forms)
    const SampleRec *recs;
    int fin_start, fin_deg;  // the in-list of the phony final state = the omega column (its self-loop left out)
};
struct SampleParams {
    const SampleDev *forms;  // [B]
    int *paths;
    long long psb, psk;
    float *logprob;  // NULL: not asked for
    long long lsb;
    float *ttl;      // NULL: not asked for
    int K;
    unsigned key0, key1;  // the seed's two halves: the key of the counter-based generator
};
// forward launch as mm_launch_arcs (NW, NI, bigv, lds_bytes of the item kernel); stage: the alpha~ rows go through the LDS of
// mm_sample_kernel (2 * max_S1p floats), else they are gathered from global memory
int mm_launch_sample(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, bool stage, int max_S1p, int n_cus, const RunParams &p,
                     const SampleParams &sp, hipStream_t stream);

// ---- expected path cost and its gradient (mm_cost_tu.hip: mm_cost_fwd_kernel, mm_cost_bwd_kernel on the item form)
struct CostParams {
    const float *cost;  // [b * csb + n * csn + p], frames below len_b only
    long long csb, csn;
    float *risk;   // [B]
    float *grad;   // strides as gamma's
    float *gamma;  // NULL: not asked for
    long long gsb, gsn, gsp;
    float *ttl;    // NULL: not asked for
    float *ws_r;   // [sum_b S1p_b][N+1] the centred r rows, laid out like RunParams::ws_alpha
    double *ws_o;  // [B][N+2] per-frame offsets O_n of the r rows; [0]: risk
    float *ws_big; // global-memory vectors: [B][big_stride] floats (8 * max S1p)
    long long big_stride;
};
// lds_bytes: cost_lds_plan(...).total * 4 of the geometry (state vectors in LDS, or bigv: in CostParams::ws_big)
int mm_launch_cost(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const CostParams &cp, hipStream_t stream);
size_t mm_cost_lds_bytes(int S1p, int P1p);

// ---- expected arc-class cost and its gradient (mm_classcost_tu.hip: mm_classcost_fwd_kernel, mm_classcost_bwd_kernel on the item form)
struct ClassCostParams {
    const ScoredDev *sc;  // [B] the class planes of the plan (as ScoredParams::sc)
    const float *A;       // [b * asb + t * asn + c * asc], rows t < len_b only
    long long asb, asn, asc;
    int C;                // classes of the plan
    int urow;             // floats of one cost row in LDS: mm_scored_urow(C)
    const float *D;       // [b * dsb + n * dsn + p], frames below len_b only; NULL: zeros
    long long dsb, dsn;
    float *risk;   // [B]
    float *grad;   // strides as gamma's
    float *gamma;  // NULL: not asked for
    long long gsb, gsn, gsp;
    float *ttl;    // NULL: not asked for
    float *ws_r;   // as CostParams
    double *ws_o;
    float *ws_big;
    long long big_stride;
};
// lds_bytes: the cost kernels' plan (mm_cost_lds_bytes) + the two cost rows
int mm_launch_classcost(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const ClassCostParams &cp, hipStream_t stream);

// ---- posterior path entropy and its gradient (mm_entropy_tu.hip: mm_entropy_fwd_kernel, mm_entropy_bwd_kernel on the item form)
struct EntropyParams {
    float *entropy;  // [B]
    float *grad;     // strides as gamma's; NULL: not asked for
    float *gamma;    // NULL: not asked for
    long long gsb, gsn, gsp;
    float *ttl;      // NULL: not asked for
    float *ws_h;     // [sum_b S1p_b][N+1] the centred Hf rows, laid out like RunParams::ws_alpha; NULL: a value-only call keeps
                     // no frame (neither the alpha~ rows nor C_n, O_n are written)
    double *ws_o;    // [B][N+2] per-frame offsets O_n of the Hf rows; [0]: H
    float *ws_big;   // global-memory vectors: [B][big_stride] floats (8 * max S1p)
    long long big_stride;
};
// lds_bytes: entropy_lds_plan(...).total * 4 of the geometry (state vectors in LDS, or bigv: in EntropyParams::ws_big);
// backward false: the forward kernel alone (value and ttl)
int mm_launch_entropy(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, bool backward, const RunParams &p, const EntropyParams &ep,
                      hipStream_t stream);
size_t mm_entropy_lds_bytes(int S1p, int P1p);

// ---- pdf posteriors of the leaky HMM (mm_leaky_tu.hip: mm_leaky_fwd_kernel, mm_leaky_bwd_kernel on the item form)
struct LeakDev {  // one utterance's leak rows (mm_engine.hip ensure_leak_rows)
    const float *rho;  // [S1] log2 (+)_k pi(k) T_hat(k, j): what a leak into the initial states brings to row j
};
struct LeakParams {
    const LeakDev *rows;  // [B]
    float leps2;          // log2 of the leak coefficient (-inf: no leak)
};
// lds_bytes: leaky_lds_plan(...).total * 4 of the geometry (state vectors in LDS, or bigv: in RunParams::ws_big); gamma and ttl
// go where RunParams says
int mm_launch_leaky(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const LeakParams &lp, hipStream_t stream);
size_t mm_leaky_lds_bytes(int S1p, int P1p);

// ---- forward filtering posteriors with a carried state (mm_filter_tu.hip: mm_filter_kernel on the item form)
struct FilterParams {
    const float *state_in;  // [total states] natural log, element (b, s) at state_off_b + s; NULL: the FSMs' own initial vectors
    float *state_out;       // as state_in (may be the same buffer); NULL: not asked for
    float *filt;            // NULL: not asked for
    long long fsb, fsn, fsp;
    float *incr;            // [b * isb + n]; NULL: not asked for
    long long isb;
    float *ttl;             // NULL: not asked for
};
// lds_bytes: filter_lds_plan(...).total * 4 of the geometry (state vectors in LDS, or bigv: in RunParams::ws_big); the call keeps
// nothing in the workspace
int mm_launch_filter(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const FilterParams &fp, hipStream_t stream);
size_t mm_filter_lds_bytes(int S1p, int P1p);

// ---- fixed-lag smoothing posteriors (mm_window_tu.hip: mm_window_fwd_kernel, mm_window_bwd_kernel on the item form)
struct WindowParams {
    const float *state_in;  // as FilterParams::state_in; NULL: the FSMs' own initial vectors
    float *state_out;       // as state_in (may be the same buffer); NULL: not asked for
    const int *closed;      // [B] != 0: the window ends on the final weights; NULL: every window ends open
    const int *commit;      // [B] the frame state_out and lcommit belong to (clamped to [0, len]); NULL: len
    float *lcommit;         // [B]; NULL: not asked for
};
// lds_bytes: window_lds_plan(...).total * 4 of the geometry (state vectors in LDS, or bigv: in RunParams::ws_big); gamma and ttl
// (NULL: not asked for) go where RunParams says
int mm_launch_window(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const WindowParams &wp, hipStream_t stream);
size_t mm_window_lds_bytes(int S1p, int P1p);
// the forward kernel alone (what mm_launch_window launches first): the alpha~ store and the open / closed total in ws_c[0]
int mm_launch_window_fwd(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const WindowParams &wp, hipStream_t stream);

// ---- segment posteriors (mm_segment_tu.hip: mm_window_fwd_kernel as it stands, then mm_segment_bwd_kernel on the item form)
struct SegmentParams {
    const float *state_in;  // as FilterParams::state_in; NULL: the FSMs' own initial vectors
    const int *end_mode;    // [B] 0: open; 2 with end_in given: the carried end vector; else: the final weights.  NULL: every segment ends open
    const float *end_in;    // layout of state_in, natural log: b_len of a carried end (the final state's entry is not read); NULL: none
    float *end_out;         // as end_in (may be the same buffer): ln b_0 - lend; NULL: not asked for
    float *lend;            // [B] ln max b_0; NULL: not asked for
};
// lds_bytes: the window entry's (window_lds_plan); gamma and ttl (NULL: not asked for) go where RunParams says
int mm_launch_segment(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, const RunParams &p, const SegmentParams &sp, hipStream_t stream);

// ---- windowed best paths (mm_vitwindow_tu.hip: mm_vitwindow_fwd_kernel, mm_vitwindow_trace_kernel on the item form; tropical batches)
struct VitWindowParams {
    const float *state_in;  // layout of FilterParams::state_in, natural log; NULL: the FSMs' own initial vectors
    float *state_out;       // as state_in (may be the same buffer); NULL: not asked for
    const int *closed;      // [B] != 0: the window ends in the phony final state; NULL: every window ends open
    const int *commit;      // [B] the frame state_out and mcommit belong to (clamped to [0, len]); NULL: len, or 0 with commit_converged
    int commit_converged;   // != 0: the commit frame is no earlier than the convergence point
    float *mcommit;         // [B]; NULL: not asked for
    int *ncommit;           // [B]; NULL: not asked for
    int *converged;         // [B]; NULL: not asked for
    // workspace, rows laid out like RunParams::ws_alpha (per utterance [N + 1][S1p]):
    int *ws_bp;             // row 0: the flags of the states a surviving path ends in; row r >= 1: the back-pointers of frame r + 1
    float *ws_best;         // row r >= 1: the pre-emission maxima of step r + 1 (state_out of commit frame r before m_r is taken off)
    float *ws_m;            // [B][N + 2]: [n] = the maximum of frame n over the real states, n = 1..len
    int *ws_end;            // [B] the state the best path ends in at frame len (-1: no path)
};
// lds_bytes: mm_vitwindow_lds_bytes of the geometry (state vectors in LDS, or bigv: in RunParams::ws_big); path and score go where
// RunParams says
int mm_launch_vitwindow(int64_t B, int NW, int NI, bool bigv, size_t lds_bytes, int max_S1p, const RunParams &p, const VitWindowParams &wp,
                        hipStream_t stream);
size_t mm_vitwindow_lds_bytes(int S1p, int P1p);
bool mm_vitwindow_flags_global(int S1p);  // the trace kernel's flags do not fit the LDS: they live in RunParams::ws_big

// ---- best paths with arc classes (mm_classpath_tu.hip: mm_classpath_fwd_kernel, mm_classpath_trace_kernel on the item form; tropical
// batches)
struct ClassPathParams {
    const ScoredDev *sc;  // [B] the class planes of mm_batch_set_path_classes (plane[0] alone); NULL: no plan (mode 0)
    const float *U;       // as ScoredParams::U; NULL: no scores
    long long usb, usn, usc;
    int C;                // classes of the plan (0: none)
    int urow;             // floats of one score row in LDS: mm_scored_urow(C)
    int *classes;         // [b * csb + t]; NULL: not asked for
    long long csb;
    // workspace, rows laid out like RunParams::ws_alpha (per utterance [N + 1][S1p]); row r >= 1: frame r + 1
    int *ws_bp;               // the back-pointers
    unsigned short *ws_bc;    // the class ids of the maximisers (C: none)
    unsigned short *ws_cbuf;  // bigv: the two class rows of every utterance, [B][cbuf_stride]
    long long cbuf_stride;
};
// mode: 0 no plan, 1 classes, 2 classes and scores.  lds_bytes: mm_classpath_lds_bytes of the geometry (state vectors in LDS, or bigv:
// in RunParams::ws_big) + the two score rows (mode 2); path and score go where RunParams says
int mm_launch_classpath(int64_t B, int NW, int NI, bool bigv, int mode, size_t lds_bytes, const RunParams &p, const ClassPathParams &cp,
                        hipStream_t stream);
size_t mm_classpath_lds_bytes(int S1p, int P1p);

// ---- beam-pruned best-path lattices (mm_lattice_tu.hip: mm_lattice_prune_kernel in its count and its write mode, mm_lattice_scan_kernel
// between them; tropical batches)
struct LatticeDev {  // one utterance's arc table (mm_engine.hip ensure_lattice_arcs): the entries of T_hat in the caller's order
    const int *src;    // [nnz] source state; -1: the phony self-loop
    const int *dst;    // [nnz] destination state
    const float *w;    // [nnz] weight, natural log
    int nnz, pad;
};
struct LatticeParams {
    const LatticeDev *arcs;    // [B]
    const float *alpha, *beta; // the exported tropical recursions, row n (frame n + 1) at n * row_stride, an utterance at UttDesc::state_off
    long long row_stride;
    const float *beam;         // [B]
    const float *best;         // [B] alpha_{N+1}(f)
    int *counts;               // [b * csb + t]
    long long csb;
    long long *offs;           // [B * N + 1] the exclusive scan of the counts
    int *arc;                  // NULL: the count-only call
    float *score;
    long long cap;
};
// count pass, scan (offs and *total), write pass (skipped when lp.arc is NULL).  global: the two rows of a cell are gathered from
// global memory, else staged in mm_lattice_lds_bytes(max_S1p) of LDS
int mm_launch_lattice(int64_t B, bool global, int max_S1p, const RunParams &p, const LatticeParams &lp, long long *total, hipStream_t stream);
size_t mm_lattice_lds_bytes(int S1p);

// ---- lattice posteriors (mm_latpost_tu.hip: mm_latpost_fb_kernel, one workgroup per utterance over the records of a lattice, and
// mm_latpost_gamma_kernel, one workgroup per utterance and frame; tropical batches -- the arc table is mm_lattice_f32's)
#define MM_LATPOST_NT 1024       // threads of a workgroup of the forward-backward, by measurement (profiles/latticeposteriors_bench.json);
                                 // MM_LATPOST_NT under MM_DEBUG: 256, 512 or 1024
#define MM_LATPOST_GAMMA_NT 256  // ... and of the per-pdf sums
struct LatPostParams {
    const LatticeDev *arcs;  // [B]
    const long long *offs;   // [B * N + 1] the caller's cell offsets (clamped into [0, nrec] by the kernels)
    const int *arc;          // [nrec] the caller's records
    long long nrec;
    const float *extra;      // [nrec] or NULL
    float *post;             // [nrec]
    float *logz;             // [B]
    float *gamma;            // NULL: no per-pdf sums; row (b, n) at b * gsb + n * gsn
    long long gsb, gsn;
};
// the forward-backward in its instance of `nt` threads, then the per-pdf sums when lp.gamma is given
int mm_launch_latpost(int64_t B, int nt, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, hipStream_t stream);
size_t mm_latpost_lds_bytes(int S1p);       // a head + 16 bytes per state: two 32-bit words and a 64-bit sum
size_t mm_latpost_gamma_lds_bytes(int P1);  // a 64-bit sum per pdf

// ---- lattice expected cost (mm_latcost_tu.hip: mm_latcost_fb_kernel, the forward-backward of the lattice posteriors with the cost
// recursions ca / cb carried beside a / b, and mm_latcost_grad_kernel, the per-pdf sums of diff and of exp(post))
struct LatCostParams {       // beside a LatPostParams, whose gamma / gsb / gsn serve grad too
    const float *cost;       // [nrec]
    float *risk;             // [B]
    float *diff;             // [nrec]; between the passes the record's centred forward cost
    float *grad;             // NULL: not computed; row (b, n) at b * gsb + n * gsn
};
// the forward-backward with costs in its instance of `nt` threads, then the per-pdf sums when lc.grad or lp.gamma is given
int mm_launch_latcost(int64_t B, int nt, int max_S1p, int max_P1, const RunParams &p, const LatPostParams &lp, const LatCostParams &lc,
                      hipStream_t stream);
size_t mm_latcost_lds_bytes(int S1p);      // a head + 28 bytes per state: the 16 of the posteriors, a 64-bit cost sum and a float
size_t mm_latcost_grad_lds_bytes(int P1);  // a head + two 64-bit sums per pdf

// ---- lattice best paths (mm_latbest_tu.hip: mm_latbest_kernel, the tropical forward-backward over the records of a lattice with the
// trace of the best path, one workgroup per utterance; the workgroup is MM_LATPOST_NT's)
struct LatBestParams {       // beside a LatPostParams, whose post is score and whose logz is best (gamma unused)
    long long *rec;          // [b * rsb + t] the best path's records; NULL: not asked for
    long long rsb;
    int *path;               // [b * psb + t] their source states; NULL: not asked for
    long long psb;
};
int mm_launch_latbest(int64_t B, int nt, int max_S1p, const RunParams &p, const LatPostParams &lp, const LatBestParams &lb, hipStream_t stream);
size_t mm_latbest_lds_bytes(int S1p);  // a head + 12 bytes per state: three 32-bit words

// ---- lattice path sampling (mm_latsample_tu.hip: mm_latsample_fwd_kernel, the forward half of mm_latpost_fb_kernel, and
// mm_latsample_kernel, one workgroup per utterance and chunk of MM_LS_CHUNK samples; the workgroup is MM_LATPOST_NT's)
#define MM_LS_CHUNK 64       // samples of a workgroup: one bit each in a state's occupancy mask
#define MM_LS_MAX_CHUNKS 65535  // the grid's y extent
struct LatSampleParams {     // beside a LatPostParams, whose post is fwd (gamma unused)
    long long nsamples;
    unsigned key0, key1;     // the seed's two halves, as SampleParams splits it
    long long *rec;          // [b * rsb + k * rsk + t] the samples' records; NULL: not asked for
    long long rsb, rsk;
    int *path;               // [b * psb + k * psk + t] their source states; NULL: not asked for
    long long psb, psk;
    float *logprob;          // [b * lsb + k]; NULL: not asked for
    long long lsb;
};
// the forward pass in its instance of `nt` threads, then the samples
int mm_launch_latsample(int64_t B, int nt, int max_S1p, const RunParams &p, const LatPostParams &lp, const LatSampleParams &ls, hipStream_t stream);
size_t mm_latsample_lds_bytes(int S1p);  // the larger of the forward pass's (16 bytes per state) and the sampler's (a head + 8 per state)

// ---- posteriors with call-time arc weights (mm_weighted_tu.hip: mm_weights_kernel, mm_log_kernel's forward half on the call's
// descriptors, mm_weighted_bwd_kernel and mm_weighted_scatter_kernel on the item form)
struct UttDesc;  // mm_kernels.hip
struct Slot;     // mm_pack.h
struct WeightDev {  // one utterance's weight form (mm_engine.hip ensure_weight_forms)
    const int *slot2k[2];   // [nslots[d]] slot of the forward / backward item form -> caller entry; -1: the slot keeps the FSM's own
                            // weight (a padding slot, the phony self-loop)
    const int *state2init;  // [S1] state -> its entry of alpha_hat in init_idx order, -1: none
    long long plane_off[2];  // this utterance's first slot in a per-utterance weight plane of each direction
    int nslots[2];
};
struct WeightedParams {
    const ArcDev *arcs;       // [B]
    const WeightDev *wforms;  // [B]
    const UttDesc *utts_own;  // the batch's descriptors
    UttDesc *utts_call;       // [B] the call's descriptors: g[0].slots, g[1].slots and init point at the planes (NULL: no weights given)
    const float *W;           // NULL: the FSMs' own weights
    long long wsb;            // 0: one vector for the batch -- ONE plane, built from utterance 0's form
    const float *W_init;      // NULL: the FSMs' own alpha_hat
    long long wisb;
    Slot *plane[2];           // the call's {col, w} arrays of the forward / backward item forms
    float *init_plane;        // dense alpha_hat in log2 units, per utterance at s1p_prefix (shared: at 0)
    double *acc;              // as ArcParams
    float *post1;
    float *counts;            // NULL: not asked for
    long long csb;
    float *init_counts;       // NULL: not asked for
    long long isb;
    float *ttl;               // NULL: not asked for
};
// LDS bytes of mm_weighted_bwd_kernel: the arc kernel's + one row of state posteriors for the per-pdf pass
size_t mm_weighted_lds_bytes(int S1p, int P1p);
// lds_fwd: the item kernel's plan (the forward half, as mm_launch_arcs launches it); lds_bwd: mm_weighted_lds_bytes of the geometry.
// gamma and its strides go where RunParams says (NULL: not asked for).  p.utts: the batch's own descriptors -- with weights given
// (wp.utts_call != NULL) the prologue runs and the kernels behind it read the call's
int mm_launch_weighted(int64_t B, int NW, int NI, bool bigv, size_t lds_fwd, size_t lds_bwd, const RunParams &p, const WeightedParams &wp,
                       hipStream_t stream);

}  // namespace mm
