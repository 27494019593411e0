// mm_engine.hip -- C ABI (include/markovmodels_amd.h) over the gfx950 kernels.
// Handles, host-side compile (packing), workspace management, launches.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <new>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/markovmodels_amd.h"
#include "mm_kernels.hip"
#include "mm_kernel_quad.hip"
#include "mm_kernel_rows.hip"
#include "mm_internal.h"
#include "mm_pack.h"
#include "mm_rows.h"

using namespace mm;

namespace {
thread_local std::string g_err_store;
}
namespace mm {
int mm_fail(int code, const std::string &msg) {
    g_err_store = msg;
    return code;
}
}  // namespace mm

namespace {

int fail(int code, const std::string &msg) { return mm::mm_fail(code, msg); }

int64_t rd_index(const void *p, int bytes, int64_t i) {
    return bytes == 4 ? int64_t(static_cast<const int32_t *>(p)[i]) : static_cast<const int64_t *>(p)[i];
}
float rd_val(const void *p, int bytes, int64_t i) {
    return bytes == 4 ? static_cast<const float *>(p)[i] : float(static_cast<const double *>(p)[i]);
}

struct Csr {
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<float> val;
};

Csr transpose(const Csr &a, int64_t n) {
    Csr t;
    t.rowptr.assign(n + 1, 0);
    const int64_t nnz = a.rowptr[n];
    t.col.resize(nnz);
    t.val.resize(nnz);
    for (int64_t k = 0; k < nnz; ++k) t.rowptr[a.col[k] + 1]++;
    for (int64_t i = 0; i < n; ++i) t.rowptr[i + 1] += t.rowptr[i];
    std::vector<int64_t> cur(t.rowptr.begin(), t.rowptr.end() - 1);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t k = a.rowptr[r]; k < a.rowptr[r + 1]; ++k) {
            int64_t d = cur[a.col[k]]++;
            t.col[d] = int32_t(r);
            t.val[d] = a.val[k];
        }
    return t;
}

void sort_rows(Csr &a, int64_t n) {
    std::vector<std::pair<int32_t, float>> tmp;
    for (int64_t r = 0; r < n; ++r) {
        int64_t b = a.rowptr[r], e = a.rowptr[r + 1];
        bool sorted = true;
        for (int64_t k = b + 1; k < e; ++k) sorted &= a.col[k - 1] <= a.col[k];
        if (sorted) continue;
        tmp.clear();
        for (int64_t k = b; k < e; ++k) tmp.push_back({a.col[k], a.val[k]});
        std::stable_sort(tmp.begin(), tmp.end(), [](auto &x, auto &y) { return x.first < y.first; });
        for (int64_t k = b; k < e; ++k) {
            a.col[k] = tmp[k - b].first;
            a.val[k] = tmp[k - b].second;
        }
    }
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace

// One hipMalloc, freed with its owner.
struct HipFree {
    void operator()(void *p) const { (void)hipFree(p); }
};
using DevMem = std::unique_ptr<void, HipFree>;

// The quad form of ONE direction of an FSM laid out for KQ quads per lane (mm_pack.h), resident on the device.
struct QuadVariant {
    int KQ = 0, dir = 0;
    QuadGraph g;
    std::vector<float> init_f;      // dir 0: alpha_hat in forward numbering
    std::vector<uint16_t> map_bf;   // dir 1: backward position -> forward position (the alpha store's order)
    std::vector<uint16_t> dist;     // internal numbering
    DevMem blob;
    QuadDev qdev;
    const float *d_init_f = nullptr;
    const unsigned short *d_map_bf = nullptr;
};

// The row-lane form of ONE direction of an FSM (mm_rows.h), resident on the device.
struct RowVariant {
    RowGraph g;
    std::vector<float> init;     // forward: alpha_hat by position
    std::vector<uint32_t> ptab;  // wave form: [4 waves][2 segments][4 addresses + info][64 lanes] (wave_pdf_table)
    int pdf_nps = 0;             // ... segments per wave it uses (1 or 2)
    std::shared_ptr<void> mem;   // its device image: an allocation of its own, or a share of one allocation for many forms
                                 // (mm_fsm_create_many: freed with its last user)
    RowDev rdev;
};
// The forms of one family: both directions ([direction]), the sets of a team ([direction * H + set]), or one.
using RowForms = std::unique_ptr<RowVariant[]>;

struct StreamFree {
    void operator()(StreamForm *s) const { mm_stream_free(s); }
};

// A form that is built at most once per FSM.  `stage` goes to Tried BEFORE the attempt: a form that did not fit, or whose upload
// failed, is not built again.  Packed (the wave forms only): `form` is packed on the host -- by a worker thread -- and waits for the
// calling thread to upload it.
template <class P>
struct Once {
    P form;
    enum : char { New, Packed, Tried } stage = New;
    bool ready() const { return stage == Tried && form; }  // complete and on the device
    bool first(bool *ok) {  // *ok: it is there already; true for the one caller that builds it
        *ok = ready();
        if (stage == Tried) return false;
        stage = Tried;
        return true;
    }
};

struct mm_fsm_s {
    int semiring;
    int64_t S1, nnz;
    int32_t P1;
    int S1p;
    Csr mat[2];   // 0: T_hat' (forward), 1: T_hat (backward); engine-domain weights
    Csr qmat[2];  // the same restricted to the useful states (able to reach the final state AND reachable from an
                  // initial state -- or one of a FEW that are not: mm_fsm_create): the kernels compute posteriors,
                  // to which the other states contribute exactly nothing
    Packed packed[2];      // the item forms: packed when first needed (ensure_packed) -- a numerator graph of the wave kernel never needs them
    std::once_flag packed_once, gen_once;
    // what the generic path's copies are built from when first asked for (gen_build): the matrix as it was handed over
    int gen_layout = 0;
    std::vector<int64_t> raw_ptr;
    std::vector<int32_t> raw_col;
    std::vector<double> raw_val;
    bool fast_ok = false;  // the quad kernel's linear path is valid for this FSM
    // ProbSemiring FSMs in float32 (round 6): the SAME graph in the log semiring -- weights = log of the probabilities -- with all the
    // kernel forms of a log FSM.  mm_pdfposteriors_f32 on a batch of such FSMs takes the logarithm of the likelihoods in one pass, runs
    // the fast kernels on the twins and returns ttl as a probability; the generic entry (mm_pdfposteriors_ex) keeps the FSM as given.
    mm_fsm_s *log_twin = nullptr;
    bool export_ok[2] = {false, false};  // the pruned forms (qmat) give the reference's alpha (0) / beta (1) recursion: see mm_fsm_create
    int depth = 0;         // most arcs from an initial state to any (useful) state
    int64_t nquads[2] = {0, 0};
    std::map<int, std::unique_ptr<QuadVariant>> variants;  // by 2 * KQ + direction; never evicted
    Once<RowForms> rows;    // row-lane forms (mm_kernel_rows.hip)
    Once<RowForms> prows;   // ... and their pair variants (mm_kernel_pairs.hip)
    // split pair forms (mm_rows.h make_rows_split) for teams of 2, 4, 8 (split_hidx), for FSMs beyond the registers / LDS of one
    // compute unit: one team size per FSM -- the first that fits, `split` says which and how
    Once<RowForms> srows[3];
    SplitInfo split;
    Once<RowForms> wrows;   // wave forms (mm_kernel_wave.hip; Packed: wave_pack has run, wave_variants has not)
    Once<DevMem> lane;      // lane form (mm_kernel_lane.hip: up to 64 states): the device image, the LaneDev at its start
    Once<std::unique_ptr<StreamForm, StreamFree>> stream_h[3];  // stream forms (mm_stream.hip: graphs beyond the register-resident forms) for teams of 1, 2, 4 workgroups
    Once<RowForms> vrow;    // Viterbi form (mm_kernel_vit.hip)
    int vit_n4 = 0, vit_n2 = 0;  // its layout: positions of 4 / of 2 arc slots per wave
    // what the generic path (mm_generic.hip: any semiring, float32 or float64) works on: both matrices and alpha_hat as
    // they were handed over, in double, natural units (log weights for Log / Tropical, probabilities for Prob)
    FsmGenView gen;
    std::vector<int64_t> gen_ptr[2];
    std::vector<int32_t> gen_col[2];
    std::vector<double> gen_val[2], gen_init;
    std::vector<float> init;  // dense alpha_hat, engine domain
    std::vector<int32_t> s2p;
    int device = -1;
    DevMem dev_blob;
    size_t dev_bytes = 0;
    GraphDev gdev[2];
    const float *d_init = nullptr;
    const int *d_s2p = nullptr;
    const int *d_pdf_ptr = nullptr, *d_pdf_rows = nullptr;  // pdf -> states (CSR)
    // arc posteriors (MM_LOG): the caller's entry index of every entry of mat[1] (T_hat by source state, columns ascending, ties in
    // the caller's order), the caller's entry of the phony self-loop (-1: none), the states of alpha_hat in init_idx order; the
    // device form (ArcDev::k2slot, ::init_states) is made on the first mm_arcposteriors_f32 call that needs it
    std::vector<int64_t> bwd_caller;
    int64_t kphony = -1;
    std::vector<int32_t> init_order;
    DevMem arc_blob;
    // path sampling (MM_LOG): the sampling form -- T_hat' by destination as SampleRec lists, parallel entries merged -- made on the
    // first mm_samplepaths_f32 call that needs it; the list of the phony final state (the omega column)
    DevMem samp_blob;
    int samp_fin_start = 0, samp_fin_deg = 0;
    // leaky posteriors (MM_LOG): the leak rows -- rho(j) = (+)_k alpha_hat(k) T_hat(k, j), log2 domain, [S1] -- made on the first
    // mm_leakyposteriors_f32 call that needs them
    DevMem leak_blob;
    // posteriors with call-time weights (MM_LOG): the weight form -- slot -> caller entry of both item forms, state -> entry of
    // alpha_hat -- made on the first mm_weightedposteriors_f32 call that needs it
    DevMem weight_blob;
};

// Test/diagnostic switches.  Read from the environment at mm_batch_create (and once per process for the entries that have no
// batch: process_debug_opts), and only when MM_DEBUG is set: the run entry points never call getenv, and no environment variable
// changes what a production process computes or packs.  MM_KERNEL = item | quad | row | pair forces a pdfposteriors kernel,
// MM_KQ / MM_NWAVES / MM_NITEMS force a geometry, MM_NO_XCSR keeps the exact-fallback CSR out of LDS,
// MM_VERBOSE prints the packing statistics.
struct DebugOpts {
    enum { K_AUTO = 0, K_ITEM, K_QUAD, K_ROW, K_PAIR, K_WAVE, K_SPLIT, K_LANE, K_STREAM };
    int kernel = K_AUTO;
    int kq = 0, nwaves = 0, nitems = -1;
    bool no_xcsr = false, verbose = false;
    bool no_redo = false;           // MM_NO_REDO: the exact kernels do not run after the fast ones (what the fast path alone computes)
    bool no_dpair = false;          // MM_NO_DPAIR: no float64 pair kernels (marked utterances go straight to the quad / item kernels)
    bool bankopt = false;           // MM_BANKOPT: the pair forms choose the banks of their rows (RowPackOpts::bank_opt; an experiment, off by default)
    bool no_wpair = false;          // MM_NO_WPAIR: a whole batch on the exact kernels runs the one-utterance float64 kernels, not the wide pair kernels
    bool no_fallback = false;       // MM_NO_FALLBACK: the float64 pair kernels run, the log-domain kernels behind them do not
    int stream_h = 0;               // MM_STREAM_H: workgroups of a team of the stream kernels (0: by the batch size)
    bool no_pdf_halves = false;     // MM_NO_PDF_HALVES: the packer does not deal a segment's rows to its half-waves by the bank pair of their pdf
    int wave_place = -1;            // MM_WAVE_PLACE: placement mode of the wave forms (-1: the packer's default)
    int exact_first = -1;           // MM_EXACT_FIRST=0/1: never / always skip the float32 pair kernels (default: by the last call's marks)
    bool bigv = false;              // MM_BIGV: item / tropical kernels with the state vectors in global memory whatever the size
    int finish_cost = 0;            // MM_FINISH_COST: cost model of the pair forms (0: default)
    int split_q10 = 0;              // MM_SPLIT_Q10: where the pair kernels cut the frames between the agents (1024ths; 0: the engine's choice)
    int x_sleep = 8;                // MM_SPLIT_SLEEP: split kernels, 64-clock units the exchange wave sleeps before a step's first poll
    float group_speed[4] = {0, 0, 0, 0};  // MM_GROUP_SPEED=a,b,c,d
    int latpost_nt = 0;             // MM_LATPOST_NT: threads of mm_latpost_fb_kernel's workgroup (256, 512, 1024; 0: MM_LATPOST_NT of mm_internal.h)
    bool sample_nostage = false;    // MM_SAMPLE_NOSTAGE: mm_sample_kernel gathers alpha~ from global memory whatever the size (a measurement aid)
};
static DebugOpts read_debug_opts() {
    DebugOpts d;
    const char *on = getenv("MM_DEBUG");
    if (!on || !*on || !strcmp(on, "0")) return d;
    if (const char *e = getenv("MM_KERNEL"))
        d.kernel = !strcmp(e, "item") ? DebugOpts::K_ITEM : !strcmp(e, "quad") ? DebugOpts::K_QUAD
                 : !strcmp(e, "row") ? DebugOpts::K_ROW : !strcmp(e, "pair") ? DebugOpts::K_PAIR : !strcmp(e, "wave") ? DebugOpts::K_WAVE : !strcmp(e, "split") ? DebugOpts::K_SPLIT : !strcmp(e, "lane") ? DebugOpts::K_LANE : !strcmp(e, "stream") ? DebugOpts::K_STREAM : DebugOpts::K_AUTO;
    if (const char *e = getenv("MM_KQ")) d.kq = atoi(e);
    if (const char *e = getenv("MM_NWAVES")) d.nwaves = atoi(e);
    if (const char *e = getenv("MM_NITEMS")) d.nitems = atoi(e);
    d.no_xcsr = getenv("MM_NO_XCSR") != nullptr;
    d.verbose = getenv("MM_VERBOSE") != nullptr;
    d.bigv = getenv("MM_BIGV") != nullptr;
    d.sample_nostage = getenv("MM_SAMPLE_NOSTAGE") != nullptr;
    d.no_redo = getenv("MM_NO_REDO") != nullptr;
    d.no_dpair = getenv("MM_NO_DPAIR") != nullptr;
    d.no_wpair = getenv("MM_NO_WPAIR") != nullptr;
    d.bankopt = getenv("MM_BANKOPT") != nullptr;
    d.no_fallback = getenv("MM_NO_FALLBACK") != nullptr;
    d.no_pdf_halves = getenv("MM_NO_PDF_HALVES") != nullptr;
    if (const char *e = getenv("MM_STREAM_H")) d.stream_h = atoi(e);
    if (const char *e = getenv("MM_WAVE_PLACE")) d.wave_place = atoi(e);
    if (const char *e = getenv("MM_EXACT_FIRST")) d.exact_first = atoi(e) != 0;
    if (const char *e = getenv("MM_FINISH_COST")) d.finish_cost = atoi(e);
    if (const char *e = getenv("MM_SPLIT_SLEEP")) d.x_sleep = atoi(e);
    if (const char *e = getenv("MM_SPLIT_Q10")) d.split_q10 = atoi(e);
    if (const char *e = getenv("MM_LATPOST_NT")) d.latpost_nt = atoi(e);
    if (const char *e = getenv("MM_GROUP_SPEED")) sscanf(e, "%f,%f,%f,%f", &d.group_speed[0], &d.group_speed[1], &d.group_speed[2], &d.group_speed[3]);
    return d;
}

// (entries without a batch -- mm_fsm_create_many's packing, the host-only test aids: the switches as the process started with them)
static const DebugOpts &process_debug_opts() {
    static const DebugOpts d = read_debug_opts();
    return d;
}

// The kernels mm_pdfposteriors_f32 launches first on a log batch (pick_family).  Quad and Item: none of the linear-domain families
// takes the batch; the quad kernels where they are usable (mm_batch_s::quad_ok), else the item kernel.
enum class Fb { Item, Quad, Rows, Pairs, Split, Lane, Wave, Stream };

struct mm_batch_s {
    DebugOpts dbg;
    std::vector<mm_fsm_t> fsms;
    int semiring;
    int64_t B;
    int64_t total_states = 0;
    int64_t total_s1p = 0;
    int max_S1p = 0, max_P1 = 0, max_items = 0;
    int max_quads[2] = {0, 0};  // per direction (0 forward, 1 backward)
    int max_depth = 0;     // deepest FSM of the batch (mm_fsm_s::depth)
    int64_t max_xcsr = 0;  // floats of the largest exact-fallback CSR (rowptr + col + w) of the batch
    int xcsr = 0;          // floats of LDS reserved for it (0: it stays in global memory)
    bool fast_ok = true;
    int geo_kq[2] = {0, 0}, geo_nw[2] = {1, 1};  // quad kernel geometry of the forward and the backward kernel
    Fb fb = Fb::Item;
    bool quad_ok = false;  // the quad kernels run where the item kernel would: first (Quad), and after the rows, pair and float64 kernels
    int row_ka[2] = {0, 0}, row_nwc[2] = {1, 1}, row_slotrows[2] = {0, 0};
    int pair_ka = 0, pair_nwc = 1, pair_slotrows = 0;
    bool vit_ok = false;   // every FSM has its Viterbi form: mm_vit_kernel + mm_vit_backtrace_kernel can run
    int vit_n4 = 0, vit_n2 = 0, vit_arcs = 0;
    int lane_S = 0;        // (lane kernel) the most states of one FSM
    bool lane_redo_wave = false;  // ... every FSM has its wave forms too: what the lane kernel marks goes to the wave kernel (else: the item kernel)
    int wave_nseg = 0;
    int pair_H = 1;        // workgroups per team: 1 = the pair kernels proper (Pairs), > 1 = the split pair kernels (Split)
    int split_s1p = 0;     // floats / 2 of a stored vector of the split kernels (positions of the team's vector, padded)
    bool deterministic = false;  // mm_batch_set_deterministic(): no float atomics in the item kernel
    float lt_floor = -20.f;      // mm_batch_set_posterior_floor(): smallest accepted log2 overlap of a frame (mm_pair_finish_kernel)
    float g_scale = 1.f;         // mm_batch_set_gamma_mode(): gamma_out = g_scale * gamma, or (g_acc) gamma_out += g_scale * gamma
    bool g_acc = false;
    bool keep_marks = false;     // mm_batch_set_mark_policy(MM_MARKS_KEEP): a range mark is never cleared by the finish kernels' two criteria
    float *ws_big = nullptr;  // [B][4 * max_S1p]: state vectors of FSMs beyond the LDS (launch())
    int device = -1;
    int n_cus = 256;  // compute units of the device
    UttDesc *d_utts = nullptr;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    const int *last_redo = nullptr;  // redo marks of the last pdfposteriors call (inside ws; mm_batch_last_redo_count)
    const double *last_z = nullptr;  // ... and the pair kernels' per-utterance normaliser statistics
    GenScratch gen;                  // the generic entry's workspace and descriptors (mm_generic.hip)
    // The float64 exact pair kernels (mm_kernel_dpair.hip) take the utterances the float32 pair kernels mark -- and the whole
    // batch, the float32 kernels skipped, while the inputs are "hard": more than a quarter of the last finished call's
    // utterances were beyond the float32 kernels (stat_host, written by the finish kernels; read without synchronising).
    std::vector<UttDesc> utts_host;     // what d_utts holds
    bool items_resident = true;         // the FSMs' item forms are on the device (a batch of the wave kernel uploads them on first need)
    bool dpair_ok = false;
    int stream_S1 = 0, stream_H = 1;    // (stream kernels) the most states of one FSM; workgroups of a team (mm_stream_pick_h)
    bool wpair_ok = false;              // a whole batch on the exact kernels fits the wide pair kernels (mm_kernel_wpair.hip: two utterances per workgroup)
    bool quad_built = false;            // the FSMs' quad forms exist (not built for batches whose exact path is the float64 kernels)
    int *stat_dev = nullptr;            // {count, ticket, team workgroups whose team sits on ONE XCD, team workgroups} (the last two: mm_batch_team_xcd_stats)
    bool xcd_counting = false;          // ... counted by the team kernels since mm_batch_team_xcd_stats was first called (a measurement aid: off until asked for)
    volatile int *stat_host = nullptr;  // pinned: {count of hard utterances, sequence number of the call that counted, marks of the last alpha / beta export}
    unsigned export_calls[2] = {0, 0};  // alpha / beta exports on this batch (every 32nd tries the linear-domain kernels again)
    int stat_seq = 0;
    int exact_first = -1;               // MM_EXACT_FIRST (under MM_DEBUG): 0 / 1 force the choice, -1: by the statistics
    bool last_exact_first = false;      // what the last call did
    const int *last_redo2 = nullptr;    // marks the float64 kernels left for the log-domain kernels (mm_batch_last_fallback_count)
    // a batch of ProbSemiring FSMs that all have their log twins: the batch of the twins (what mm_pdfposteriors_f32 runs), and the
    // logarithms of the call's likelihoods [B][N][P]
    mm_batch_s *log_twin = nullptr;
    float *prob_logv = nullptr;
    size_t prob_logv_bytes = 0;
    // arc posteriors (mm_arcposteriors_f32): the utterances' ArcDev descriptors on the device (made on the first call), the float64
    // sums of all their backward slots, the most caller entries / initial states of one FSM
    DevMem d_arcs;
    int64_t arc_slots = 0, arc_max_nnz = 0, arc_max_init = 0;
    // path sampling (mm_samplepaths_f32): the utterances' SampleDev descriptors on the device (made on the first call)
    DevMem d_samp;
    // leaky posteriors (mm_leakyposteriors_f32): the utterances' LeakDev descriptors on the device (made on the first call)
    DevMem d_leak;
    // posteriors with call-time weights (mm_weightedposteriors_f32): the utterances' WeightDev descriptors on the device (made on the
    // first call), the slots of all their forward / backward item forms (what a weight plane per utterance holds)
    DevMem d_wforms;
    int64_t w_slots[2] = {0, 0};
    // arc-class posteriors (mm_arcclassposteriors_f32): the class plan mm_batch_set_arc_classes made on the host -- the utterances'
    // ClassDev descriptors (pointers as byte offsets into the image until it is uploaded) in front of the records and class
    // pointers of every distinct (FSM, class array) --, its copy on the device (made by the first call behind a new plan), the
    // classes, the most ranks of one utterance and the ranks of all
    std::vector<char> cls_image;
    DevMem d_cls;
    // ... and, for mm_scoredposteriors_f32, the class planes of the same plan: the utterances' ScoredDev descriptors in front of the
    // planes of both item forms and the ranks' classes of every distinct (FSM, class array); made and replaced with the plan (empty:
    // more classes than a 16-bit id holds), on the device from the first scored call behind it
    std::vector<char> sc_image;
    DevMem d_sc;
    // lattices (mm_lattice_f32, tropical batches): the utterances' LatticeDev descriptors in front of the three arc planes of every
    // distinct FSM, on the device from the first call
    DevMem d_lat;
    int cls_C = 0;
    int64_t cls_max_M = 0, cls_terms = 0;
    // the lanes a class's sum runs on (ClassDev::lgl, a bit per value), over the utterances of the plan: what kernels() names
    uint32_t cls_lgl_mask = 0;
};

static bool on_pairs(mm_batch_t h) { return h->fb == Fb::Pairs || h->fb == Fb::Split; }

static bool capturing(void *stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return stream && hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// what every run entry hands its kernels: the utterances, their log-likelihoods V[b][n][p] and lengths, the frames
static RunParams run_params(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N) {
    RunParams p{};
    p.utts = h->d_utts;
    p.V = V;
    p.vsb = vsb;
    p.vsn = vsn;
    p.lens = lens;
    p.N = int(N);
    p.B = int(h->B);
    return p;
}

// (team kernels) ticks of s_memrealtime a poll waits before it gives the team up
static unsigned long long x_timeout(int64_t N) {
    return std::min<unsigned long long>(10000000ull, std::max<unsigned long long>(200000ull, 1000ull * (unsigned long long)N));
}

#ifdef MM_STAMPS
static unsigned long long *g_dbg = nullptr;
static size_t g_dbg_n = 0;
#endif
// (diagnostic build) where the kernels add their per-wave phase cycle sums
static void bind_stamps(mm_batch_t h, RunParams &p) {
#ifdef MM_STAMPS
    if (!g_dbg) {
        g_dbg_n = size_t(16) * MM_MAX_WAVES * size_t(h->B);
        (void)hipMalloc(&g_dbg, sizeof(unsigned long long) * g_dbg_n);
    }
    p.dbg = g_dbg;
#endif
}

static PairLaunch pair_launch_of(mm_batch_t h) {
    PairLaunch pl;
    pl.B = h->B;
    pl.nwc = h->pair_nwc;
    pl.slotrows = h->pair_slotrows;
    pl.max_P1 = h->max_P1;
    pl.pair_ka = h->pair_ka;
    pl.H = h->pair_H;
    pl.small = h->pair_H == 1 && h->max_S1p <= 128;
    return pl;
}

static WaveLaunch wave_launch_of(mm_batch_t h) {
    WaveLaunch wl;
    wl.B = h->B;
    wl.nseg = h->wave_nseg;
    wl.max_P1 = h->max_P1;
    wl.n_cus = h->n_cus;
    return wl;
}

// Launch geometry of the item kernels: NW waves per workgroup, NI register-resident items per wave
// (mm_kernels.hip, "Register-resident graph"; 8 items keep 16 waves per CU inside the 128-VGPR
// budget), the remaining items are streamed from L2.
struct Geometry {
    int NW, NI;
};

static Geometry pick_geometry(mm_batch_t h) {
    Geometry g{16, 8};
    const int it = h->max_items;
    // one workgroup per CU whatever its size: spread the items over as many waves as there are items
    g.NW = std::max(1, std::min(MM_MAX_WAVES, it + 1));  // + one wave without items: it normalises the frames (FB)
    if (h->dbg.nwaves >= 1 && h->dbg.nwaves <= MM_MAX_WAVES) g.NW = h->dbg.nwaves;
    if (h->dbg.nitems == 0 || h->dbg.nitems == 8) g.NI = h->dbg.nitems;
    if (h->max_S1p > 65534) g.NI = 0;  // (resident items hold 16-bit state indices)
    return g;
}

// ---- one plan per entry that runs on the item form: its launch geometry and where its state vectors live
enum class ItemEntry { Fb, Export, Tropical, Arcs, Sample, Cost, Leaky, Entropy, Filter, Window, VitWindow, Weighted, Segment, ArcClass, Scored, ClassCost, ClassPath, Lattice };
struct ItemPlan {
    ItemEntry e;
    int NW, NI;        // waves per workgroup, register-resident items per wave of the instance (8 or 0)
    bool global;       // the state vectors in global memory (BIGV), else in LDS
    bool stage;        // (Sample) mm_sample_kernel keeps two alpha~ rows in LDS, else it gathers them from global memory
    size_t lds_bytes;  // dynamic LDS of the chosen placement (Arcs, ArcClass: of the forward kernel; mm_arc_kernel adds MM_ARC_LDS_EXTRA,
                       // mm_arcclass_kernel that and its term rows;
                       // Weighted: of mm_weighted_bwd_kernel -- its forward launch takes the item kernel's plan, as the arc entry's)
};
// The only source of the above.  The vectors are global when the entry's LDS plan (the item kernel's, with the stage rows for
// all but the export modes, + the arc kernel's extra; Cost: cost_lds_plan; Leaky: leaky_lds_plan; Entropy: entropy_lds_plan; Filter:
// filter_lds_plan, no larger than the export modes'; Window and Segment: window_lds_plan, the arc kernel's size) does not fit 160 KB, when
// MM_BIGV asks for it, or for the arc, sampling, cost, leaky, entropy, filter, window and segment kernels when NI = 0: they have no
// streamed-only instance with the vectors in LDS.  VitWindow (tropical batches): the tropical kernel's geometry, its LDS plan + the
// arc kernel's extra.  Weighted: the arc kernel's size + one row of state posteriors (mm_weighted_lds_bytes), 8 waves like Arcs.
// ArcClass: the arc entry's plan (its term rows take what LDS the plan leaves, or the workspace: arcclass_cap).
// Scored: the arc entry's plan as well; the two score rows come behind it (scored_class_cap), the term rows behind them (scored_term_cap).
// ClassCost: the cost entry's plan; the two cost rows come behind it (classcost_class_cap).
// ClassPath (tropical batches): the tropical kernel's geometry, its LDS plan + the two 16-bit class rows; the two score rows come
// behind them (classpath_class_cap).
// Lattice (tropical batches): the tropical kernel's plan as it stands -- the forward recursion of mm_lattice_f32 is launch_tropical's; the
// prune kernel has a placement of its own (lattice_global).
// `global` never depends on max_items, nor does NI except Tropical's (8: the whole graph is register-resident): mm_batch_create
// asks before the item forms are up, and ensure_item_forms raises max_items later -- only NW follows it.
static ItemPlan item_plan(mm_batch_t h, ItemEntry e) {
    const size_t lds_max = MM_LDS_MAX;
    const Geometry g = pick_geometry(h);
    const int P1p = (h->max_P1 + 3) & ~3;
    auto bytes = [&](int S1p) {
        if (e == ItemEntry::Leaky) return mm_leaky_lds_bytes(S1p, P1p);
        if (e == ItemEntry::Entropy) return mm_entropy_lds_bytes(S1p, P1p);
        if (e == ItemEntry::Filter) return mm_filter_lds_bytes(S1p, P1p);
        if (e == ItemEntry::Window || e == ItemEntry::Segment) return mm_window_lds_bytes(S1p, P1p);
        if (e == ItemEntry::VitWindow) return mm_vitwindow_lds_bytes(S1p, P1p);
        if (e == ItemEntry::ClassPath) return mm_classpath_lds_bytes(S1p, P1p);
        if (e == ItemEntry::Weighted) return mm_weighted_lds_bytes(S1p, P1p);
        return e == ItemEntry::Cost || e == ItemEntry::ClassCost ? mm_cost_lds_bytes(S1p, P1p) : size_t(lds_plan(S1p, P1p, e != ItemEntry::Export).total) * 4;
    };
    const bool derived = e == ItemEntry::Arcs || e == ItemEntry::Sample || e == ItemEntry::Cost || e == ItemEntry::Leaky || e == ItemEntry::Entropy ||
                         e == ItemEntry::Filter || e == ItemEntry::Window || e == ItemEntry::Weighted || e == ItemEntry::Segment || e == ItemEntry::ArcClass || e == ItemEntry::Scored ||
                         e == ItemEntry::ClassCost;
    ItemPlan pl{e, g.NW, g.NI, false, false, 0};
    pl.global = bytes(h->max_S1p) + (e == ItemEntry::Arcs || e == ItemEntry::ArcClass || e == ItemEntry::Scored ? MM_ARC_LDS_EXTRA : 0) > lds_max || h->dbg.bigv || (derived && g.NI == 0);
    pl.lds_bytes = bytes(pl.global ? 0 : h->max_S1p);
    // (8 items' arcs and their sums / the pair arithmetic / the leak term and its sums per wave: compiled for 8 waves per CU)
    if (e == ItemEntry::Arcs || e == ItemEntry::Cost || e == ItemEntry::Leaky || e == ItemEntry::Entropy || e == ItemEntry::Filter ||
        e == ItemEntry::Window || e == ItemEntry::Weighted || e == ItemEntry::Segment || e == ItemEntry::ArcClass || e == ItemEntry::Scored ||
        e == ItemEntry::ClassCost)
        pl.NW = std::min(g.NW, 8);
    if (e == ItemEntry::Sample) pl.stage = !pl.global && !h->dbg.sample_nostage && size_t(h->max_S1p) * 8 <= lds_max;
    if (e == ItemEntry::Tropical || e == ItemEntry::VitWindow || e == ItemEntry::ClassPath || e == ItemEntry::Lattice) {
        // register-resident items when the whole graph fits 8 items per wave -- as many waves as there is work for (latency), at most
        // 8 items each --, else streamed
        pl.NI = g.NI == 8 && h->max_items <= 8 * MM_MAX_WAVES ? 8 : 0;
        pl.NW = pl.NI ? std::min(MM_MAX_WAVES, std::max(g.NW, (h->max_items + 3) / 4)) : 16;
        if (pl.NI && h->dbg.nwaves >= g.NW && h->dbg.nwaves <= MM_MAX_WAVES) pl.NW = h->dbg.nwaves;
    }
    return pl;
}
// ... for an entry about to launch: refuses what the plan cannot run.  (Cost and Entropy keep their global vectors in the workspace
// at 8 floats per state, the others in h->ws_big at 4: bind_big, ItemWs)
static bool ws_holds_big(ItemEntry e) { return e == ItemEntry::Cost || e == ItemEntry::Entropy || e == ItemEntry::ClassCost; }
static int item_plan_check(mm_batch_t h, const ItemPlan &pl) {
    if (pl.global && !ws_holds_big(pl.e) && !h->ws_big)
        return fail(MM_ERR_UNSUPPORTED, "FSM too large for the LDS and no global-memory vectors were allocated");
    return pl.lds_bytes > MM_LDS_MAX ? fail(MM_ERR_UNSUPPORTED, "too many pdfs for the LDS: " + std::to_string(h->max_P1)) : int(MM_OK);
}
static void bind_big(mm_batch_t h, const ItemPlan &pl, RunParams &p) {
    if (!pl.global || ws_holds_big(pl.e)) return;
    p.ws_big = h->ws_big;
    p.big_stride = 4ll * h->max_S1p;
}
static const char *where_of(bool global) { return global ? "global" : "lds"; }
// the most ranks of one utterance whose two term rows mm_arcclass_kernel keeps in LDS, behind the arc kernel's plan
static int64_t arcclass_cap(const ItemPlan &pl) {
    const size_t used = pl.lds_bytes + MM_ARC_LDS_EXTRA;
    return used >= MM_LDS_MAX ? 0 : int64_t((MM_LDS_MAX - used) / (2 * sizeof(float)));
}

// mm_scoredposteriors_f32: the most classes whose two score rows (C + 1 floats each, padded to 4) fit the LDS behind the arc kernel's
// plan -- and a 16-bit class id --, and the most ranks of one utterance whose two term rows fit behind the score rows of C classes
static int64_t scored_class_cap(const ItemPlan &pl) {
    const size_t used = pl.lds_bytes + MM_ARC_LDS_EXTRA;
    if (used + 2 * 4 * sizeof(float) > MM_LDS_MAX) return 0;
    const int64_t row = int64_t((MM_LDS_MAX - used) / (2 * sizeof(float))) & ~int64_t(3);  // floats of one row
    return std::min<int64_t>(row - 1, 65534);
}
static size_t scored_lds_bytes(const ItemPlan &pl, int64_t C) { return pl.lds_bytes + MM_ARC_LDS_EXTRA + size_t(mm_scored_urow(C)) * 2 * sizeof(float); }
static int64_t scored_term_cap(const ItemPlan &pl, int64_t C) {
    const size_t used = scored_lds_bytes(pl, C);
    return used >= MM_LDS_MAX ? 0 : int64_t((MM_LDS_MAX - used) / (2 * sizeof(float)));
}

// mm_classcost_f32: the most classes whose two cost rows (C + 1 floats each, padded to 4) fit the LDS behind the cost kernels' plan
// -- and a 16-bit class id
static int64_t classcost_class_cap(const ItemPlan &pl) {
    if (pl.lds_bytes + 2 * 4 * sizeof(float) > MM_LDS_MAX) return 0;
    const int64_t row = int64_t((MM_LDS_MAX - pl.lds_bytes) / (2 * sizeof(float))) & ~int64_t(3);  // floats of one row
    return std::min<int64_t>(row - 1, 65534);
}
static size_t classcost_lds_bytes(const ItemPlan &pl, int64_t C) { return pl.lds_bytes + size_t(mm_scored_urow(C)) * 2 * sizeof(float); }

// mm_classpath_f32: the most classes whose two score rows fit the LDS behind the forward kernel's plan -- and a 16-bit class id
static int64_t classpath_class_cap(const ItemPlan &pl) { return classcost_class_cap(pl); }
static size_t classpath_lds_bytes(const ItemPlan &pl, int64_t C, bool scored) { return pl.lds_bytes + (scored ? size_t(mm_scored_urow(C)) * 2 * sizeof(float) : 0); }

// mm_lattice_f32: the prune kernel gathers the two rows of a cell from global memory when they do not fit the LDS, or under MM_BIGV
static bool lattice_global(mm_batch_t h) { return h->dbg.bigv || mm_lattice_lds_bytes(h->max_S1p) > MM_LDS_MAX; }

// mm_latticeposteriors_f32: the workgroup of its forward-backward, and the states its three per-state LDS arrays hold
static int latpost_nt(mm_batch_t h) { return h->dbg.latpost_nt ? h->dbg.latpost_nt : MM_LATPOST_NT; }
static int64_t latpost_state_cap() { return int64_t((MM_LDS_MAX - mm_latpost_lds_bytes(0)) / (mm_latpost_lds_bytes(1) - mm_latpost_lds_bytes(0))); }
// mm_latticecost_f32: the same workgroup, five per-state LDS arrays
static int64_t latcost_state_cap() { return int64_t((MM_LDS_MAX - mm_latcost_lds_bytes(0)) / (mm_latcost_lds_bytes(1) - mm_latcost_lds_bytes(0))); }
// mm_latticebest_f32: the same workgroup, three per-state LDS words
static int64_t latbest_state_cap() { return int64_t((MM_LDS_MAX - mm_latbest_lds_bytes(0)) / (mm_latbest_lds_bytes(1) - mm_latbest_lds_bytes(0))); }
// mm_latticesample_f32: its forward pass is mm_latticeposteriors_f32's, and the draw needs less
static int64_t latsample_state_cap() { return latpost_state_cap(); }

// item / tropical kernels: `kernel` keeps the state vectors in LDS; `big` is the same kernel with the vectors in global
// memory, for FSMs beyond the LDS (the reference has no size limit: src/linalg.jl:170-181)
static int fsm_to_device(mm_fsm_t f);
// The item forms of a batch that was created without them (a batch of the wave kernel): upload them and refresh the
// utterance descriptors, once, when an entry that runs the item / tropical kernels is first called on the batch.
static int ensure_item_forms(mm_batch_t h, void *stream) {
    if (h->items_resident) return MM_OK;
    if (capturing(stream))
        return fail(MM_ERR_INVALID, "the item forms of this batch are not on the device yet: run the entry once outside a stream capture");
    for (int64_t b = 0; b < h->B; ++b) {
        mm_fsm_t f = h->fsms[size_t(b)];
        int rc = fsm_to_device(f);
        if (rc) return rc;
        UttDesc &u = h->utts_host[size_t(b)];
        u.g[0] = f->gdev[0];
        u.g[1] = f->gdev[1];
        u.init = f->d_init;
        u.s2p = f->d_s2p;
        u.pdf_ptr = f->d_pdf_ptr;
        u.pdf_rows = f->d_pdf_rows;
        h->max_items = std::max(h->max_items, int(std::max(f->packed[0].items.size(), f->packed[1].items.size())));
    }
    // (every other field keeps its value: a kernel still reading the descriptors sees the same bytes)
    HIP_TRY(hipMemcpy(h->d_utts, h->utts_host.data(), sizeof(UttDesc) * size_t(h->B), hipMemcpyHostToDevice));
    h->items_resident = true;
    return MM_OK;
}

// (NW is the caller's: launch_log and launch_tropical read their plan BEFORE the item forms of a batch created without them are
// up, so the first call on such a batch runs with fewer waves than the later ones)
template <typename K>
static int launch(K kernel, K big, mm_batch_t h, const RunParams &p0, ItemEntry e, int NW, void *stream) {
    int rc = ensure_item_forms(h, stream);
    if (rc) return rc;
    const ItemPlan pl = item_plan(h, e);
    rc = item_plan_check(h, pl);
    if (rc) return rc;
    RunParams p = p0;
    p.deterministic = h->deterministic ? 1 : 0;
    if (pl.global) kernel = big;
    bind_big(h, pl, p);
    return mm_launch(kernel, dim3(unsigned(h->B)), dim3(64 * NW), pl.lds_bytes, static_cast<hipStream_t>(stream), p);
}

template <int MODE, bool TROP = false>
static int launch_log(mm_batch_t h, const RunParams &p, void *stream) {
    const ItemEntry e = MODE == MODE_FB ? ItemEntry::Fb : ItemEntry::Export;
    const ItemPlan g = item_plan(h, e);
    if (MODE == MODE_FB && g.NI != 0) {  // forward kernel, then backward kernel on the same stream
        int rc = launch(mm_log_kernel<MODE, 8, 1, TROP, false>, mm_log_kernel<MODE, 8, 1, TROP, true>, h, p, e, g.NW, stream);
        if (rc) return rc;
        return launch(mm_log_kernel<MODE, 8, 2, TROP, false>, mm_log_kernel<MODE, 8, 2, TROP, true>, h, p, e, g.NW, stream);
    }
    switch (g.NI) {
        case 0: return launch(mm_log_kernel<MODE, 0, 0, TROP, false>, mm_log_kernel<MODE, 0, 0, TROP, true>, h, p, e, g.NW, stream);
        default: return launch(mm_log_kernel<MODE, 8, 0, TROP, false>, mm_log_kernel<MODE, 8, 0, TROP, true>, h, p, e, g.NW, stream);
    }
}

// The quad kernels (mm_kernel_quad.hip): KQ register-resident quads per lane, NW waves; one kernel per
// direction (PASS 0: forward, 1: backward), each with the geometry its own matrix needs.
static size_t quad_lds_bytes(mm_batch_t h, int dir) {
    const int P1p = (h->max_P1 + 3) & ~3, KQ = h->geo_kq[dir], NW = h->geo_nw[dir];
    const int vl = (h->max_quads[dir] + KQ - 1) / KQ;
    return (size_t(lds_plan_q(h->max_S1p, P1p, std::max(vl, 64 * NW) * KQ).total) + size_t(h->xcsr)) * 4;
}

// (batch creation: h->quad_ok.  No quad forms are built for the lane, wave and stream kernels, nor without fast_ok)
static bool quad_kernel_usable(mm_batch_t h) {
    if (h->dbg.kernel == DebugOpts::K_ITEM || !h->quad_built || h->geo_kq[0] < 1 || h->geo_kq[1] < 1) return false;
    // small deep graphs (numerators): measured on the reference's WSJ numerator graph (depth 165),
    // item kernel 2.3 ms against 2.7 ms; shallow graphs of the same size are 1.6x faster on the quad kernels
    if (h->max_depth >= 64 && h->geo_kq[0] <= 3 && h->geo_kq[1] <= 3 && h->dbg.kernel == DebugOpts::K_AUTO) return false;
    return quad_lds_bytes(h, 0) <= MM_LDS_MAX && quad_lds_bytes(h, 1) <= MM_LDS_MAX;
}

// (the quad kernels' instances live in mm_quad_tu.hip)
template <int PASS>
static int launch_quad_pass(mm_batch_t h, const RunParams &p, void *stream) {
    QuadLaunch ql;
    ql.B = h->B;
    ql.kq = h->geo_kq[PASS];
    ql.nw = h->geo_nw[PASS];
    ql.max_S1p = h->max_S1p;
    ql.lds = quad_lds_bytes(h, PASS);
    return mm_launch_quad_pass(PASS, ql, p, static_cast<hipStream_t>(stream));
}

// forward kernel, then backward kernel on the same stream: alpha, the per-frame normalisers and log Z travel
// through the workspace
static int launch_quad(mm_batch_t h, const RunParams &p, void *stream) {
    int rc = launch_quad_pass<0>(h, p, stream);
    if (rc) return rc;
    return launch_quad_pass<1>(h, p, stream);
}

static int launch_tropical(mm_batch_t h, const RunParams &p, void *stream) {
    const ItemPlan pl = item_plan(h, ItemEntry::Tropical);
    if (pl.NI == 8) return launch(mm_tropical_kernel<8, false>, mm_tropical_kernel<8, true>, h, p, pl.e, pl.NW, stream);
    return launch(mm_tropical_kernel<0, false>, mm_tropical_kernel<0, true>, h, p, pl.e, pl.NW, stream);
}

// The row kernels (mm_kernel_rows.hip): KA register-resident arcs per lane, NWC compute waves + 1 service wave.
static const int kRowKA[] = {24, 40, 42, 44};  // instantiated register windows (48 arcs per lane spill)

template <int KA, int PASS>
static int launch_row_ka(mm_batch_t h, const RunParams &p, void *stream) {
    const size_t lds = row_lds_bytes(MM_ROW_RS, PASS, h->row_slotrows[PASS]);
    if (lds > MM_LDS_MAX) return fail(MM_ERR_UNSUPPORTED, "row kernel: LDS");
    return mm_launch(mm_fbr_kernel<KA, MM_ROW_RS, PASS>, dim3(unsigned(h->B)), dim3(64 * (h->row_nwc[PASS] + 1)), lds, static_cast<hipStream_t>(stream), p);
}
template <int PASS>
static int launch_row_pass(mm_batch_t h, const RunParams &p, void *stream) {
    const int ka = h->row_ka[PASS];
    if (ka <= 24) return launch_row_ka<24, PASS>(h, p, stream);
    if (ka <= 40) return launch_row_ka<40, PASS>(h, p, stream);
    if (ka <= 42) return launch_row_ka<42, PASS>(h, p, stream);
    if (ka <= 44) return launch_row_ka<44, PASS>(h, p, stream);
    return MM_ERR_UNSUPPORTED;
}
static int launch_rows(mm_batch_t h, const RunParams &p, void *stream) {
    int rc = launch_row_pass<0>(h, p, stream);
    if (rc) return rc;
    return launch_row_pass<1>(h, p, stream);
}

// The pair kernels live in a translation unit of their own (mm_pairs_tu.hip)
static int launch_pairs(mm_batch_t h, const RunParams &p, void *stream) {
    const PairLaunch pl = pair_launch_of(h);
    return h->pair_H > 1 ? mm_launch_split(pl, p, static_cast<hipStream_t>(stream)) : mm_launch_pairs(pl, p, static_cast<hipStream_t>(stream));
}

namespace {
// one device allocation per FSM: sections appended with 256-byte alignment
struct Blob {
    std::vector<char> host;
    // (mm_fsm_create_many) sizes only (dry), or written straight into a staging buffer shared by many forms (ext)
    bool dry = false;
    char *ext = nullptr;
    size_t ext_size = 0;
    size_t size() const { return (dry || ext) ? ext_size : host.size(); }
    template <class T>
    size_t add(const std::vector<T> &v) {
        const size_t bytes = v.size() * sizeof(T);
        if (dry || ext) {
            const size_t off = align_up(ext_size, 256);
            ext_size = off + bytes;
            if (ext && bytes) memcpy(ext + off, v.data(), bytes);
            return off;
        }
        const size_t off = align_up(host.size(), 256);
        host.resize(off + bytes);
        if (bytes) memcpy(host.data() + off, v.data(), bytes);
        return off;
    }
};
}  // namespace

// (no C++ exception crosses the C boundary: the functions that build host structures in proportion to their input catch
// what the standard library throws -- an allocation that fails, a size beyond max_size -- and report it as a status)
template <class F>
static int no_throw(const char *what, F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(MM_ERR_NOMEM, std::string(what) + ": out of host memory");
    } catch (const std::exception &ex) {
        return fail(MM_ERR_INVALID, std::string(what) + ": " + ex.what());
    } catch (...) {
        return fail(MM_ERR_INVALID, std::string(what) + ": unknown exception");
    }
}

extern "C" {

int mm_abi_version(void) { return MM_ABI_VERSION; }
const char *mm_last_error(void) { return g_err_store.c_str(); }

// the generic path's copies of an FSM (mm_generic.hip): both matrices in double, natural units, rows sorted by column
static void gen_build(mm_fsm_s *f) {
    const int64_t S1 = f->S1, nnz = f->nnz;
    std::vector<int64_t> gptr(f->raw_ptr);
    std::vector<int32_t> gcol(std::move(f->raw_col));
    std::vector<double> gval(std::move(f->raw_val));
    std::vector<std::pair<int32_t, double>> tmp;
    for (int64_t r = 0; r < S1; ++r) {
        tmp.clear();
        for (int64_t k = gptr[r]; k < gptr[r + 1]; ++k) tmp.push_back({gcol[size_t(k)], gval[size_t(k)]});
        std::stable_sort(tmp.begin(), tmp.end(), [](auto &x, auto &y) { return x.first < y.first; });
        for (int64_t k = gptr[r]; k < gptr[r + 1]; ++k) {
            gcol[size_t(k)] = tmp[size_t(k - gptr[r])].first;
            gval[size_t(k)] = tmp[size_t(k - gptr[r])].second;
        }
    }
    std::vector<int64_t> tptr(size_t(S1) + 1, 0);
    std::vector<int32_t> tcol(static_cast<size_t>(nnz));
    std::vector<double> tval(static_cast<size_t>(nnz));
    for (int64_t k = 0; k < nnz; ++k) tptr[size_t(gcol[size_t(k)]) + 1]++;
    for (int64_t i = 0; i < S1; ++i) tptr[size_t(i) + 1] += tptr[size_t(i)];
    std::vector<int64_t> cur(tptr.begin(), tptr.end() - 1);
    for (int64_t r = 0; r < S1; ++r)
        for (int64_t k = gptr[r]; k < gptr[r + 1]; ++k) {
            const int64_t d = cur[size_t(gcol[size_t(k)])]++;
            tcol[size_t(d)] = int32_t(r);
            tval[size_t(d)] = gval[size_t(k)];
        }
    const int gi = f->gen_layout == MM_CSC ? 0 : 1;  // (the given matrix is the forward one when it came as CSC(T_hat))
    f->gen_ptr[gi] = std::move(gptr);
    f->gen_col[gi] = std::move(gcol);
    f->gen_val[gi] = std::move(gval);
    f->gen_ptr[1 - gi] = std::move(tptr);
    f->gen_col[1 - gi] = std::move(tcol);
    f->gen_val[1 - gi] = std::move(tval);
    for (int d = 0; d < 2; ++d) {
        f->gen.ptr[d] = f->gen_ptr[d].data();
        f->gen.col[d] = f->gen_col[d].data();
        f->gen.val[d] = f->gen_val[d].data();
    }
    f->raw_ptr.clear();
    f->raw_ptr.shrink_to_fit();
}
// the item forms of an FSM (mm_pack.h), packed when first needed
static void ensure_packed(mm_fsm_s *f) {
    if (f->semiring == MM_PROB) return;  // (the generic path only)
    std::call_once(f->packed_once, [&]() {
        const float NINF = -std::numeric_limits<float>::infinity();
        for (int d = 0; d < 2; ++d) f->packed[d] = pack_rows(f->S1, f->mat[d].rowptr, f->mat[d].col, f->mat[d].val, f->s2p, NINF);
    });
}

static int fsm_create_impl(int semiring, int64_t S1, int64_t nnz, int layout, int index_bytes, int index_base, int val_bytes,
                           const void *ptr, const void *idx, const void *val, int64_t n_init, const void *init_idx,
                           const void *init_val, const int32_t *state2pdf, int32_t P1, mm_fsm_t *out) {
    if (!out) return fail(MM_ERR_INVALID, "mm_fsm_create: out is NULL");
    *out = nullptr;
    if (semiring != MM_LOG && semiring != MM_TROPICAL && semiring != MM_PROB) return fail(MM_ERR_INVALID, "mm_fsm_create: unknown semiring");
    if (layout != MM_CSC && layout != MM_CSR) return fail(MM_ERR_INVALID, "mm_fsm_create: unknown layout");
    if ((index_bytes != 4 && index_bytes != 8) || (val_bytes != 4 && val_bytes != 8) ||
        (index_base != 0 && index_base != 1))
        return fail(MM_ERR_INVALID, "mm_fsm_create: index_bytes/val_bytes must be 4 or 8, index_base 0 or 1");
    if (S1 < 2 || P1 < 2 || nnz < 0 || n_init < 0) return fail(MM_ERR_DIM, "mm_fsm_create: need S1 >= 2, P1 >= 2");
    if (S1 > (int64_t(1) << 30)) return fail(MM_ERR_UNSUPPORTED, "mm_fsm_create: too many states");
    if (!ptr || !state2pdf || (nnz && (!idx || !val)) || (n_init && (!init_idx || !init_val)))
        return fail(MM_ERR_INVALID, "mm_fsm_create: NULL array");
    if (rd_index(ptr, index_bytes, 0) != index_base || rd_index(ptr, index_bytes, S1) - index_base != nnz)
        return fail(MM_ERR_DIM, "mm_fsm_create: ptr[0]/ptr[S1] do not match index_base/nnz");
    Csr given;
    given.rowptr.resize(S1 + 1);
    given.col.resize(nnz);
    given.val.resize(nnz);
    const float scale = semiring == MM_LOG ? MM_LOG2E : 1.0f;
    for (int64_t i = 0; i <= S1; ++i) {
        given.rowptr[i] = rd_index(ptr, index_bytes, i) - index_base;
        if (given.rowptr[i] < 0 || given.rowptr[i] > nnz || (i && given.rowptr[i] < given.rowptr[i - 1]))
            return fail(MM_ERR_DIM, "mm_fsm_create: ptr is not monotone within [0, nnz]");
    }
    for (int64_t k = 0; k < nnz; ++k) {
        int64_t c = rd_index(idx, index_bytes, k) - index_base;
        if (c < 0 || c >= S1) return fail(MM_ERR_DIM, "mm_fsm_create: state index out of range");
        given.col[k] = int32_t(c);
        given.val[k] = rd_val(val, val_bytes, k) * scale;
    }
    // (the caller's arrays as given, 0-based: the arc posteriors report in their entry order)
    const bool entry_order = semiring == MM_LOG || semiring == MM_TROPICAL;  // (tropical: the class planes of mm_batch_set_path_classes)
    const std::vector<int64_t> given_ptr = entry_order ? given.rowptr : std::vector<int64_t>();
    const std::vector<int32_t> given_idx = entry_order ? given.col : std::vector<int32_t>();
    sort_rows(given, S1);
    // MM_CSC(T_hat) is CSR(T_hat') = the forward matrix; MM_CSR(T_hat) the backward one
    Csr other = transpose(given, S1);
    const Csr &fwd = layout == MM_CSC ? given : other;
    const Csr &bwd = layout == MM_CSC ? other : given;

    mm_fsm_s *f = new mm_fsm_s();
    f->semiring = semiring;
    f->S1 = S1;
    f->nnz = nnz;
    f->P1 = P1;
    f->S1p = padded_states(S1);  // at least one slot beyond the last state (the row kernels' "no row" position)
    f->s2p.resize(S1);
    for (int64_t s = 0; s < S1; ++s) {
        int32_t pdf = state2pdf[s] - index_base;
        if (pdf < 0 || pdf >= P1) {
            delete f;
            return fail(MM_ERR_DIM, "mm_fsm_create: state2pdf out of range");
        }
        f->s2p[s] = pdf;
    }
    if (f->s2p[S1 - 1] != P1 - 1) {
        delete f;
        return fail(MM_ERR_DIM, "mm_fsm_create: the final state must map to the last (phony) pdf");
    }
    const float NINF = -std::numeric_limits<float>::infinity();
    f->init.assign(S1, NINF);
    for (int64_t k = 0; k < n_init; ++k) {
        int64_t s = rd_index(init_idx, index_bytes, k) - index_base;
        if (s < 0 || s >= S1) {
            delete f;
            return fail(MM_ERR_DIM, "mm_fsm_create: initial state out of range");
        }
        f->init[s] = rd_val(init_val, val_bytes, k) * scale;
    }
    {   // the generic path's copy (double, natural units) is built when mm_pdfposteriors_ex first asks for it: gen_build()
        f->gen_layout = layout;
        f->raw_ptr = given.rowptr;
        f->raw_col.resize(static_cast<size_t>(nnz));
        f->raw_val.resize(static_cast<size_t>(nnz));
        for (int64_t k = 0; k < nnz; ++k) {
            f->raw_col[size_t(k)] = int32_t(rd_index(idx, index_bytes, k) - index_base);
            f->raw_val[size_t(k)] = val_bytes == 4 ? double(static_cast<const float *>(val)[k]) : static_cast<const double *>(val)[k];
        }
        const double zero = semiring == MM_PROB ? 0.0 : -std::numeric_limits<double>::infinity();
        f->gen_init.assign(size_t(S1), zero);
        for (int64_t k = 0; k < n_init; ++k) {
            const int64_t s = rd_index(init_idx, index_bytes, k) - index_base;
            f->gen_init[size_t(s)] = val_bytes == 4 ? double(static_cast<const float *>(init_val)[k]) : static_cast<const double *>(init_val)[k];
        }
        f->gen.semiring = semiring;
        f->gen.S1 = S1;
        f->gen.P1 = P1;
        f->gen.init = f->gen_init.data();
        f->gen.s2p = f->s2p.data();
    }
    if (semiring == MM_PROB) {
        // the generic path (mm_pdfposteriors_ex) works on the FSM as given; Float32 FSMs with non-negative weights also get their
        // log-semiring twin for the fast kernels (mm_pdfposteriors_f32)
        bool twin = val_bytes == 4;
        std::vector<float> lv(static_cast<size_t>(nnz)), liv(static_cast<size_t>(n_init));
        for (int64_t k = 0; k < nnz && twin; ++k) {
            const float x = static_cast<const float *>(val)[k];
            twin = x >= 0.f;
            lv[size_t(k)] = std::log(x);  // (log 0 = -inf = zero(LogSemiring))
        }
        for (int64_t k = 0; k < n_init && twin; ++k) {
            const float x = static_cast<const float *>(init_val)[k];
            twin = x >= 0.f;
            liv[size_t(k)] = std::log(x);
        }
        if (twin) {
            mm_fsm_t tw = nullptr;
            // (a graph the log forms refuse stays what it was before round 6: a ProbSemiring FSM of the generic entry, without a twin)
            if (fsm_create_impl(MM_LOG, S1, nnz, layout, index_bytes, index_base, 4, ptr, idx, lv.data(), n_init, init_idx, liv.data(), state2pdf, P1, &tw) == MM_OK)
                f->log_twin = tw;
        }
        *out = f;
        return MM_OK;
    }
    f->mat[0] = fwd;
    f->mat[1] = bwd;
    {
        // the caller's entry behind every entry of bwd (sort_rows and transpose are stable: a row of bwd lists its arcs by
        // destination, the arcs of one (source, destination) in the caller's order) -- tropical FSMs too: the class planes of
        // mm_batch_set_path_classes go by the caller's entries
        f->bwd_caller.resize(size_t(nnz));
        if (layout == MM_CSR) {
            std::vector<int64_t> ks;
            for (int64_t r = 0; r < S1; ++r) {
                ks.clear();
                for (int64_t k = given_ptr[size_t(r)]; k < given_ptr[size_t(r) + 1]; ++k) ks.push_back(k);
                std::stable_sort(ks.begin(), ks.end(), [&](int64_t x, int64_t y) { return given_idx[size_t(x)] < given_idx[size_t(y)]; });
                std::copy(ks.begin(), ks.end(), f->bwd_caller.begin() + given_ptr[size_t(r)]);
            }
        } else {  // CSC(T_hat): the caller's entries come by destination; bucket them by source
            std::vector<int64_t> cur(bwd.rowptr.begin(), bwd.rowptr.end() - 1);
            for (int64_t k = 0; k < nnz; ++k) f->bwd_caller[size_t(cur[size_t(given_idx[size_t(k)])]++)] = k;
        }
        for (int64_t k = given_ptr[size_t(S1 - 1)]; k < given_ptr[size_t(S1)] && f->kphony < 0; ++k)
            if (given_idx[size_t(k)] == S1 - 1) f->kphony = k;
        f->init_order.resize(size_t(n_init));
        for (int64_t k = 0; k < n_init; ++k) f->init_order[size_t(k)] = int32_t(rd_index(init_idx, index_bytes, k) - index_base);
    }
    if (semiring == MM_LOG) {
        // useful states: forward reachable (over out-arcs = rows of T_hat) and co-reachable (over in-arcs)
        std::vector<char> reach(S1, 0), coreach(S1, 0);
        std::vector<int32_t> stack;
        for (int64_t s = 0; s < S1; ++s)
            if (f->init[s] > NINF) {
                reach[s] = 1;
                stack.push_back(int32_t(s));
            }
        while (!stack.empty()) {
            const int32_t i = stack.back();
            stack.pop_back();
            for (int64_t k = bwd.rowptr[i]; k < bwd.rowptr[i + 1]; ++k)
                if (bwd.val[k] > NINF && !reach[bwd.col[k]]) {
                    reach[bwd.col[k]] = 1;
                    stack.push_back(bwd.col[k]);
                }
        }
        coreach[S1 - 1] = 1;
        stack.push_back(int32_t(S1 - 1));
        while (!stack.empty()) {
            const int32_t j = stack.back();
            stack.pop_back();
            for (int64_t k = fwd.rowptr[j]; k < fwd.rowptr[j + 1]; ++k)
                if (fwd.val[k] > NINF && !coreach[fwd.col[k]]) {
                    coreach[fwd.col[k]] = 1;
                    stack.push_back(fwd.col[k]);
                }
        }
        // Which states the kernel forms keep.  A state that cannot reach the final state has beta = zero(K), one that cannot be
        // reached alpha = zero(K): neither contributes to any posterior, and until round 6 both were dropped.  Now a FEW unreachable
        // states that do reach the final state stay (config 3's generator leaves 4 of 2000 units without a predecessor): their rows
        // cost nothing to speak of, their alpha is exactly 0 on every path of the kernels, and the backward forms then hold every
        // state with a non-zero beta -- the beta-recursion export (mm_betarecursion_f32) can run on them.  The alpha-recursion export
        // needs every reachable state to reach the final state (export_on_pairs).
        int64_t n_extra = 0;
        f->export_ok[0] = true;
        for (int64_t s = 0; s < S1; ++s) {
            if (reach[s] && !coreach[s]) f->export_ok[0] = false;
            n_extra += coreach[s] && !reach[s];
        }
        const bool keep_extra = n_extra * 64 <= S1;
        f->export_ok[1] = keep_extra || n_extra == 0;
        std::vector<char> useful(S1, 0);
        for (int64_t s = 0; s < S1; ++s) useful[s] = coreach[s] && (reach[s] || keep_extra);
        for (int d = 0; d < 2; ++d) {
            const Csr &m = d == 0 ? fwd : bwd;
            Csr &q = f->qmat[d];
            q.rowptr.assign(S1 + 1, 0);
            for (int64_t r = 0; r < S1; ++r) {
                if (useful[r])
                    for (int64_t k = m.rowptr[r]; k < m.rowptr[r + 1]; ++k)
                        if (m.val[k] > NINF && useful[m.col[k]]) {
                            q.col.push_back(m.col[k]);
                            q.val.push_back(m.val[k]);
                        }
                q.rowptr[r + 1] = int64_t(q.col.size());
            }
            f->nquads[d] = count_quads(S1, q.rowptr);
        }
        f->fast_ok = quad_range_ok(S1, f->qmat[0].rowptr, f->qmat[0].val, P1) &&
                     quad_range_ok(S1, f->qmat[1].rowptr, f->qmat[1].val, P1);
        // depth = the most arcs any state is away from the initial states.  A deep (left-to-right) graph keeps
        // states alive whose values differ by more than the float range within one frame, so most rows of the
        // quad kernels' linear-domain sums would take the exact fallback: such graphs run on the item kernel.
        std::vector<int32_t> seeds;
        for (int64_t s = 0; s < S1; ++s)
            if (f->init[s] > NINF) seeds.push_back(int32_t(s));
        for (uint16_t d : reach_distance(S1, f->qmat[1].rowptr, f->qmat[1].col, seeds))
            if (d != 0xffff) f->depth = std::max(f->depth, int(d));
    }
    *out = f;
    return MM_OK;
}

// one device allocation (DevMem: freed with its owner) holding a blob
static int upload(const Blob &bl, DevMem &out) {
    void *blob = nullptr;
    HIP_TRY(hipMalloc(&blob, bl.host.size() ? bl.host.size() : 256));
    DevMem own(blob);
    hipError_t e = hipMemcpy(blob, bl.host.data(), bl.host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(MM_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    out = std::move(own);
    return MM_OK;
}

static int fsm_to_device(mm_fsm_t f) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (f->dev_blob && f->device == dev) return MM_OK;
    if (f->dev_blob) return fail(MM_ERR_INVALID, "FSM already resident on another device");
    ensure_packed(f);
    Blob bl;
    size_t o_items[2], o_rows[2], o_slots[2];
    for (int d = 0; d < 2; ++d) {
        o_items[d] = bl.add(f->packed[d].items);
        o_rows[d] = bl.add(f->packed[d].rowinfo);
        o_slots[d] = bl.add(f->packed[d].slots);
    }
    const size_t o_init = bl.add(f->init), o_s2p = bl.add(f->s2p);
    // pdf -> states (CSR): in deterministic mode the item kernel sums a pdf's state posteriors over this list, in this order
    std::vector<int32_t> pdf_ptr(size_t(f->P1) + 1, 0), pdf_rows(size_t(f->S1), 0);
    for (int64_t s = 0; s < f->S1; ++s) ++pdf_ptr[size_t(f->s2p[s]) + 1];
    for (int32_t q = 0; q < f->P1; ++q) pdf_ptr[q + 1] += pdf_ptr[q];
    {
        std::vector<int32_t> fill(pdf_ptr.begin(), pdf_ptr.end() - 1);
        for (int64_t s = 0; s < f->S1; ++s) pdf_rows[size_t(fill[f->s2p[s]]++)] = int32_t(s);
    }
    const size_t o_pptr = bl.add(pdf_ptr), o_prows = bl.add(pdf_rows);
    int rc = upload(bl, f->dev_blob);
    if (rc) return rc;
    char *base = static_cast<char *>(f->dev_blob.get());
    for (int d = 0; d < 2; ++d) {
        f->gdev[d].items = reinterpret_cast<const ItemMeta *>(base + o_items[d]);
        f->gdev[d].rowinfo = reinterpret_cast<const RowInfo *>(base + o_rows[d]);
        f->gdev[d].slots = reinterpret_cast<const Slot *>(base + o_slots[d]);
        f->gdev[d].n_items = int(f->packed[d].items.size());
        f->gdev[d].n_short = 0;
        for (const auto &im : f->packed[d].items) f->gdev[d].n_short += im.R <= 4 ? 1 : 0;
    }
    f->d_init = reinterpret_cast<const float *>(base + o_init);
    f->d_s2p = reinterpret_cast<const int *>(base + o_s2p);
    f->d_pdf_ptr = reinterpret_cast<const int *>(base + o_pptr);
    f->d_pdf_rows = reinterpret_cast<const int *>(base + o_prows);
    f->dev_bytes = bl.host.size();
    f->device = dev;
    return MM_OK;
}

// alpha_hat in the order of a form (position -> original state)
static std::vector<float> init_by(mm_fsm_t f, const std::vector<int32_t> &order) {
    std::vector<float> v(size_t(f->S1));
    for (int64_t i = 0; i < f->S1; ++i) v[size_t(i)] = f->init[size_t(order[size_t(i)])];
    return v;
}

// build (once per direction and KQ) and upload the quad form of an FSM
static int quad_variant(mm_fsm_t f, int dir, int KQ, bool verbose, QuadVariant **out) {
    auto it = f->variants.find(2 * KQ + dir);
    if (it != f->variants.end()) {
        *out = it->second.get();
        return MM_OK;
    }
    auto v = std::make_unique<QuadVariant>();
    v->KQ = KQ;
    v->dir = dir;
    v->g = make_quads(f->S1, f->qmat[dir].rowptr, f->qmat[dir].col, f->qmat[dir].val, f->s2p, f->P1, dir == 1, KQ);
    if (verbose)
        fprintf(stderr, "[mm] quad form dir %d: KQ %d, %zu quads, %lld arcs, LDS cycles/gather (bank model) %.2f -> %.2f\n",
                dir, KQ, v->g.quads.size(), (long long)f->qmat[dir].rowptr[f->S1], v->g.conflict_before,
                v->g.conflict_after);
    if (dir == 0) {
        v->init_f = init_by(f, v->g.order);
    } else {
        // the forward numbering does not depend on KQ (rows by decreasing quads): take it from any forward form
        std::vector<int32_t> order_f, pos_f;
        quad_order(f->S1, f->qmat[0].rowptr, f->s2p, f->P1, false, order_f, pos_f);
        v->map_bf.resize(f->S1);
        for (int64_t i = 0; i < f->S1; ++i) v->map_bf[i] = uint16_t(pos_f[v->g.order[i]]);
    }
    {   // distances in original numbering: forward = arcs from an initial state (successor lists = rows of
        // T_hat, qmat[1]); backward = arcs to the phony final state (predecessor lists = rows of T_hat', qmat[0])
        std::vector<int32_t> seeds;
        if (dir == 0) {
            for (int64_t s = 0; s < f->S1; ++s)
                if (f->init[s] > -std::numeric_limits<float>::infinity()) seeds.push_back(int32_t(s));
        } else {
            seeds.push_back(int32_t(f->S1 - 1));
        }
        const std::vector<uint16_t> d0 = reach_distance(f->S1, f->qmat[1 - dir].rowptr, f->qmat[1 - dir].col, seeds);
        v->dist.resize(f->S1);
        for (int64_t i = 0; i < f->S1; ++i) v->dist[i] = d0[v->g.order[i]];
    }
    Blob bl;
    const size_t o_q = bl.add(v->g.quads), o_rec = bl.add(v->g.recs), o_ptr = bl.add(v->g.rowptr);
    const size_t o_col = bl.add(v->g.col), o_w = bl.add(v->g.w), o_pse = bl.add(v->g.pdfstart);
    const size_t o_dist = bl.add(v->dist), o_initf = bl.add(v->init_f), o_map = bl.add(v->map_bf);
    int rc = upload(bl, v->blob);
    if (rc) return rc;
    char *base = static_cast<char *>(v->blob.get());
    v->qdev.quads = reinterpret_cast<const Quad *>(base + o_q);
    v->qdev.recs = reinterpret_cast<const RowRec *>(base + o_rec);
    v->qdev.rowptr = reinterpret_cast<const int *>(base + o_ptr);
    v->qdev.col = reinterpret_cast<const int *>(base + o_col);
    v->qdev.w = reinterpret_cast<const float *>(base + o_w);
    v->qdev.pdfse = reinterpret_cast<const unsigned short *>(base + o_pse);
    v->qdev.dist = reinterpret_cast<const unsigned short *>(base + o_dist);
    v->qdev.nq = int(v->g.quads.size());
    v->qdev.fpos = v->g.pos[f->S1 - 1];
    v->qdev.ncopy = v->g.ncopy;
    v->qdev.pad = 0;
    v->d_init_f = reinterpret_cast<const float *>(base + o_initf);
    v->d_map_bf = reinterpret_cast<const unsigned short *>(base + o_map);
    *out = v.get();
    f->variants[2 * KQ + dir] = std::move(v);
    return MM_OK;
}

// the device image of a row-lane form: sections of one blob (offsets in RowBlob) ...
struct RowBlob {
    Blob bl;
    size_t o_w, o_a, o_s, o_sc, o_ptr, o_col, o_cw, o_pdf, o_pse, o_init, o_ord, o_pt, o_tab;
};
static void row_variant_blob(RowVariant &v, bool pad, RowBlob &rb) {
    // (zero rows up to MM_ROW_KA_PAD arc slots: the kernels load their whole register window unconditionally)
    if (pad) {
        v.g.w.resize(size_t(MM_ROW_KA_PAD) * 64 * v.g.NWC, 0.f);
        v.g.addr.resize(size_t(MM_ROW_KA_PAD) * 64 * v.g.NWC, 0u);
    }
    Blob &bl = rb.bl;
    rb.o_w = bl.add(v.g.w), rb.o_a = bl.add(v.g.addr), rb.o_s = bl.add(v.g.slots), rb.o_sc = bl.add(v.g.sched);
    rb.o_ptr = bl.add(v.g.rowptr), rb.o_col = bl.add(v.g.col), rb.o_cw = bl.add(v.g.cw);
    rb.o_pdf = bl.add(v.g.rowpdf), rb.o_pse = bl.add(v.g.pdfse), rb.o_init = bl.add(v.init), rb.o_ord = bl.add(v.g.order);
    rb.o_pt = bl.add(v.ptab);
    rb.o_tab = bl.add(v.g.pdftab);
}
// ... and the form's device descriptor once the blob sits at `base`
static void row_variant_bind(mm_fsm_t f, RowVariant &v, const RowBlob &rb, char *base, float thr) {
    RowDev &d = v.rdev;
    d.w = reinterpret_cast<const float *>(base + rb.o_w);
    d.addr = reinterpret_cast<const unsigned *>(base + rb.o_a);
    d.slots = reinterpret_cast<const unsigned *>(base + rb.o_s);
    d.sched = reinterpret_cast<const RowSched *>(base + rb.o_sc);
    d.rowptr = reinterpret_cast<const int *>(base + rb.o_ptr);
    d.col = reinterpret_cast<const int *>(base + rb.o_col);
    d.cw = reinterpret_cast<const float *>(base + rb.o_cw);
    d.rowpdf = reinterpret_cast<const unsigned short *>(base + rb.o_pdf);
    d.pdfse = reinterpret_cast<const unsigned short *>(base + rb.o_pse);
    d.init = reinterpret_cast<const float *>(base + rb.o_init);
    d.order = reinterpret_cast<const int *>(base + rb.o_ord);
    d.ptab = v.ptab.empty() ? nullptr : reinterpret_cast<const unsigned *>(base + rb.o_pt);
    d.pdftab = v.g.pdftab.empty() ? nullptr : reinterpret_cast<const unsigned *>(base + rb.o_tab);
    d.KA = v.g.KA;
    d.NWC = v.g.NWC;
    d.nslotrows = v.g.nslotrows;
    d.fpos = v.g.pos[f->S1 - 1];
    d.rows = int(f->S1);
    d.thr = thr;
}
// a row-lane form to a device allocation of its own
static int upload_row_variant(mm_fsm_t f, RowVariant &v, float thr, bool pad = true) {
    RowBlob rb;
    row_variant_blob(v, pad, rb);
    DevMem mem;
    int rc = upload(rb.bl, mem);
    if (rc) return rc;
    v.mem = std::move(mem);
    row_variant_bind(f, v, rb, static_cast<char *>(v.mem.get()), thr);
    return MM_OK;
}

// ---- pack options: one function per form, for the builders below and for the host-only mm_debug_*_product entries

// the row forms.  windows = false (mm_debug_row_product_ex alone): KA is not rounded up to one of the kernels' register windows
static RowPackOpts row_pack_opts(bool windows) {
    const size_t n = sizeof(kRowKA) / sizeof(kRowKA[0]);
    RowPackOpts opt;
    opt.rs = MM_ROW_RS;
    opt.ka_max = kRowKA[n - 1];
    for (size_t i = 0; i < n && windows; ++i) opt.ka_choices[i] = kRowKA[i];
    return opt;
}

// the pair forms of direction dir (same schedule rules as the row forms; 8-byte positions, one copy of the vector, the other
// direction's numbering in the slot table).  lag = false (mm_debug_row_product_ex alone): the backward agent's group_speed stays 1
static RowPackOpts pair_pack_opts(const DebugOpts &dbg, int dir, bool lag) {
    RowPackOpts opt;
    opt.rs = MM_ROW_RS;
    opt.ka_max = MM_PAIR_KA;
    opt.pair = true;
    opt.pdf_halves = !dbg.no_pdf_halves;
    for (float &x : opt.group_speed) x = 1.f;  // (the waves of a SIMD progress together: mm_rows.h)
    // (cost of a finish in arcs: measured with cycle stamps on config 3 -- the backward agent's finishes are the dearer
    // ones, its phase B is the longest kernel of a call: 8 / 24 against 8 / 8 shortens it by 4 %)
    if (dbg.finish_cost > 0) opt.finish_cost = dbg.finish_cost;
    else if (dir == 1) opt.finish_cost = 24;
    if (dbg.group_speed[0] > 0) {
        for (int i = 0; i < 4; ++i) opt.group_speed[i] = dbg.group_speed[i];
    } else if (dir == 1 && lag) {  // (the backward agent's younger waves still lag a little: stamps, -1..2 % with these weights)
        const float sp[4] = {1.08f, 1.04f, 0.97f, 0.92f};
        for (int i = 0; i < 4; ++i) opt.group_speed[i] = sp[i];
    }
    opt.ka_choices[0] = MM_PAIR_KA;
    opt.bank_opt = dbg.bankopt ? 1 : 0;
    return opt;
}

// options of the split pair forms (mm_rows.h make_rows_split; the kernels: mm_kernel_pairs.hip with H > 1)
static void split_pack_opts(const DebugOpts &dbg, RowPackOpts &opt, RowPackOpts &optb, int H = 2) {
    opt = RowPackOpts();
    opt.rs = mm_split_rs(H);
    opt.ka_max = mm_split_ka(H);
    opt.nwc_max = MM_SPLIT_NWC;
    opt.pair = true;
    opt.pdf_halves = !dbg.no_pdf_halves;
    for (float &x : opt.group_speed) x = 1.f;
    if (dbg.finish_cost > 0) opt.finish_cost = dbg.finish_cost;
    opt.ka_choices[0] = mm_split_ka(H);
    // (the old cap list: with every even cap up to the window the teams of 4 measured 1 % slower on 4000 states and the teams of 2
    // 1 % faster on the WSJ denominator, inside three times its spread -- the step of a team waits for its mates' rows)
    opt.every_cap = false;
    optb = opt;
    if (dbg.finish_cost <= 0) optb.finish_cost = 24;
}

// the wave forms.  lean = false (mm_debug_wave_product alone): place, naive_stats and q_positions stay at the packer's defaults
static RowPackOpts wave_pack_opts(bool lean) {
    RowPackOpts opt;
    opt.rs = MM_WAVE_RS;
    opt.nwc_max = MM_WAVE_WAVES;
    opt.ka_max = 16;  // (4 segments of 4 slots per wave)
    opt.copies = 1;
    opt.acap_force = 4;
    opt.seg_stride = 4;
    opt.log_weights = true;
    opt.want_partner = true;
    opt.spread_pdf = true;
    opt.finish_cost = 4;
    for (float &x : opt.group_speed) x = 1.f;
    if (!lean) return opt;
    // (greedy placement without the local search: the wave kernel is bound by its waves' latency chains, not by LDS cycles --
    // 0.434 -> 0.437 ms on the WSJ numerators x 128 -- and the search is half the host time of packing a small graph)
    opt.place = 1;
    opt.naive_stats = false;
    opt.q_positions = false;  // (the wave kernel sums the posteriors per pdf through its own tables: wave_pdf_table)
    if (process_debug_opts().wave_place >= 0) opt.place = process_debug_opts().wave_place;
    return opt;
}

// the Viterbi form, but for its layout (mix_n4, mix_n2, ka_max: vit_variant tries the kernel's instances)
static RowPackOpts vit_pack_opts() {
    RowPackOpts opt;
    opt.rs = 65536;
    opt.nwc_max = 15;
    opt.copies = 1;
    opt.acap_force = 4;
    opt.log_weights = true;
    opt.keep_order = true;
    opt.finish_cost = 4;
    for (float &x : opt.group_speed) x = 1.f;
    return opt;
}

// ---- the builders: each form once per FSM (Once), owned by the builder until it is complete and on the device

// Both directions of a row-lane family from the pruned matrices: the forward form, the backward form in the forward numbering,
// the forward form's partner words (where the kernels read them), alpha_hat in the forward form's order.  Empty: does not fit.
static RowForms pack_both(mm_fsm_t f, const RowPackOpts &opt, const RowPackOpts &optb, bool partner) {
    RowForms rv = std::make_unique<RowVariant[]>(2);
    const Csr *m = f->qmat;
    const std::vector<int32_t> none;
    if (!make_rows(f->S1, m[0].rowptr, m[0].col, m[0].val, f->s2p, f->P1, false, none, opt, rv[0].g) ||
        !make_rows(f->S1, m[1].rowptr, m[1].col, m[1].val, f->s2p, f->P1, true, rv[0].g.pos, optb, rv[1].g))
        return nullptr;
    if (partner) set_partner(rv[0].g, rv[1].g.pos);
    rv[0].init = init_by(f, rv[0].g.order);
    return rv;
}
// (arc weights below 2^-60 leave too little of the float range to the values of the linear-domain kernels: such graphs run on the
// other kernels)
static float wmin_log2(const RowForms &rv) { return std::min(rv[0].g.wmin_log2, rv[1].g.wmin_log2); }

static void say_rows(const char *name, int dir, const RowGraph &g) {
    fprintf(stderr, "[mm] %s form dir %d: KA %d, %d compute waves, %d segments, arcs/slots %.3f, cost %d..%d, "
                    "LDS cycles/gather (bank model) %.2f -> %.2f\n",
            name, dir, g.KA, g.NWC, g.nslotrows - 2, g.pad_eff, g.mincost, g.maxcost, g.conflict_before, g.conflict_after);
}

// build (once) and upload the row-lane forms of both directions of an FSM; *ok = false if it does not fit them
static int row_variants(mm_fsm_t f, bool verbose, bool *ok) {
    if (!f->rows.first(ok)) return MM_OK;
    if (f->semiring != MM_LOG || !f->fast_ok || f->P1 > 250 || (f->S1 + 1) * 4 > MM_ROW_RS) return MM_OK;
    RowForms rv = pack_both(f, row_pack_opts(true), row_pack_opts(true), false);
    if (!rv || !(wmin_log2(rv) >= -60.f)) return MM_OK;
    for (int dir = 0; dir < 2; ++dir) {
        const RowGraph &g = rv[dir].g;
        if (verbose) say_rows("row", dir, g);
        for (int w = 0; w < g.NWC && verbose; ++w) {
            const RowSched &sc = g.sched[w];
            int last = 0;
            for (int k = 0; k < 64; ++k)
                if ((sc.endmask >> k) & 1) last = k;
            fprintf(stderr, "[mm]   wave %2d: %u segments, %d arcs, lg %llx\n", w, sc.nslots & 0xffffu,
                    2 * (last + 1 - int(sc.nslots >> 16)), (unsigned long long)sc.lg);
        }
        int rc = upload_row_variant(f, rv[dir], 125.f + wmin_log2(rv));
        if (rc) return rc;
    }
    f->rows.form = std::move(rv);
    *ok = true;
    return MM_OK;
}

// the pair variants of the row-lane forms (built once; *ok = false if the FSM does not fit them)
static int pair_variants(mm_fsm_t f, const DebugOpts &dbg, bool *ok) {
    const bool verbose = dbg.verbose;
    if (!f->prows.first(ok)) return MM_OK;
    // (the row forms' conditions, with the pair kernels' own pdf capacity: 251 .. 506 pdfs run their NJ = 8 instances, which the row
    // kernels do not have)
    if (f->semiring != MM_LOG || !f->fast_ok || f->P1 > MM_PAIR_P1MAX || (f->S1 + 1) * 4 > MM_ROW_RS) {
        if (verbose) fprintf(stderr, "[mm] pair form: not tried (semiring %d, fast_ok %d, P1 %d, S1 %lld)\n", f->semiring, int(f->fast_ok), int(f->P1), (long long)f->S1);
        return MM_OK;
    }
    RowForms rv = pack_both(f, pair_pack_opts(dbg, 0, true), pair_pack_opts(dbg, 1, true), true);
    if (verbose && !rv) fprintf(stderr, "[mm] pair form: the graph does not fit the register windows (KA %d)\n", MM_PAIR_KA);
    if (rv && wmin_log2(rv) < -60.f) {
        if (verbose) fprintf(stderr, "[mm] pair form: arc weights down to 2^%.0f\n", wmin_log2(rv));
        rv.reset();
    }
    if (!rv) return MM_OK;
    for (int dir = 0; dir < 2; ++dir) {
        if (verbose) say_rows("pair", dir, rv[dir].g);
        int rc = upload_row_variant(f, rv[dir], 125.f + wmin_log2(rv));
        if (rc) return rc;
    }
    f->prows.form = std::move(rv);
    *ok = true;
    return MM_OK;
}

// the Viterbi form of a tropical FSM (built once; *ok = false if it does not fit: a row of more than 255 arcs, more than 8
// segments per wave -- 5760 rows at most)
static int vit_variant(mm_fsm_t f, const DebugOpts &dbg, bool *ok) {
    if (!f->vrow.first(ok)) return MM_OK;
    if (f->semiring != MM_TROPICAL || f->P1 > 256) return MM_OK;
    RowPackOpts opt = vit_pack_opts();
    RowForms rv = std::make_unique<RowVariant[]>(1);
    RowVariant &v = rv[0];
    const std::vector<int32_t> none;
    // per wave N4 positions of 4 arc slots and N2 of 2: the cheapest layout the graph fits (the kernel's instances)
    static const int shapes[3][2] = {{1, 5}, {2, 4}, {6, 0}};
    bool fits = false;
    for (const auto &sh : shapes) {
        opt.mix_n4 = sh[0];
        opt.mix_n2 = sh[1];
        opt.ka_max = 4 * sh[0] + 2 * sh[1];
        if (make_rows(f->S1, f->mat[0].rowptr, f->mat[0].col, f->mat[0].val, f->s2p, f->P1, false, none, opt, v.g)) {
            fits = true;
            f->vit_n4 = sh[0];
            f->vit_n2 = sh[1];
            break;
        }
    }
    if (!fits) return MM_OK;
    v.init = init_by(f, v.g.order);
    if (dbg.verbose)
        fprintf(stderr, "[mm] Viterbi form: %d waves, %d segments, %d x 4 + %d x 2 arc slots per lane, arcs/slots %.3f\n", v.g.NWC,
                v.g.nslotrows - 2, f->vit_n4, f->vit_n2, v.g.pad_eff);
    int rc = upload_row_variant(f, v, 0.f, false);
    if (rc) return rc;
    f->vrow.form = std::move(rv);
    *ok = true;
    return MM_OK;
}

// the lane form of an FSM (mm_kernel_lane.hip): up to 64 real states, every one on a real pdf, up to 64 pdfs; built once
static int lane_variant(mm_fsm_t f, bool *ok) {
    if (!f->lane.first(ok)) return MM_OK;
    const int64_t S = f->S1 - 1;
    const int P = f->P1 - 1;
    if (f->semiring != MM_LOG || S < 1 || S > 64 || P < 1 || P > 64) return MM_OK;
    for (int64_t s = 0; s < S; ++s)
        if (f->s2p[size_t(s)] >= P) return MM_OK;  // (a real state on the phony pdf)
    std::vector<double> w0(64 * 64, 0.0), w1(64 * 64, 0.0);
    std::vector<float> init(64, -std::numeric_limits<float>::infinity()), fin(64, -std::numeric_limits<float>::infinity());
    std::vector<int32_t> s2p(64, 0), pdf_ptr(size_t(P) + 1, 0), pdf_states(64, 0);
    const Csr &fwd = f->mat[0], &bwd = f->mat[1];
    for (int64_t j = 0; j < S; ++j)  // forward: row j of T_hat' = the arcs INTO j
        for (int64_t k = fwd.rowptr[size_t(j)]; k < fwd.rowptr[size_t(j) + 1]; ++k)
            if (fwd.col[size_t(k)] < S) w0[size_t(fwd.col[size_t(k)]) * 64 + size_t(j)] += std::exp2(double(fwd.val[size_t(k)]));
    for (int64_t i = 0; i < S; ++i)  // backward: row i of T_hat = the arcs OUT OF i
        for (int64_t k = bwd.rowptr[size_t(i)]; k < bwd.rowptr[size_t(i) + 1]; ++k) {
            const int64_t d = bwd.col[size_t(k)];
            if (d < S) w1[size_t(d) * 64 + size_t(i)] += std::exp2(double(bwd.val[size_t(k)]));
            else if (bwd.val[size_t(k)] > -std::numeric_limits<float>::infinity())  // the arc to the final state: omega_i
                fin[size_t(i)] = fin[size_t(i)] > -std::numeric_limits<float>::infinity()
                                     ? float(std::log2(std::exp2(double(fin[size_t(i)])) + std::exp2(double(bwd.val[size_t(k)]))))
                                     : bwd.val[size_t(k)];
        }
    bool ident = true;
    for (int64_t s = 0; s < S; ++s) {
        init[size_t(s)] = f->init[size_t(s)];
        s2p[size_t(s)] = f->s2p[size_t(s)];
        ident = ident && f->s2p[size_t(s)] == int32_t(s);
        ++pdf_ptr[size_t(f->s2p[size_t(s)]) + 1];
    }
    for (int q = 0; q < P; ++q) pdf_ptr[size_t(q) + 1] += pdf_ptr[size_t(q)];
    {
        std::vector<int32_t> fill(pdf_ptr.begin(), pdf_ptr.end() - 1);
        for (int64_t s = 0; s < S; ++s) pdf_states[size_t(fill[size_t(f->s2p[size_t(s)])]++)] = int32_t(s);
    }
    Blob bl;
    std::vector<char> head(align_up(mm_lane_dev_bytes(), 256), 0);
    const size_t o_head = bl.add(head), o_w0 = bl.add(w0), o_w1 = bl.add(w1), o_init = bl.add(init), o_fin = bl.add(fin), o_s2p = bl.add(s2p),
                 o_pp = bl.add(pdf_ptr), o_ps = bl.add(pdf_states);
    void *raw = nullptr;
    HIP_TRY(hipMalloc(&raw, bl.host.size()));
    DevMem blob(raw);
    char *base = static_cast<char *>(raw);
    mm_lane_dev_fill(bl.host.data() + o_head, reinterpret_cast<const double *>(base + o_w0), reinterpret_cast<const double *>(base + o_w1),
                     reinterpret_cast<const float *>(base + o_init), reinterpret_cast<const float *>(base + o_fin),
                     reinterpret_cast<const int *>(base + o_s2p), reinterpret_cast<const int *>(base + o_pp),
                     reinterpret_cast<const int *>(base + o_ps), int(S), P, ident ? 1 : 0);
    if (hipMemcpy(raw, bl.host.data(), bl.host.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(MM_ERR_HIP, "lane form: upload failed");
    f->lane.form = std::move(blob);
    *ok = true;
    return MM_OK;
}

// the stream form of an FSM for teams of H workgroups (mm_stream.hip): built once per H; *ok = false if the graph does not fit it
static int stream_hidx(int H) { return H == 4 ? 2 : (H == 2 ? 1 : 0); }
static int stream_variant(mm_fsm_t f, int H, bool *ok) {
    auto &o = f->stream_h[stream_hidx(H)];
    if (!o.first(ok)) return MM_OK;
    if (f->semiring != MM_LOG) return MM_OK;
    const int64_t *rp[2] = {f->mat[0].rowptr.data(), f->mat[1].rowptr.data()};
    const int32_t *cl[2] = {f->mat[0].col.data(), f->mat[1].col.data()};
    const float *vl[2] = {f->mat[0].val.data(), f->mat[1].val.data()};
    int dev = -1;
    const bool have_dev = hipGetDevice(&dev) == hipSuccess;
    StreamForm *sf = nullptr;
    int rc = mm_stream_build(f->S1, f->P1, rp, cl, vl, f->init.data(), f->s2p.data(), have_dev, H, &sf);
    o.form.reset(sf);
    if (rc) return rc;
    *ok = sf != nullptr;
    return MM_OK;
}

// The per-pdf sums of the wave kernel (C_hat' * (A .* B), src/inference.jl:155) as packed segments of their own: pdf p
// with n_p states gets a group of L_p = pow2(ceil(n_p / 4)) adjacent lanes, each of which reads 4 of the states' values
// (byte addresses relative to the vector u in the numbering of `g`: 4 * position; unused slots read the trash position,
// which holds zero(K)); the lanes of a group combine by a butterfly.  Groups are placed largest first, so every group
// starts at a multiple of its size; a segment is 64 lanes.  Segment s runs on compute wave 3 - s % 4 as its pdf segment
// s / 4.  tab[((w * 2 + j) * 5 + k) * 64 + lane]: k < 4 the addresses, k = 4: 4 * pdf of the group's first lane (the lane
// that stores; others: the trash slot 4 * P1p) | log2(L) << 16.  Returns the segments per wave (1 or 2), 0 if it does not fit.
static int wave_pdf_table(const RowGraph &g, const std::vector<int32_t> &s2p, int64_t S1, int32_t P1, std::vector<uint32_t> &tab) {
    std::vector<std::vector<uint32_t>> src(static_cast<size_t>(P1));
    std::vector<std::pair<int32_t, int32_t>> bypos;  // (position, pdf): a fixed order of the states of a pdf
    for (int64_t r = 0; r < S1; ++r) bypos.emplace_back(g.pos[size_t(r)], s2p[size_t(r)]);
    std::sort(bypos.begin(), bypos.end());
    for (const auto &pp : bypos) src[size_t(pp.second)].push_back(4u * uint32_t(pp.first));
    struct Item {
        int32_t pdf, lg;
    };
    std::vector<Item> items;
    for (int32_t p = 0; p < P1; ++p) {
        const size_t n = src[size_t(p)].size();
        if (n == 0) continue;  // (no state emits it: its sum stays zero(K), the buffers start that way)
        int lg = 0;
        while ((size_t(4) << lg) < n) ++lg;
        if (lg > 6) return 0;
        items.push_back({p, lg});
    }
    std::stable_sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.lg > b.lg; });
    const uint32_t trash_src = 4u * uint32_t(S1), trash_pdf = 4u * uint32_t((P1 + 3) & ~3);
    tab.assign(size_t(4) * 2 * 5 * 64, 0u);
    for (int w = 0; w < 4; ++w)
        for (int j = 0; j < 2; ++j) {
            for (int k = 0; k < 4; ++k)
                for (int l = 0; l < 64; ++l) tab[size_t(((w * 2 + j) * 5 + k) * 64 + l)] = trash_src;
            for (int l = 0; l < 64; ++l) tab[size_t(((w * 2 + j) * 5 + 4) * 64 + l)] = trash_pdf;
        }
    int seg = 0, lane = 0;
    for (const Item &it : items) {
        const int L = 1 << it.lg;
        if (lane + L > 64) {
            ++seg;
            lane = 0;
        }
        if (seg >= 8) return 0;
        const int w = 3 - seg % 4, j = seg / 4;  // (the largest groups to the last wave: the first has the widest rows of the graph)
        const std::vector<uint32_t> &sv = src[size_t(it.pdf)];
        for (int i = 0; i < L; ++i) {
            for (int k = 0; k < 4; ++k) {
                const size_t q = size_t(4 * i + k);
                if (q < sv.size()) tab[size_t(((w * 2 + j) * 5 + k) * 64 + lane + i)] = sv[q];
            }
            tab[size_t(((w * 2 + j) * 5 + 4) * 64 + lane + i)] = (i == 0 ? 4u * uint32_t(it.pdf) : trash_pdf) | (uint32_t(it.lg) << 16);
        }
        lane += L;
    }
    const int nseg = items.empty() ? 1 : seg + 1;
    return nseg <= 4 ? 1 : 2;
}

// host part of the wave forms (no device call: mm_batch_create runs it for the FSMs of a batch on several host threads --
// an LF-MMI step brings a batch of numerator graphs that were never seen before, and packing them one after the other
// cost 150 ms per 128 graphs against 0.4 ms of kernel time).  Leaves the packed forms with the FSM (stage Packed),
// or nothing if it does not fit them.
static void wave_pack(mm_fsm_t f) {
    Once<RowForms> &o = f->wrows;
    if (o.stage != o.New) return;
    o.stage = o.Packed;
    if (f->semiring != MM_LOG || f->P1 > 256 || f->qmat[0].rowptr.empty()) return;
    const RowPackOpts opt = wave_pack_opts(true);
    RowForms rv = pack_both(f, opt, opt, true);
    for (int d = 0; d < 2 && rv; ++d) {
        rv[d].pdf_nps = wave_pdf_table(rv[d].g, f->s2p, f->S1, f->P1, rv[d].ptab);
        if (rv[d].pdf_nps <= 0) rv.reset();
    }
    o.form = std::move(rv);
}

// the wave forms of an FSM (built once; *ok = false if it does not fit them: more than 16 segments of 64 rows, ...)
static int wave_variants(mm_fsm_t f, const DebugOpts &dbg, bool *ok) {
    Once<RowForms> &o = f->wrows;
    wave_pack(f);  // (unless a worker thread has: try_wave, mm_fsm_create_many)
    if (!o.first(ok)) return MM_OK;
    RowForms rv = std::move(o.form);
    if (!rv) return MM_OK;
    for (int d = 0; d < 2; ++d) {
        if (dbg.verbose)
            fprintf(stderr, "[mm] wave form dir %d: %d segments, arcs/slots %.3f, LDS cycles/gather (bank model) %.2f -> %.2f\n", d,
                    rv[d].g.nslotrows - 2, rv[d].g.pad_eff, rv[d].g.conflict_before, rv[d].g.conflict_after);
        int rc = upload_row_variant(f, rv[d], 0.f, false);
        if (rc) return rc;
    }
    o.form = std::move(rv);
    *ok = true;
    return MM_OK;
}

// the split pair forms of an FSM for teams of H workgroups (built once per H; *ok = false if it does not fit them)
static int split_hidx(int H) { return H == 8 ? 2 : (H == 4 ? 1 : 0); }
static const RowVariant &split_row(mm_fsm_t f, int d, int set) { return f->srows[split_hidx(f->split.H)].form[d * f->split.H + set]; }
static int split_variants(mm_fsm_t f, const DebugOpts &dbg, int H, bool *ok) {
    if (!f->srows[split_hidx(H)].first(ok) || f->split.H) return MM_OK;  // (one team size per FSM: the first that fits)
    if (f->semiring != MM_LOG || !f->fast_ok || mm_pair_nj(f->P1, H) == 0 || H > MM_SPLIT_HMAX) return MM_OK;
    RowPackOpts opt, optb;
    split_pack_opts(dbg, opt, optb, H);
    std::vector<RowGraph> gs;
    SplitInfo info;
    if (!make_rows_split(H, f->S1, f->qmat[0].rowptr, f->qmat[0].col, f->qmat[0].val, f->qmat[1].rowptr, f->qmat[1].col,
                         f->qmat[1].val, f->s2p, f->P1, opt, optb, gs, info)) {
        if (dbg.verbose) fprintf(stderr, "[mm] split forms for teams of %d: the graph does not fit them\n", H);
        return MM_OK;
    }
    float wmin = 0.f;
    for (const RowGraph &g : gs) wmin = std::min(wmin, g.wmin_log2);
    if (wmin < -60.f) return MM_OK;  // (as for the row forms: too little of the float range would be left to the values)
    for (int h = 0; h < H; ++h)
        if (size_t(info.count[h] + 1) * 8 > size_t(mm_split_rsh(H))) {
            if (dbg.verbose) fprintf(stderr, "[mm] split forms for teams of %d: set %d has %d rows\n", H, h, info.count[h]);
            return MM_OK;
        }
    const float NINF = -std::numeric_limits<float>::infinity();
    RowForms rv = std::make_unique<RowVariant[]>(size_t(2 * H));
    for (int d = 0; d < 2; ++d) {
        // rowpdf / init by position of the TEAM's vector (0xffff / -inf at the alignment padding between the regions)
        std::vector<uint16_t> rowpdf_g(size_t(info.total) + 1, uint16_t(0xffff));
        std::vector<float> init_g(size_t(info.total) + 1, NINF);
        for (int64_t r = 0; r < f->S1; ++r) {
            rowpdf_g[size_t(info.gpos[d][size_t(r)])] = uint16_t(f->s2p[size_t(r)]);
            if (d == 0) init_g[size_t(info.gpos[d][size_t(r)])] = f->init[size_t(r)];
        }
        for (int h = 0; h < H; ++h) {
            RowVariant &v = rv[size_t(d * H + h)];
            v.g = std::move(gs[size_t(d * H + h)]);
            if (dbg.verbose)
                fprintf(stderr, "[mm] split form dir %d set %d/%d: %d rows at %d, KA %d, %d compute waves, %d segments, arcs/slots %.3f, "
                                "cost %d..%d, LDS cycles/gather (bank model) %.2f -> %.2f\n",
                        d, h, H, info.count[h], info.base[h], v.g.KA, v.g.NWC, v.g.nslotrows - 2, v.g.pad_eff, v.g.mincost,
                        v.g.maxcost, v.g.conflict_before, v.g.conflict_after);
            v.g.rowpdf = rowpdf_g;
            v.init = init_g;
            int rc = upload_row_variant(f, v, 125.f + wmin);
            if (rc) return rc;
            v.rdev.rows = info.total;  // (the team's vector, not the set's)
            v.rdev.fpos = info.gpos[d][size_t(f->S1 - 1)];
        }
    }
    f->srows[split_hidx(H)].form = std::move(rv);
    f->split = std::move(info);
    *ok = true;
    return MM_OK;
}

// (the forms free themselves with the FSM)
int mm_fsm_destroy(mm_fsm_t f) {
    if (!f) return MM_OK;
    if (f->log_twin) (void)mm_fsm_destroy(f->log_twin);
    for (void *&d : f->gen.dev)
        if (d) {
            mm_generic_free(d);
            d = nullptr;
        }
    delete f;
    return MM_OK;
}

int mm_fsm_info(mm_fsm_t f, int64_t *S1, int64_t *nnz, int32_t *P1, int64_t packed_slots[2], int64_t packed_items[2]) {
    if (!f) return fail(MM_ERR_INVALID, "mm_fsm_info: NULL handle");
    if (S1) *S1 = f->S1;
    if (nnz) *nnz = f->nnz;
    if (P1) *P1 = f->P1;
    for (int d = 0; d < 2; ++d) {
        ensure_packed(f);
        if (packed_slots) packed_slots[d] = f->packed[d].n_slot_rows * 64;
        if (packed_items) packed_items[d] = int64_t(f->packed[d].items.size());
    }
    return MM_OK;
}

int mm_debug_packed_product(mm_fsm_t f, int direction, const float *in, float *out, int32_t *argmax) {
    if (!f || !in || !out || direction < 0 || direction > 1) return fail(MM_ERR_INVALID, "mm_debug_packed_product");
    std::vector<float> x(f->S1);
    const float s = f->semiring == MM_LOG ? MM_LOG2E : 1.0f;
    for (int64_t i = 0; i < f->S1; ++i) x[i] = in[i] * s;
    ensure_packed(f);
    eval_packed(f->packed[direction], f->semiring, x.data(), out, argmax, f->S1);
    if (f->semiring == MM_LOG)
        for (int64_t i = 0; i < f->S1; ++i) out[i] *= MM_LN2;
    return MM_OK;
}

int mm_debug_reach_distance(mm_fsm_t f, int direction, int32_t *out) {
    if (!f || !out || direction < 0 || direction > 1) return fail(MM_ERR_INVALID, "mm_debug_reach_distance: bad argument");
    if (f->qmat[0].rowptr.empty()) return fail(MM_ERR_INVALID, "mm_debug_reach_distance: log-semiring FSMs only");
    std::vector<int32_t> seeds;
    if (direction == 0) {
        for (int64_t s = 0; s < f->S1; ++s)
            if (f->init[s] > -std::numeric_limits<float>::infinity()) seeds.push_back(int32_t(s));
    } else {
        seeds.push_back(int32_t(f->S1 - 1));
    }
    const std::vector<uint16_t> d = reach_distance(f->S1, f->qmat[1 - direction].rowptr, f->qmat[1 - direction].col, seeds);
    for (int64_t s = 0; s < f->S1; ++s) out[s] = d[s] == 0xffff ? -1 : int32_t(d[s]);
    return MM_OK;
}

int mm_debug_quad_product(mm_fsm_t f, int direction, int KQ, const float *in, float *out, double stats[4]) {
    if (!f || !in || !out || direction < 0 || direction > 1 || KQ < 1 || KQ > 32)
        return fail(MM_ERR_INVALID, "mm_debug_quad_product: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_quad_product: log-semiring FSMs only");
    const Csr &m = f->mat[direction];
    QuadGraph g = make_quads(f->S1, m.rowptr, m.col, m.val, f->s2p, f->P1, direction == 1, KQ);
    const int64_t S1 = f->S1, nq = int64_t(g.quads.size());
    // p = 2^(in * log2e - max) in the internal numbering
    float mx = -std::numeric_limits<float>::infinity();
    for (int64_t s = 0; s < S1; ++s) mx = std::max(mx, in[s] * MM_LOG2E);
    if (!(mx > -std::numeric_limits<float>::infinity())) mx = 0.f;
    std::vector<float> p(S1), qs(nq, 0.f);
    for (int64_t i = 0; i < S1; ++i) p[i] = std::exp2(in[g.order[i]] * MM_LOG2E - mx);
    const int64_t lanes = (nq + KQ - 1) / KQ;
    for (int64_t l = 0; l < lanes; ++l) {
        const uint32_t mask = g.quads[size_t(l * KQ)].mask;
        float run = 0.f;
        for (int j = 0; j < KQ && l * KQ + j < nq; ++j) {
            const Quad &q = g.quads[size_t(l * KQ + j)];
            float s = 0.f;
            const bool cont = std::signbit(q.wl[0]);
            if (cont != bool((mask >> j) & 1u)) return fail(MM_ERR_INVALID, "mm_debug_quad_product: sign flags and lane mask disagree");
            for (int k = 0; k < 4; ++k)
                s = std::fmaf(std::fabs(q.wl[k]), p[(q.off[k] / 4) % quad_pstride(f->S1p, g.ncopy)], s);
            run = cont ? run + s : s;
            qs[size_t(l * KQ + j)] = run;
        }
    }
    for (int64_t i = 0; i < S1; ++i) {
        const RowRec &r = g.recs[i];
        float acc = 0.f;
        if (r.qe) {  // the kernel's row_total(): qs2 = {0, 0, qs...}
            auto at = [&](int idx) { return idx < MM_QS_PAD ? 0.f : qs[size_t(idx - MM_QS_PAD)]; };
            if (r.i2 == MM_ROW_LONG) {
                acc = at(r.qe);
                for (int q = r.i1; q < r.qe; q += KQ) acc += at(q);
            } else {
                acc = at(r.qe) + (at(r.i1) + at(r.i2));
            }
        }
        out[g.order[i]] = (std::log2(acc) + mx) * MM_LN2;
    }
    if (stats) {
        stats[0] = double(nq);
        stats[1] = double(lanes);
        stats[2] = g.conflict_before;
        stats[3] = g.conflict_after;
    }
    return MM_OK;
}

int mm_debug_quad_layout(mm_fsm_t f, int direction, int KQ, int32_t *order, uint16_t *recs) {
    if (!f || !order || !recs || direction < 0 || direction > 1 || KQ < 1 || KQ > 32)
        return fail(MM_ERR_INVALID, "mm_debug_quad_layout: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_quad_layout: log-semiring FSMs only");
    const Csr &m = f->mat[direction];
    const QuadGraph g = make_quads(f->S1, m.rowptr, m.col, m.val, f->s2p, f->P1, direction == 1, KQ);
    for (int64_t i = 0; i < f->S1; ++i) {
        order[i] = g.order[size_t(i)];
        const RowRec &r = g.recs[size_t(i)];
        recs[4 * i + 0] = r.qe;
        recs[4 * i + 1] = r.i1;
        recs[4 * i + 2] = r.pdf;
        recs[4 * i + 3] = r.i2;
    }
    return MM_OK;
}

int mm_debug_row_product(mm_fsm_t f, int direction, const float *in, float *out, double stats[8]) {
    return mm_debug_row_product_ex(f, direction, 0, in, out, stats);
}

int mm_debug_row_product_ex(mm_fsm_t f, int direction, int flags, const float *in, float *out, double stats[8]) {
    if (!f || !in || !out || direction < 0 || direction > 1 || flags < 0 || flags > 31)
        return fail(MM_ERR_INVALID, "mm_debug_row_product: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_row_product: log-semiring FSMs only");
    // The options of the forms that ship (row_pack_opts, pair_pack_opts), but: the matrices are mat[], not the pruned qmat[]; of the
    // debug switches only the process's MM_NO_PDF_HALVES is read; the row form's KA is not rounded to a register window and the pair
    // form's backward group_speed stays 1; the forward numbering of a backward pair product is packed with the backward options
    // (finish_cost 24); copies, copy_perm and bank_opt are the caller's flags.
    DebugOpts dbg;
    dbg.no_pdf_halves = process_debug_opts().no_pdf_halves;
    RowPackOpts opt = (flags & 1) ? pair_pack_opts(dbg, direction, false) : row_pack_opts(false);
    opt.copies = (flags >> 1) & 3;
    opt.copy_perm = (flags & 8) != 0;
    opt.bank_opt = (flags & 16) ? 1 : 0;
    if (opt.copies > 2) return fail(MM_ERR_INVALID, "mm_debug_row_product: at most two copies");
    RowGraph gf, g;
    const std::vector<int32_t> none;
    const Csr &mf = f->mat[0], &m = f->mat[direction];
    if ((f->S1 + 1) * 4 > MM_ROW_RS || !make_rows(f->S1, mf.rowptr, mf.col, mf.val, f->s2p, f->P1, false, none, opt, gf))
        return fail(MM_ERR_UNSUPPORTED, "mm_debug_row_product: the FSM does not fit the row-lane form");
    if (direction == 1) {
        if (!make_rows(f->S1, m.rowptr, m.col, m.val, f->s2p, f->P1, true, gf.pos, opt, g))
            return fail(MM_ERR_UNSUPPORTED, "mm_debug_row_product: the FSM does not fit the row-lane form");
    } else {
        g = gf;
    }
    const int64_t S1 = f->S1;
    float mx = -std::numeric_limits<float>::infinity();
    for (int64_t s = 0; s < S1; ++s) mx = std::max(mx, in[s] * MM_LOG2E);
    if (!(mx > -std::numeric_limits<float>::infinity())) mx = 0.f;
    std::vector<float> pl(S1 + 1, 0.f), ol(S1 + 1, 0.f);
    for (int64_t i = 0; i < S1; ++i) pl[i] = std::exp2(in[g.order[i]] * MM_LOG2E - mx);
    eval_rows(g, pl.data(), ol.data());
    for (int64_t i = 0; i < S1; ++i) out[g.order[i]] = (std::log2(ol[i]) + mx) * MM_LN2;
    if (stats) {
        stats[0] = g.KA;
        stats[1] = g.NWC;
        stats[2] = g.nslotrows - 2;
        stats[3] = g.pad_eff;
        stats[4] = g.maxcost;
        stats[5] = g.mincost;
        stats[6] = g.conflict_before;
        stats[7] = g.conflict_after;
    }
    return MM_OK;
}

int mm_debug_pair_pdftab(mm_fsm_t f, int direction, int64_t *rows, uint32_t *tab, uint16_t *pdfse, uint32_t *slots) {
    if (!f || direction < 0 || direction > 1 || !rows || !tab || !pdfse || !slots) return fail(MM_ERR_INVALID, "mm_debug_pair_pdftab: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_pair_pdftab: log-semiring FSMs only");
    // both directions as pack_both() builds them (the forward form's partner halves come from the backward numbering), with the
    // options and matrices of mm_debug_row_product_ex
    DebugOpts dbg;
    dbg.no_pdf_halves = process_debug_opts().no_pdf_halves;
    RowGraph g[2];
    const std::vector<int32_t> none;
    const Csr *m = f->mat;
    if ((f->S1 + 1) * 4 > MM_ROW_RS || !make_rows(f->S1, m[0].rowptr, m[0].col, m[0].val, f->s2p, f->P1, false, none, pair_pack_opts(dbg, 0, false), g[0]) ||
        !make_rows(f->S1, m[1].rowptr, m[1].col, m[1].val, f->s2p, f->P1, true, g[0].pos, pair_pack_opts(dbg, 1, false), g[1]))
        return fail(MM_ERR_UNSUPPORTED, "mm_debug_pair_pdftab: the FSM does not fit the pair form");
    set_partner(g[0], g[1].pos);
    const RowGraph &r = g[direction];
    if (int64_t(r.pdftab.size()) != f->S1 || int64_t(r.pdfse.size()) != 2 * f->P1) return fail(MM_ERR_UNSUPPORTED, "mm_debug_pair_pdftab: table sizes");
    *rows = f->S1;
    std::copy(r.pdftab.begin(), r.pdftab.end(), tab);
    std::copy(r.pdfse.begin(), r.pdfse.end(), pdfse);
    int64_t n = 0;
    for (size_t e = 0; e + 1 < r.slots.size(); e += 2) {
        if (int((r.slots[e] & 0xffffu) / uint32_t(r.scale)) == r.trash) continue;
        if (n < f->S1) slots[2 * n] = r.slots[e], slots[2 * n + 1] = r.slots[e + 1];
        ++n;
    }
    if (n != f->S1) return fail(MM_ERR_UNSUPPORTED, "mm_debug_pair_pdftab: finishing lanes");
    return MM_OK;
}

int mm_debug_stream_product(mm_fsm_t f, int direction, const float *in, float *out, double stats[4]) {
    if (!f || !in || !out || (direction != 0 && direction != 1)) return fail(MM_ERR_INVALID, "mm_debug_stream_product: bad argument");
    return mm_debug_stream_team_product(f, 1, direction, in, out, stats);
}

int mm_debug_stream_team_product(mm_fsm_t f, int H, int direction, const float *in, float *out, double stats[4]) {
    if (!f || !in || !out || (direction != 0 && direction != 1) || (H != 1 && H != 2 && H != 4))
        return fail(MM_ERR_INVALID, "mm_debug_stream_team_product: bad argument");
    return no_throw("mm_debug_stream_team_product", [&]() {
        bool ok = false;
        int rc = stream_variant(f, H, &ok);
        if (rc) return rc;
        if (!ok) return fail(MM_ERR_UNSUPPORTED, "mm_debug_stream_team_product: the FSM does not fit the stream form");
        mm_stream_eval(f->stream_h[stream_hidx(H)].form.get(), direction, in, out, stats);
        return int(MM_OK);
    });
}

int mm_debug_wave_product(mm_fsm_t f, int direction, const float *in, float *out, double stats[4]) {
    if (!f || !in || !out || direction < 0 || direction > 1) return fail(MM_ERR_INVALID, "mm_debug_wave_product: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_wave_product: log-semiring FSMs only");
    // (the options of wave_pack but for place, naive_stats, q_positions -- the packer's defaults here; mat[], not the pruned qmat[])
    const RowPackOpts opt = wave_pack_opts(false);
    RowGraph gf, g;
    const std::vector<int32_t> none;
    if (!make_rows(f->S1, f->mat[0].rowptr, f->mat[0].col, f->mat[0].val, f->s2p, f->P1, false, none, opt, gf) ||
        (direction == 1 && !make_rows(f->S1, f->mat[1].rowptr, f->mat[1].col, f->mat[1].val, f->s2p, f->P1, true, gf.pos, opt, g)))
        return fail(MM_ERR_UNSUPPORTED, "mm_debug_wave_product: the FSM does not fit the wave form");
    if (direction == 0) g = gf;
    {   // (what wave_pack refuses beyond the rows: more than 256 pdfs, a pdf of more than 256 states, more than 8 pdf segments)
        std::vector<uint32_t> tab;
        if (f->P1 > 256 || wave_pdf_table(g, f->s2p, f->S1, f->P1, tab) <= 0)
            return fail(MM_ERR_UNSUPPORTED, "mm_debug_wave_product: the FSM's pdf sums do not fit the wave form");
    }
    const float NINF = -std::numeric_limits<float>::infinity();
    std::vector<float> x(size_t(f->S1) + 1, NINF), y(size_t(f->S1) + 1, NINF);
    for (int64_t i = 0; i < f->S1; ++i) x[size_t(i)] = in[g.order[size_t(i)]] * MM_LOG2E;
    eval_rows_log(g, 4, x.data(), y.data());
    for (int64_t i = 0; i < f->S1; ++i) out[g.order[size_t(i)]] = y[size_t(i)] * MM_LN2;
    if (stats) {
        stats[0] = g.KA;
        stats[1] = g.nslotrows - 2;
        stats[2] = g.pad_eff;
        stats[3] = g.conflict_after;
    }
    return MM_OK;
}

int mm_debug_split_product(mm_fsm_t f, int H, int direction, const float *in, float *out, double stats[8]) {
    if (!f || !in || !out || direction < 0 || direction > 1 || H < 2 || H > 8)
        return fail(MM_ERR_INVALID, "mm_debug_split_product: bad argument");
    if (f->semiring != MM_LOG) return fail(MM_ERR_INVALID, "mm_debug_split_product: log-semiring FSMs only");
    RowPackOpts opt, optb;
    split_pack_opts(DebugOpts(), opt, optb, H);  // (no debug switch is read; mat[], not the pruned qmat[])
    std::vector<RowGraph> gs;
    SplitInfo info;
    if (!make_rows_split(H, f->S1, f->mat[0].rowptr, f->mat[0].col, f->mat[0].val, f->mat[1].rowptr, f->mat[1].col,
                         f->mat[1].val, f->s2p, f->P1, opt, optb, gs, info))
        return fail(MM_ERR_UNSUPPORTED, "mm_debug_split_product: the FSM does not fit the split forms");
    const int64_t S1 = f->S1;
    float mx = -std::numeric_limits<float>::infinity();
    for (int64_t s = 0; s < S1; ++s) mx = std::max(mx, in[s] * MM_LOG2E);
    if (!(mx > -std::numeric_limits<float>::infinity())) mx = 0.f;
    std::vector<float> pl(size_t(info.total) + 1, 0.f), ol(size_t(info.total) + 1, 0.f);
    for (int64_t r = 0; r < S1; ++r) pl[size_t(info.gpos[direction][size_t(r)])] = std::exp2(in[r] * MM_LOG2E - mx);
    double ka = 0, segs = 0, eff = 0, maxc = 0, minc = 1e30, cb = 0, ca = 0;
    for (int h = 0; h < H; ++h) {
        const RowGraph &g = gs[size_t(direction * H + h)];
        eval_rows(g, pl.data(), ol.data());
        ka = std::max(ka, double(g.KA));
        segs += g.nslotrows - 2;
        eff += g.pad_eff / H;
        maxc = std::max(maxc, double(g.maxcost));
        minc = std::min(minc, double(g.mincost));
        cb += g.conflict_before / H;
        ca += g.conflict_after / H;
    }
    for (int64_t r = 0; r < S1; ++r) out[r] = (std::log2(ol[size_t(info.gpos[direction][size_t(r)])]) + mx) * MM_LN2;
    if (stats) {
        stats[0] = ka;
        stats[1] = double(info.total);
        stats[2] = segs;
        stats[3] = eff;
        stats[4] = maxc;
        stats[5] = minc;
        stats[6] = cb;
        stats[7] = ca;
    }
    return MM_OK;
}

int mm_fsm_create(int semiring, int64_t S1, int64_t nnz, int layout, int index_bytes, int index_base, int val_bytes,
                  const void *ptr, const void *idx, const void *val, int64_t n_init, const void *init_idx,
                  const void *init_val, const int32_t *state2pdf, int32_t P1, mm_fsm_t *out) {
    return no_throw("mm_fsm_create", [&]() {
        return fsm_create_impl(semiring, S1, nnz, layout, index_bytes, index_base, val_bytes, ptr, idx, val, n_init, init_idx, init_val,
                               state2pdf, P1, out);
    });
}

// Pinned staging buffer of mm_fsm_create_many (grow only; one upload at a time).
namespace {
std::mutex g_stage_lock;
char *g_stage = nullptr;
size_t g_stage_bytes = 0;
}  // namespace

extern "C" std::atomic<long long> mm_rows_prof_ns[8];  // (mm_rows.cpp: where the time of make_rows goes, MM_VERBOSE)
static int fsm_create_many_impl(int64_t n, int semiring, int layout, int index_bytes, int index_base, int val_bytes, const int64_t *S1,
                                const int64_t *nnz, const void *const *ptr, const void *const *idx, const void *const *val,
                                const int64_t *n_init, const void *const *init_idx, const void *const *init_val,
                                const int32_t *const *state2pdf, const int32_t *P1, int threads, mm_fsm_t *out) {
    if (!out || n < 1) return fail(MM_ERR_INVALID, "mm_fsm_create_many: bad argument");
    for (int64_t i = 0; i < n; ++i) out[i] = nullptr;
    if (!S1 || !nnz || !ptr || !idx || !val || !n_init || !init_idx || !init_val || !state2pdf || !P1)
        return fail(MM_ERR_INVALID, "mm_fsm_create_many: NULL array");
    const bool verbose = process_debug_opts().verbose;
    const auto tc0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (verbose) fprintf(stderr, "[mm] create_many: %s at %.2f ms\n", what, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count());
    };
    const size_t nthr = size_t(std::max(1, std::min<int>({threads > 0 ? threads : 16, int(std::max(1u, std::thread::hardware_concurrency())), int((n + 3) / 4), 64})));
    std::vector<int> rcs(static_cast<size_t>(n), MM_OK);
    std::vector<std::string> msgs{size_t(n), std::string()};
    std::vector<size_t> bytes(static_cast<size_t>(n), 0);  // device bytes of the FSM's wave forms (0: none)
    // ---- 1. every graph on a host thread: the FSM (mm_fsm_create), its wave forms, the size of their device image
    auto run_pool = [&](auto &&body) {
        std::atomic<int64_t> next{0};
        auto work = [&]() {
            for (int64_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) body(i);
        };
        if (nthr <= 1) {
            work();
            return;
        }
        std::vector<std::thread> pool;
        for (size_t t = 0; t < nthr; ++t) pool.emplace_back(work);
        for (std::thread &t : pool) t.join();
    };
    std::atomic<long long> ns_create{0}, ns_pack{0};
    run_pool([&](int64_t i) {
        try {
            const auto ta = std::chrono::steady_clock::now();
            rcs[size_t(i)] = fsm_create_impl(semiring, S1[i], nnz[i], layout, index_bytes, index_base, val_bytes, ptr[i], idx[i], val[i], n_init[i],
                                             init_idx[i], init_val[i], state2pdf[i], P1[i], &out[i]);
            if (rcs[size_t(i)]) {
                msgs[size_t(i)] = mm_last_error();
                return;
            }
            mm_fsm_t f = out[i];
            const auto tb = std::chrono::steady_clock::now();
            ns_create += std::chrono::duration_cast<std::chrono::nanoseconds>(tb - ta).count();
            if (f->semiring == MM_LOG && f->P1 <= 250 && f->S1 <= 1023 && f->qmat[0].rowptr[size_t(f->S1)] <= 16 * 64 * 4) {
                wave_pack(f);
                ns_pack += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tb).count();
                if (f->wrows.form) {
                    size_t tot = 0;
                    for (int d = 0; d < 2; ++d) {
                        RowBlob rb;
                        rb.bl.dry = true;
                        row_variant_blob(f->wrows.form[d], false, rb);
                        tot += align_up(rb.bl.size(), 256);
                    }
                    bytes[size_t(i)] = tot;
                }
            }
        } catch (const std::exception &e) {
            rcs[size_t(i)] = MM_ERR_NOMEM;
            msgs[size_t(i)] = std::string("mm_fsm_create_many: ") + e.what();
        }
    });
    lap("graphs compiled and packed");
    if (verbose) {
        fprintf(stderr, "[mm] make_rows sections (us per graph): plan %.0f, numbering %.0f, csr %.0f, slots+placement %.0f\n", 1e-3 * double(mm_rows_prof_ns[0].exchange(0)) / double(n),
                1e-3 * double(mm_rows_prof_ns[1].exchange(0)) / double(n), 1e-3 * double(mm_rows_prof_ns[2].exchange(0)) / double(n), 1e-3 * double(mm_rows_prof_ns[3].exchange(0)) / double(n));
    }
    if (verbose) fprintf(stderr, "[mm] create_many: per graph %.0f us mm_fsm_create + %.0f us wave forms (%zu threads)\n", 1e-3 * double(ns_create.load()) / double(n), 1e-3 * double(ns_pack.load()) / double(n), nthr);
    auto undo = [&](int rc, const std::string &msg) {
        for (int64_t i = 0; i < n; ++i)
            if (out[i]) {
                (void)mm_fsm_destroy(out[i]);
                out[i] = nullptr;
            }
        return fail(rc, msg);
    };
    for (int64_t i = 0; i < n; ++i)
        if (rcs[size_t(i)]) return undo(rcs[size_t(i)], "graph " + std::to_string(i) + ": " + msgs[size_t(i)]);
    // ---- 2. ONE device allocation and ONE copy for the wave forms of all graphs
    std::vector<size_t> off(size_t(n) + 1, 0);
    for (int64_t i = 0; i < n; ++i) off[size_t(i) + 1] = off[size_t(i)] + bytes[size_t(i)];
    const size_t total = off[size_t(n)];
    if (total == 0) return MM_OK;
    {   // (without a device the packed forms stay with their FSMs, like after mm_fsm_create: mm_batch_create uploads them)
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
            (void)hipGetLastError();
            return MM_OK;
        }
    }
    void *dev = nullptr;
    if (hipMalloc(&dev, total) != hipSuccess) return undo(MM_ERR_HIP, "mm_fsm_create_many: device allocation failed");
    std::shared_ptr<void> arena(dev, HipFree());
    lap("arena allocated");
    std::lock_guard<std::mutex> guard(g_stage_lock);
    if (g_stage_bytes < total) {
        if (g_stage) (void)hipHostFree(g_stage);
        g_stage = nullptr;
        g_stage_bytes = 0;
        void *q = nullptr;
        const size_t want = std::max(total + total / 2, size_t(1) << 22);
        if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) return undo(MM_ERR_HIP, "mm_fsm_create_many: staging allocation failed");
        g_stage = static_cast<char *>(q);
        g_stage_bytes = want;
    }
    std::vector<RowBlob> rbs(size_t(n) * 2);
    run_pool([&](int64_t i) {
        if (!bytes[size_t(i)]) return;
        mm_fsm_t f = out[i];
        size_t o = off[size_t(i)];
        for (int d = 0; d < 2; ++d) {
            RowBlob &rb = rbs[size_t(i) * 2 + d];
            rb.bl.ext = g_stage + o;
            row_variant_blob(f->wrows.form[d], false, rb);
            o += align_up(rb.bl.size(), 256);
        }
    });
    lap("staged");
    if (hipMemcpy(dev, g_stage, total, hipMemcpyHostToDevice) != hipSuccess) return undo(MM_ERR_HIP, "mm_fsm_create_many: upload failed");
    lap("uploaded");
    for (int64_t i = 0; i < n; ++i) {
        if (!bytes[size_t(i)]) continue;
        mm_fsm_t f = out[i];
        size_t o = off[size_t(i)];
        for (int d = 0; d < 2; ++d) {
            RowVariant &rv = f->wrows.form[d];
            const RowBlob &rb = rbs[size_t(i) * 2 + d];
            rv.mem = arena;
            row_variant_bind(f, rv, rb, static_cast<char *>(dev) + o, 0.f);
            o += align_up(rb.bl.size(), 256);
        }
        f->wrows.stage = f->wrows.Tried;
    }
    return MM_OK;
}

int mm_fsm_create_many(int64_t n, int semiring, int layout, int index_bytes, int index_base, int val_bytes, const int64_t *S1,
                       const int64_t *nnz, const void *const *ptr, const void *const *idx, const void *const *val, const int64_t *n_init,
                       const void *const *init_idx, const void *const *init_val, const int32_t *const *state2pdf, const int32_t *P1,
                       int threads, mm_fsm_t *out) {
    return no_throw("mm_fsm_create_many", [&]() {
        return fsm_create_many_impl(n, semiring, layout, index_bytes, index_base, val_bytes, S1, nnz, ptr, idx, val, n_init, init_idx, init_val,
                                    state2pdf, P1, threads, out);
    });
}

// a batch of ProbSemiring FSMs answers for its settings and counters through the batch of its log twins (what runs its fast calls)
static mm_batch_t twin_of(mm_batch_t h) { return h && h->log_twin ? h->log_twin : h; }

// The wave forms of every FSM of the batch (packed on the host's cores for the FSMs that are new): *ok, h->wave_nseg.
static int try_wave(mm_batch_t h, const mm_fsm_t *fsms, bool *ok) {
    const int64_t B = h->B;
    *ok = true;
    {   // pack the forms of the FSMs that are new, on the host's cores
        std::vector<mm_fsm_t> todo;
        for (int64_t b = 0; b < B; ++b)
            if (fsms[b]->wrows.stage == fsms[b]->wrows.New &&
                std::find(todo.begin(), todo.end(), fsms[b]) == todo.end())
                todo.push_back(fsms[b]);
        const size_t nthr = std::min<size_t>({todo.size() / 4, size_t(std::max(1u, std::thread::hardware_concurrency())), size_t(16)});
        if (nthr > 1) {
            std::atomic<size_t> next{0};
            std::vector<std::thread> pool;
            for (size_t t = 0; t < nthr; ++t)
                pool.emplace_back([&]() {
                    // (an exception must not leave a thread: an FSM whose packing failed is packed again, and fails
                    // again, on the calling thread -- wave_variants below)
                    for (size_t i = next.fetch_add(1); i < todo.size(); i = next.fetch_add(1)) {
                        try {
                            wave_pack(todo[i]);
                        } catch (...) {
                            todo[i]->wrows.stage = todo[i]->wrows.New;
                        }
                    }
                });
            for (std::thread &t : pool) t.join();
        }
    }
    for (int64_t b = 0; b < B && *ok; ++b) {
        bool fit = false;
        int rc = wave_variants(fsms[b], h->dbg, &fit);
        if (rc) return rc;
        *ok = fit;
        // (segments of a wave's registers: the state segments, and twice the pdf segments -- the kernel has NSEG / 2 of those)
        if (fit)
            h->wave_nseg = std::max({h->wave_nseg, std::max(fsms[b]->wrows.form[0].g.KA, fsms[b]->wrows.form[1].g.KA) / 4,
                                     2 * std::max(fsms[b]->wrows.form[0].pdf_nps, fsms[b]->wrows.form[1].pdf_nps)});
    }
    return MM_OK;
}

// The kernel family of a log batch (h->fb), with the forms it needs packed, and what goes with it: h->lane_redo_wave, the wave,
// pair and stream geometries, h->quad_built, h->quad_ok.  *rows: every FSM has its row-lane forms (a batch of the pair kernels
// keeps them too).  Reads the quad geometry, h->xcsr and h->n_cus; nq_max, s1_max: the most quads per direction, states of one FSM.
static int pick_family(mm_batch_t h, const mm_fsm_t *fsms, const int64_t nq_max[2], int64_t s1_max, bool *rows_out) {
    const int64_t B = h->B;
    const int kernel = h->dbg.kernel;
    bool lane = false, wave = false, rows = false, pairs = false, stream = false, same = true;  // (same: one FSM shared by all utterances)
    for (int64_t b = 1; b < B && same; ++b) same = fsms[b] == fsms[0];
    // The wave kernel FIRST wherever every graph of the batch fits it (up to 1023 states, 16 segments of 64 lanes x 4 arcs
    // per direction, 250 pdfs): one workgroup per utterance runs both directions at once in the log domain, without the
    // marks and the exact second pass of the linear-domain kernels -- measured against the row kernels on batches of
    // different graphs (1.18 -> 0.72 ms: 128 lexicon graphs of 150..400 states, T = 700) and against the pair kernels on one
    // shared small graph (0.80 -> 0.47 ms: 300 states, B = 256, T = 500; 3-state HMM, B = 1, T = 100: 0.18 -> 0.06 ms).  The
    // exception: one shared DENSE graph (more than 16 arcs per state, more than 2 segments per wave) on a batch of more than
    // two utterances per compute unit, where the pair kernels' two utterances per workgroup win (32-state ergodic HMM,
    // B = 1024: 1.90 against 2.33 ms).
    // The lane kernel FIRST for batches of tiny graphs (every FSM: up to 64 states and 64 pdfs): one wave per utterance and
    // direction with the graph in its registers, float64, exact -- BASELINE config 2 (dense 64-state HMM, B = 32, T = 500):
    // 0.60 ms on the pair kernels; config 1 (3-state HMM, one utterance).
    if (h->semiring == MM_LOG && (kernel == DebugOpts::K_AUTO || kernel == DebugOpts::K_LANE)) {
        lane = true;
        for (int64_t b = 0; b < B && lane; ++b) {
            bool ok = false;
            int rc = lane_variant(fsms[b], &ok);
            if (rc) return rc;
            lane = ok;
            h->lane_S = std::max(h->lane_S, int(fsms[b]->S1 - 1));
        }
    }
    // What the lane kernel marks (mass beyond the double's range: the one path of a sharp left-to-right graph) is computed again in the
    // log domain: by the WAVE kernel when every graph has its wave forms (up to 4096 arc slots per direction; packed with the graph by
    // mm_fsm_create_many, nothing to upload at the first call, capturable from the first call on), else -- a dense 64-state HMM has
    // 4161 arcs -- by the item kernel, whose forms then go to the device here.
    if (lane) {
        int rc = try_wave(h, fsms, &h->lane_redo_wave);
        if (rc) return rc;
        if (!h->lane_redo_wave) h->wave_nseg = 0;
    }
    bool wave_first_tried = false;
    if (h->semiring == MM_LOG && kernel == DebugOpts::K_AUTO && !lane) {
        bool small = h->max_P1 <= 250;
        for (int64_t b = 0; b < B && small; ++b)
            small = fsms[b]->S1 <= 1023 && fsms[b]->qmat[0].rowptr[fsms[b]->S1] <= 16 * 64 * 4;
        const bool dense_many = same && B > 2 * int64_t(h->n_cus) && fsms[0]->qmat[0].rowptr[fsms[0]->S1] > 16 * fsms[0]->S1;
        if (small) {
            wave_first_tried = true;
            int rc = try_wave(h, fsms, &wave);
            if (rc) return rc;
            // (the exception; the forms stay with the FSM.  Graphs of up to 2 segments per wave run the kernel instance of
            // which two workgroups fit a compute unit and win at every batch size: 16-state ergodic HMM, B = 1024: 1.18
            // against 1.88 ms)
            if (wave && dense_many && h->wave_nseg > 2) wave = false;
        }
    }
    // row kernels: every FSM of the batch needs its row-lane forms.  Small deep (left-to-right) graphs keep states
    // alive whose values differ by more than the float range within one frame, so most of their rows would take the
    // exact fallback of the linear-domain kernels: they run on the item kernel (unless a kernel is forced).
    const bool linear_first = !wave && !lane && h->fast_ok && kernel != DebugOpts::K_ITEM && kernel != DebugOpts::K_QUAD &&
                              kernel != DebugOpts::K_WAVE && kernel != DebugOpts::K_STREAM &&
                              !(h->max_depth >= 64 && nq_max[0] <= 3 * 1024 && nq_max[1] <= 3 * 1024 && kernel == DebugOpts::K_AUTO);
    rows = linear_first;
    for (int64_t b = 0; b < B && rows; ++b) {
        bool ok = false;
        int rc = row_variants(fsms[b], h->dbg.verbose, &ok);
        if (rc) return rc;
        rows = ok;
    }
    // pair kernels: all utterances on ONE FSM (the graph registers are shared by the two utterances of a workgroup)
    // (a batch of ONE utterance too: its pair runs the utterance twice, the copy writes nothing outside the workspace -- both
    // directions at once instead of the row kernels' two passes: 4.1 -> 2.6 ms on config 3's graph)
    // (the row kernels take up to 250 pdfs, the pair kernels 506: a shared graph of more pdfs has no row forms)
    pairs = linear_first && same && (rows || h->max_P1 > 250) && kernel != DebugOpts::K_ROW && kernel != DebugOpts::K_SPLIT;
    if (pairs) {
        bool ok = false;
        int rc = pair_variants(fsms[0], h->dbg, &ok);
        if (rc) return rc;
        pairs = ok;
        if (ok) {
            h->pair_ka = std::max(fsms[0]->prows.form[0].g.KA, fsms[0]->prows.form[1].g.KA);
            h->pair_nwc = std::max(fsms[0]->prows.form[0].g.NWC, fsms[0]->prows.form[1].g.NWC);
            h->pair_slotrows = std::max(fsms[0]->prows.form[0].g.nslotrows, fsms[0]->prows.form[1].g.nslotrows);
            pairs = h->pair_ka <= MM_PAIR_KA && mm_pair_lds_bytes(1, h->pair_slotrows, h->max_P1) <= MM_LDS_MAX;
        }
    }
    // split pair kernels: one shared FSM that is too large for the pair kernels proper (more arcs than the registers of a
    // compute unit hold, more states than half its LDS) -- teams of 2 workgroups per utterance pair and direction
    if (linear_first && same && !pairs && kernel != DebugOpts::K_ROW) {
        bool ok = false;
        int rc = split_variants(fsms[0], h->dbg, 2, &ok);
        // (a graph beyond the teams of 2 -- more than 3070 states or 2 x 14 x 64 x 36 arcs: teams of 4; beyond those -- more
        // than 4094 states: teams of 8, up to 6014 states and 314 pdfs)
        if (!rc && !ok) rc = split_variants(fsms[0], h->dbg, 4, &ok);
        if (!rc && !ok) rc = split_variants(fsms[0], h->dbg, 8, &ok);
        if (rc) return rc;
        if (ok) {
            const mm_fsm_t f0 = fsms[0];
            h->pair_H = f0->split.H;
            h->pair_ka = 0;
            h->pair_nwc = 1;
            h->pair_slotrows = 0;
            for (int d = 0; d < 2; ++d)
                for (int s = 0; s < h->pair_H; ++s) {
                    h->pair_ka = std::max(h->pair_ka, split_row(f0, d, s).g.KA);
                    h->pair_nwc = std::max(h->pair_nwc, split_row(f0, d, s).g.NWC);
                    h->pair_slotrows = std::max(h->pair_slotrows, split_row(f0, d, s).g.nslotrows);
                }
            h->split_s1p = (f0->split.total + 2 + 3) & ~3;
            const size_t lds = mm_split_lds_bytes(h->pair_H, 1, h->pair_slotrows, h->max_P1);
            pairs = h->pair_ka <= mm_split_ka(h->pair_H) && h->pair_nwc <= MM_SPLIT_NWC && lds > 0 && lds <= MM_LDS_MAX;
            if (h->dbg.verbose) fprintf(stderr, "[mm] teams of %d: LDS %zu bytes in phase B\n", h->pair_H, lds);
            if (!pairs) h->pair_H = 1;
        }
    }
    // wave kernel, the other case: small graphs that none of the linear-domain kernels takes (deep left-to-right graphs:
    // numerators), or the kernel is asked for by name
    if (h->semiring == MM_LOG && !wave && !lane && !wave_first_tried && !rows && !pairs &&
        (kernel == DebugOpts::K_WAVE ||
         (kernel == DebugOpts::K_AUTO && (!h->fast_ok || (h->max_depth >= 64 && h->geo_kq[0] <= 3 && h->geo_kq[1] <= 3))))) {
        // (= where the item kernel would run: quad_kernel_usable() says no for these; see there)
        int rc = try_wave(h, fsms, &wave);
        if (rc) return rc;
    }
    // stream kernels (mm_stream.hip): graphs beyond every register-resident form and beyond the quad kernels' LDS (more than ~3000
    // states, more than 250 pdfs on different graphs / 506 on a shared one, weights outside the float range) -- what the item
    // kernel ran until round 5
    const bool beyond = s1_max > 3000 || h->max_P1 > 250 || !h->fast_ok;
    if (h->semiring == MM_LOG && !lane && !wave && !pairs && !rows &&
        (kernel == DebugOpts::K_STREAM || (kernel == DebugOpts::K_AUTO && beyond))) {
        stream = true;
        // teams of 2 or 4 workgroups per utterance and direction when the batch leaves compute units idle (round 6: a direction's
        // record stream through ONE compute unit's memory path is what bounds a frame)
        h->stream_H = (h->dbg.stream_h == 1 || h->dbg.stream_h == 2 || h->dbg.stream_h == 4) ? h->dbg.stream_h : mm_stream_pick_h(B, h->n_cus);
        for (int64_t b = 0; b < B && stream; ++b) {
            bool ok = false;
            int rc = stream_variant(fsms[b], h->stream_H, &ok);
            if (rc) return rc;
            stream = ok && mm_stream_dev(fsms[b]->stream_h[stream_hidx(h->stream_H)].form.get()) != nullptr;
        }
        h->stream_S1 = int(s1_max);
    }
    // (a batch of the wave kernel never runs the quad kernels, and one whose marked utterances go to the float64 pair kernels
    // has the item kernel behind those: their quad forms are not built)
    const bool want_dpair = pairs && !h->dbg.no_dpair;
    h->quad_built = h->fast_ok && !wave && !lane && !stream && !(want_dpair && kernel != DebugOpts::K_QUAD);
    h->quad_ok = quad_kernel_usable(h);
    h->fb = lane ? Fb::Lane : stream ? Fb::Stream : wave ? Fb::Wave : pairs ? (h->pair_H > 1 ? Fb::Split : Fb::Pairs) : rows ? Fb::Rows
          : h->quad_ok ? Fb::Quad : Fb::Item;
    *rows_out = rows;
    return MM_OK;
}

static int batch_create_impl(const mm_fsm_t *fsms, int64_t B, mm_batch_t *out) {
    if (!out) return fail(MM_ERR_INVALID, "mm_batch_create: out is NULL");
    *out = nullptr;
    if (!fsms || B < 1) return fail(MM_ERR_INVALID, "mm_batch_create: empty batch");
    const auto tb0 = std::chrono::steady_clock::now();
    for (int64_t b = 0; b < B; ++b) {
        if (!fsms[b]) return fail(MM_ERR_INVALID, "mm_batch_create: NULL FSM handle");
        if (fsms[b]->semiring != fsms[0]->semiring)
            return fail(MM_ERR_INVALID, "mm_batch_create: FSMs of one batch must share the semiring (FSM{K})");
    }
    // (owned here until it is handed out: every early return and every exception -- the packers allocate -- destroys it)
    struct Drop {
        void operator()(mm_batch_s *x) const { (void)mm_batch_destroy(x); }
    };
    std::unique_ptr<mm_batch_s, Drop> hold(new mm_batch_s());
    mm_batch_s *h = hold.get();
    h->dbg = read_debug_opts();
    h->B = B;
    h->semiring = fsms[0]->semiring;
    h->fsms.assign(fsms, fsms + B);
    if (hipGetDevice(&h->device) != hipSuccess) return fail(MM_ERR_HIP, "mm_batch_create: no device");
    if (h->semiring == MM_PROB) {  // the generic path (mm_pdfposteriors_ex): no kernel forms, no descriptors of its own
        bool twins = true;
        for (int64_t b = 0; b < B; ++b) {
            h->total_states += fsms[b]->S1;
            h->max_P1 = std::max(h->max_P1, int(fsms[b]->P1));
            twins = twins && fsms[b]->log_twin != nullptr;
        }
        if (twins) {  // ... and the batch of the log twins for the fast entry (a repeated handle repeats its twin: stored once)
            std::vector<mm_fsm_t> tw(static_cast<size_t>(B));
            for (int64_t b = 0; b < B; ++b) tw[size_t(b)] = fsms[b]->log_twin;
            const int rc = batch_create_impl(tw.data(), B, &h->log_twin);
            if (rc) return rc;
        }
        *out = hold.release();
        return MM_OK;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->n_cus = cus;
    }
    // (the choice of kernels below reads them)
    int64_t nq_max[2] = {0, 0}, s1_max = 0;
    for (int64_t b = 0; b < B; ++b) {
        h->max_P1 = std::max(h->max_P1, int(fsms[b]->P1));
        h->max_S1p = std::max(h->max_S1p, fsms[b]->S1p);
        s1_max = std::max(s1_max, fsms[b]->S1);
        h->fast_ok = h->fast_ok && fsms[b]->fast_ok;
        for (int d = 0; d < 2; ++d) nq_max[d] = std::max(nq_max[d], fsms[b]->nquads[d]);
        h->max_depth = std::max(h->max_depth, fsms[b]->depth);
    }
    // quad kernels: one geometry (quads per lane, waves) per direction for the whole batch
    h->fast_ok = h->fast_ok && h->semiring == MM_LOG;
    if (h->fast_ok) {
        for (int d = 0; d < 2; ++d) {
            QuadGeometry geo = pick_quad_geometry(nq_max[d]);
            // (MM_KQ: a value without a kernel instance -- 4, 8, 12, 14, 16, ... -- is ignored, not left to fail at the launch)
            if (quad_kq_has_instance(h->dbg.kq)) geo.KQ = h->dbg.kq;
            // enough waves for the quads, and for at most two rows per thread where the workgroup can be that large
            geo.NW = int(std::min<int64_t>(geo.KQ > 13 ? 8 : MM_MAX_WAVES,
                                           std::max<int64_t>({1, (nq_max[d] + 64 * geo.KQ - 1) / (64 * geo.KQ),
                                                              (s1_max + 127) / 128})));
            if (h->dbg.nwaves >= 1 && h->dbg.nwaves <= (geo.KQ > 13 ? 8 : MM_MAX_WAVES)) geo.NW = h->dbg.nwaves;
            h->geo_kq[d] = geo.KQ;
            h->geo_nw[d] = geo.NW;
            h->max_quads[d] = int(nq_max[d]);
        }
        // small graphs keep the CSR the exact fallback walks in LDS (left-to-right graphs spread the
        // values of one frame over far more than the float range: most of their rows take that path)
        for (int64_t b = 0; b < B; ++b)
            h->max_xcsr = std::max<int64_t>(h->max_xcsr, fsms[b]->S1 + 1 + 2 * std::max(fsms[b]->qmat[0].rowptr[fsms[b]->S1],
                                                                                  fsms[b]->qmat[1].rowptr[fsms[b]->S1]));
        if (h->geo_kq[0] <= 3 && h->geo_kq[1] <= 3 && !h->dbg.no_xcsr) {
            h->xcsr = int((h->max_xcsr + 3) & ~int64_t(3));
            if (h->max_xcsr > 16 * 1024 || quad_lds_bytes(h, 0) > 128 * 1024 || quad_lds_bytes(h, 1) > 128 * 1024) h->xcsr = 0;
        }
    }
    bool rows = false;
    int rc = pick_family(h, fsms, nq_max, s1_max, &rows);
    if (rc) return rc;
    std::vector<UttDesc> utts(B);
    if (h->semiring == MM_TROPICAL && h->dbg.kernel != DebugOpts::K_ITEM) {
        h->vit_ok = true;
        for (int64_t b = 0; b < B && h->vit_ok; ++b) {
            bool ok = false;
            rc = vit_variant(fsms[b], h->dbg, &ok);
            if (rc) return rc;
            h->vit_ok = ok;
            if (ok) {  // (one layout per batch: the first FSM's; an FSM that needed another one keeps the batch on the item kernel)
                if (b == 0) {
                    h->vit_n4 = fsms[b]->vit_n4;
                    h->vit_n2 = fsms[b]->vit_n2;
                }
                h->vit_ok = fsms[b]->vit_n4 == h->vit_n4 && fsms[b]->vit_n2 == h->vit_n2;
                h->vit_arcs = std::max(h->vit_arcs, int(fsms[b]->vrow.form[0].g.col.size()));
                h->vit_ok = h->vit_ok && size_t(fsms[b]->S1p) * 4 <= 24576;  // (the kernel's state vectors: mm_vit_tu.hip)
            }
        }
    }
    // (the item forms -- the general fallback, the alpha / beta export, the total-sum family -- of a batch of the wave kernel go to
    // the device when an entry first needs them, ensure_item_forms(): a batch of new numerator graphs every training step
    // never does)
    h->items_resident = h->fb != Fb::Wave && !h->lane_redo_wave;
    for (int64_t b = 0; b < B; ++b) {
        mm_fsm_t f = fsms[b];
        rc = h->items_resident ? fsm_to_device(f) : MM_OK;
        QuadVariant *qv[2] = {nullptr, nullptr};
        for (int d = 0; d < 2 && !rc && h->quad_built; ++d) rc = quad_variant(f, d, h->geo_kq[d], h->dbg.verbose, &qv[d]);
        if (rc) return rc;
        UttDesc &u = utts[b];
        memset(&u, 0, sizeof(u));
        u.g[0] = f->gdev[0];
        u.g[1] = f->gdev[1];
        if (qv[0] && qv[1]) {
            u.q[0] = qv[0]->qdev;
            u.q[1] = qv[1]->qdev;
            u.init_f = qv[0]->d_init_f;
            u.map_bf = qv[1]->d_map_bf;
        }
        if (h->fb == Fb::Lane) u.lane = static_cast<const LaneDev *>(f->lane.form.get());
        if (h->fb == Fb::Stream) u.stream = mm_stream_dev(f->stream_h[stream_hidx(h->stream_H)].form.get());
        if (h->vit_ok) u.rv = f->vrow.form[0].rdev;
        if (h->fb == Fb::Wave || h->lane_redo_wave)
            for (int d = 0; d < 2; ++d) u.rw[d] = f->wrows.form[d].rdev;
        if (h->fb == Fb::Pairs)
            for (int d = 0; d < 2; ++d) u.rp[d] = f->prows.form[d].rdev;
        if (h->fb == Fb::Split)
            for (int d = 0; d < 2; ++d)
                for (int s = 0; s < h->pair_H; ++s) u.rps[d][s] = split_row(f, d, s).rdev;
        if (rows)
            for (int d = 0; d < 2; ++d) {
                u.r[d] = f->rows.form[d].rdev;
                h->row_ka[d] = std::max(h->row_ka[d], f->rows.form[d].g.KA);
                h->row_nwc[d] = std::max(h->row_nwc[d], f->rows.form[d].g.NWC);
                h->row_slotrows[d] = std::max(h->row_slotrows[d], f->rows.form[d].g.nslotrows);
            }
        u.init = f->d_init;
        u.s2p = f->d_s2p;
        u.pdf_ptr = f->d_pdf_ptr;
        u.pdf_rows = f->d_pdf_rows;
        u.S1 = int(f->S1);
        u.S1p = f->S1p;
        u.P1 = f->P1;
        u.pad = 0;
        u.state_off = h->total_states;
        u.s1p_prefix = h->total_s1p;
        h->total_states += f->S1;
        h->total_s1p += f->S1p;
        if (h->items_resident) h->max_items = std::max(h->max_items, int(std::max(f->packed[0].items.size(), f->packed[1].items.size())));
    }
    if (hipGetDevice(&h->device) != hipSuccess || hipMalloc(&h->d_utts, sizeof(UttDesc) * B) != hipSuccess ||
        hipMemcpy(h->d_utts, utts.data(), sizeof(UttDesc) * B, hipMemcpyHostToDevice) != hipSuccess) {
        return fail(MM_ERR_HIP, "mm_batch_create: device allocation failed");
    }
    h->utts_host = std::move(utts);
    // FSMs whose state vectors do not fit the LDS of some entry that keeps them in h->ws_big (every one but Cost and Entropy): the arc kernel's
    // plan is the largest, and the streamed-only instances of the arc and sampling entries have the vectors there whatever the
    // size (MM_NITEMS=0 on a small graph)
    bool big = false;
    for (ItemEntry e : {ItemEntry::Fb, ItemEntry::Export, ItemEntry::Tropical, ItemEntry::Arcs, ItemEntry::Sample}) big |= item_plan(h, e).global;
    if (big && hipMalloc(&h->ws_big, size_t(B) * 4 * size_t(h->max_S1p) * sizeof(float)) != hipSuccess) {
        h->ws_big = nullptr;
        return fail(MM_ERR_HIP, "mm_batch_create: device allocation failed");
    }
    if (on_pairs(h) && !h->dbg.no_dpair) {
        void *hp = nullptr;
        if (hipMalloc(&h->stat_dev, 4 * sizeof(int)) == hipSuccess && hipMemset(h->stat_dev, 0, 4 * sizeof(int)) == hipSuccess &&
            hipHostMalloc(&hp, 4 * sizeof(int), hipHostMallocMapped) == hipSuccess) {
            h->stat_host = static_cast<volatile int *>(hp);
            for (int k = 0; k < 4; ++k) h->stat_host[k] = 0;  // ([2], [3]: utterances the last alpha / beta export handed to the item kernel)
            h->dpair_ok = true;
            h->exact_first = h->dbg.exact_first;
            h->wpair_ok = !h->dbg.no_wpair && mm_wpair_fits(pair_launch_of(h));
        }
    }
    if (h->dbg.verbose)
        fprintf(stderr, "[mm] batch of %lld created in %.1f ms\n", (long long)B, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tb0).count());
    *out = hold.release();
    return MM_OK;
}

int mm_batch_create(const mm_fsm_t *fsms, int64_t B, mm_batch_t *out) {
    return no_throw("mm_batch_create", [&]() { return batch_create_impl(fsms, B, out); });
}

#ifdef MM_STAMPS
// diagnostic build: copy the per-wave phase cycle sums of the last pdfposteriors call to the host
int mm_debug_read_stamps(unsigned long long *out, int64_t n) {
    if (!g_dbg) return fail(MM_ERR_INVALID, "no stamps recorded");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, g_dbg, sizeof(unsigned long long) * size_t(std::min<int64_t>(n, int64_t(g_dbg_n))),
                      hipMemcpyDeviceToHost));
    return MM_OK;
}
#endif

int mm_batch_destroy(mm_batch_t h) {
    if (!h) return MM_OK;
    if (h->log_twin) (void)mm_batch_destroy(h->log_twin);
    if (h->prob_logv) (void)hipFree(h->prob_logv);
    if (h->d_utts) (void)hipFree(h->d_utts);
    if (h->ws_big) (void)hipFree(h->ws_big);
    if (h->ws) (void)hipFree(h->ws);
    if (h->stat_dev) (void)hipFree(h->stat_dev);
    if (h->stat_host) (void)hipHostFree(const_cast<int *>(h->stat_host));
    if (h->gen.ws) (void)hipFree(h->gen.ws);
    if (h->gen.d_utts) (void)hipFree(h->gen.d_utts);
    delete h;
    return MM_OK;
}

int64_t mm_batch_total_states(mm_batch_t h) { return h ? h->total_states : -1; }

}  // extern "C"
namespace mm {
FsmGenView *mm_fsm_gen_view(mm_fsm_t f) {
    if (!f) return nullptr;
    std::call_once(f->gen_once, [&]() { gen_build(f); });
    return &f->gen;
}
GenScratch *mm_batch_gen_scratch(mm_batch_t h) { return h ? &h->gen : nullptr; }
int mm_batch_gen_view(mm_batch_t h, int64_t *B, const mm_fsm_t **fsms, int *semiring, int *device) {
    if (!h) return MM_ERR_INVALID;
    *B = h->B;
    *fsms = h->fsms.data();
    *semiring = h->semiring;
    *device = h->device;
    return MM_OK;
}
}  // namespace mm
extern "C" {

int mm_batch_set_posterior_floor(mm_batch_t h, float floor) {
    h = twin_of(h);
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_set_posterior_floor: NULL batch");
    if (!(floor >= 1e-30f && floor <= 1e-6f)) return fail(MM_ERR_INVALID, "mm_batch_set_posterior_floor: floor outside [1e-30, 1e-6]");
    // a term that dropped out of the linear path would have had a posterior below 2^(-120 - L_n) (mm_pair_finish_kernel):
    // L_n >= -120 - log2(floor) keeps every loss below the floor (1e-30 -> -20.3, the default -20; 1e-12 -> -80)
    h->lt_floor = std::min(-20.f, -120.f - std::log2(floor));
    if (h->stat_host) h->stat_host[0] = 0;  // (what was hard under the old floor need not be under the new one: float32 kernels first)
    return MM_OK;
}

int mm_batch_set_exact_policy(mm_batch_t h, int policy) {
    h = twin_of(h);
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_set_exact_policy: NULL batch");
    if (policy != MM_EXACT_AUTO && policy != MM_EXACT_F32_FIRST && policy != MM_EXACT_F64_FIRST)
        return fail(MM_ERR_INVALID, "mm_batch_set_exact_policy: unknown policy");
    h->exact_first = policy == MM_EXACT_AUTO ? -1 : (policy == MM_EXACT_F64_FIRST ? 1 : 0);
    return MM_OK;
}

int mm_batch_set_gamma_mode(mm_batch_t h, int accumulate, float scale) {
    h = twin_of(h);
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_set_gamma_mode: NULL batch");
    if (!(scale == scale) || std::isinf(scale)) return fail(MM_ERR_INVALID, "mm_batch_set_gamma_mode: scale is not finite");
    const bool plain = !accumulate && scale == 1.f;
    // (every other kernel family may compute an utterance TWICE -- the linear-domain kernels first, the exact ones for what they
    // mark -- and the second result must replace the first, not add to it)
    if (!plain && h->fb != Fb::Wave)
        return fail(MM_ERR_UNSUPPORTED, "mm_batch_set_gamma_mode: only batches of the wave kernel (every graph <= 1023 states, <= 4096 arc slots per direction: "
                                        "LF-MMI numerators) scale or accumulate their posteriors");
    h->g_acc = accumulate != 0;
    h->g_scale = scale;
    return MM_OK;
}

int mm_batch_set_mark_policy(mm_batch_t h, int policy) {
    h = twin_of(h);
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_set_mark_policy: NULL batch");
    if (policy != MM_MARKS_DECIDE && policy != MM_MARKS_KEEP) return fail(MM_ERR_INVALID, "mm_batch_set_mark_policy: unknown policy");
    h->keep_marks = policy == MM_MARKS_KEEP;
    if (h->stat_host) h->stat_host[0] = 0;  // (what the last call counted was counted under the other policy: float32 kernels first)
    return MM_OK;
}

int mm_batch_set_deterministic(mm_batch_t h, int on) {
    h = twin_of(h);
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_set_deterministic: NULL batch");
    h->deterministic = on != 0;
    return MM_OK;
}

int mm_batch_last_redo_count(mm_batch_t h, void *stream, int64_t *n) {
    h = twin_of(h);
    if (!h || !n) return fail(MM_ERR_INVALID, "mm_batch_last_redo_count: bad argument");
    *n = 0;
    if (!h->last_redo) return MM_OK;
    std::vector<int> marks(size_t(h->B), 0);
    HIP_TRY(hipMemcpyAsync(marks.data(), h->last_redo, size_t(h->B) * sizeof(int), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int m : marks) *n += m != 0;
    if (h->dbg.verbose && h->last_z) {  // what mm_pair_finish_kernel decided on
        std::vector<double> z(size_t(h->B) * 6);
        HIP_TRY(hipMemcpy(z.data(), h->last_z, z.size() * 8, hipMemcpyDeviceToHost));
        double sp = 0, lm = 0;
        int worst_b = -1, below[5] = {0, 0, 0, 0, 0};
        const double thr[5] = {-8, -11, -14, -17, -20};
        for (int64_t b = 0; b < h->B; ++b) {
            const double zmin = std::min(z[6 * b], z[6 * b + 1]), zmax = std::max(z[6 * b + 2], z[6 * b + 3]);
            if (zmax - zmin > sp) sp = zmax - zmin, worst_b = int(b);
            const double l = std::min(z[6 * b + 4], z[6 * b + 5]);
            lm = std::min(lm, l);
            for (int k = 0; k < 5; ++k) below[k] += l < thr[k];
        }
        fprintf(stderr, "[mm] per-frame log2 normalisers: largest spread %.3g (utterance %d), smallest overlap term %.3g; utterances with an overlap term "
                        "below -8 / -11 / -14 / -17 / -20: %d / %d / %d / %d / %d of %lld\n", sp, worst_b, lm, below[0], below[1], below[2], below[3], below[4],
                (long long)h->B);
    }
    return MM_OK;
}

int mm_batch_last_fallback_count(mm_batch_t h, void *stream, int64_t *n) {
    h = twin_of(h);
    if (!h || !n) return fail(MM_ERR_INVALID, "mm_batch_last_fallback_count: bad argument");
    *n = 0;
    if (!h->last_redo2) return MM_OK;
    std::vector<int> marks(size_t(h->B), 0);
    HIP_TRY(hipMemcpyAsync(marks.data(), h->last_redo2, size_t(h->B) * sizeof(int), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int m : marks) *n += m != 0;
    return MM_OK;
}

int mm_batch_last_exact_first(mm_batch_t h) {
    h = twin_of(h);
    return h && h->last_exact_first ? 1 : 0;
}

int mm_batch_team_xcd_stats(mm_batch_t h, int out[2]) {
    h = twin_of(h);
    if (!h || !out) return fail(MM_ERR_INVALID, "mm_batch_team_xcd_stats: bad argument");
    out[0] = out[1] = 0;
    if (!h->stat_dev) return MM_OK;
    h->xcd_counting = true;  // (the calls from here on count; the first call returns the zeros nothing has been added to)
    return no_throw("mm_batch_team_xcd_stats", [&]() {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, h->stat_dev + 2, 2 * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(h->stat_dev + 2, 0, 2 * sizeof(int)));
        return int(MM_OK);
    });
}

// (mm_batch_kernels, entry 0) what mm_pdfposteriors_f32 launches on a log batch
// the item kernel by instance: <MODE, NI, where the state vectors live> (FB: <MODE_FB, NI, pass, where>)
static std::string item_fb_kernels(mm_batch_t h, bool one_launch) {
    const ItemPlan pl = item_plan(h, ItemEntry::Fb);
    const std::string w = where_of(pl.global);
    if (one_launch || pl.NI == 0)  // (redo_on_items always, launch_log without resident items)
        return "mm_log_kernel<MODE_FB,0,0," + w + "> (forward and backward in one launch, every item streamed)";
    return "mm_log_kernel<MODE_FB,8,1," + w + "> (forward) + mm_log_kernel<MODE_FB,8,2," + w + "> (backward)";
}
static std::string item_export_kernel(mm_batch_t h, const char *mode, bool trop) {
    const ItemPlan pl = item_plan(h, ItemEntry::Export);
    return std::string("mm_log_kernel<") + mode + "," + std::to_string(pl.NI) + "," + where_of(pl.global) + (trop ? ",TROP>" : ">");
}
static std::string tropical_kernel(mm_batch_t h) {  // (launch_tropical)
    const ItemPlan pl = item_plan(h, ItemEntry::Tropical);
    return "mm_tropical_kernel<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
}

// the wave kernel's instance (wave_launch_of): a wave batch's kernel, and what a lane batch with wave forms runs for its marked utterances
static std::string wave_instance(mm_batch_t h) {
    return "mm_wave_kernel<" + std::to_string(h->wave_nseg <= 2 ? 2 : 4) + "," + std::to_string(h->max_P1 <= 128 ? 2 : 4) +
        (h->wave_nseg <= 2 && h->B > h->n_cus ? ",two per CU>" : ">");
}

static std::string fb_kernels(mm_batch_t h) {
    // what fb_exact runs, and (`redo`) what the families that hand their marked utterances to redo_on_items run
    auto quad_instance = [&](int d) {  // (RPT as launch_quad_kq of mm_quad_tu.hip derives it)
        const int NT = 64 * h->geo_nw[d], rpt = (h->max_S1p + NT - 1) / NT <= 2 ? 2 : 3;
        return "mm_fbq_kernel<" + std::to_string(h->geo_kq[d]) + "," + std::to_string(rpt) + "," + std::to_string(d) + "> x " +
            std::to_string(h->geo_nw[d]) + " waves";
    };
    // (which body of the exact fallback: the CSR it walks is staged in LDS for KQ <= 3 where it fits, see mm_batch_create)
    const std::string quad = quad_instance(0) + " + " + quad_instance(1) + (h->xcsr > 0 ? " (fallback CSR in LDS)" : " (fallback CSR in global memory)");
    const std::string exact = h->quad_ok ? quad : item_fb_kernels(h, false);
    const std::string redo = item_fb_kernels(h, true);
    const std::string pair_tail = h->dpair_ok && !h->quad_ok ? redo : exact;
    switch (h->fb) {
    case Fb::Lane:
        return "mm_lane_kernel<" + std::to_string(h->lane_S <= 8 ? 8 : h->lane_S <= 16 ? 16 : h->lane_S <= 32 ? 32 : 64) +
            "> (one wave per utterance and direction, the graph in its registers, float64), then for marked utterances only " +
            (h->lane_redo_wave ? wave_instance(h) : redo);
    case Fb::Wave:
        return wave_instance(h);
    case Fb::Stream:
        return "mm_stream_kernel<" + std::to_string(mm_stream_nj(h->max_P1)) + "," + std::to_string(h->stream_H) + "> (forward and backward recursions as workgroups of one grid" +
            (h->stream_H > 1 ? ", teams of " + std::to_string(h->stream_H) + " workgroups per utterance and direction" : std::string()) +
            "; arcs streamed from L2, the vector in LDS as wide-exponent "
            "32-bit values), mm_stream_combine_kernel, mm_stream_finish_kernel, then for marked utterances only " + redo;
    case Fb::Split: {
        const std::string k = std::to_string(mm_pair_nj(h->max_P1, h->pair_H)), H = std::to_string(h->pair_H);
        return "mm_fbs_kernel<" + k + ",A," + H + ">, then <" + k + ",B," + H + "> (forward and backward agents in one grid, teams of " + H +
            " workgroups), mm_pair_finish_kernel, then for marked utterances only " +
            (h->dpair_ok ? "mm_fbds_kernel<" + k + ",A," + H + ">, then <" + k + ",B," + H + "> (float64, one utterance per team" +
                               (h->wpair_ok ? std::string("); FIRST and alone while the inputs are hard: mm_fbws_kernel<") + k + ",A," + H + ">, then <" + k +
                                                  ",B," + H + "> (wide-exponent pairs, two utterances per team)"
                                            : std::string("; FIRST and alone while the inputs are hard)")) +
                               ", mm_dpair_finish_kernel, then for what those mark "
                         : std::string()) +
            pair_tail;
    }
    case Fb::Pairs: {
        const std::string k = std::to_string(mm_pair_nj(h->max_P1));
        const std::string small = pair_small_instances(pair_launch_of(h)) ? ", the instances for graphs of up to 127 states" : "";
        return "mm_fbp_kernel<" + k + ",A>, then <" + k + ",B> (forward and backward agents in one grid" + small + "), mm_pair_finish_kernel, then for marked "
            "utterances only " +
            (h->dpair_ok ? "mm_fbd_kernel<" + k + ",A>, then <" + k + ",B> (float64, one utterance per workgroup" +
                               (h->wpair_ok ? std::string("); FIRST and alone while the inputs are hard: mm_fbw_kernel<") + k + ",A>, then <" + k +
                                                  ",B> (wide-exponent pairs, two utterances per workgroup)"
                                            : std::string("; FIRST and alone while the inputs are hard)")) +
                               ", mm_dpair_finish_kernel, then for what those mark "
                         : std::string()) +
            pair_tail;
    }
    case Fb::Rows: {
        auto ka = [&](int d) {
            for (int k : kRowKA)
                if (h->row_ka[d] <= k) return k;
            return 0;
        };
        return "mm_fbr_kernel<" + std::to_string(ka(0)) + ",8192,0> + mm_fbr_kernel<" + std::to_string(ka(1)) +
            ",8192,1>, then for marked utterances only " + exact;
    }
    case Fb::Quad:
    case Fb::Item:
        break;
    }
    return exact;
}

static bool export_on_pairs(mm_batch_t h, int dir);
// what mm_launch_viterbi is told about a batch whose FSMs all have the Viterbi form (h->vit_ok)
static VitLaunch vit_launch_of(mm_batch_t h) {
    VitLaunch vl;
    vl.B = h->B;
    vl.n4 = h->vit_n4;
    vl.n2 = h->vit_n2;
    vl.max_P1 = h->max_P1;
    vl.max_S1p = h->max_S1p;
    vl.max_arcs = h->vit_arcs;
    vl.bp_row = int((size_t(h->max_S1p) + 255) & ~size_t(255));  // bytes of a row of one-byte back-pointers, padded to 256
    return vl;
}
// "; class sums on 8, 64 lanes": the distinct widths of the class pass over the utterances of the current class plan
static std::string class_lanes_text(mm_batch_t h) {
    std::string s;
    for (int lgl = 0; lgl < 32; ++lgl)
        if (h->cls_lgl_mask >> lgl & 1u) s += (s.empty() ? "" : ", ") + std::to_string(1 << lgl);
    return "; class sums on " + s + " lanes";
}
int mm_batch_kernels(mm_batch_t h, int entry, char *buf, size_t n) {
    if (!h || !buf || n < 2) return fail(MM_ERR_INVALID, "mm_batch_kernels: bad argument");
    if (entry == 0) h = twin_of(h);  // (ProbSemiring: the fast entry runs the log twins' kernels)
    if (entry == 0 && h->semiring == MM_PROB)
        return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: this ProbSemiring batch has no log twins (Float64 FSMs, or negative weights): mm_pdfposteriors_ex only");
    std::string s;
    if (entry == 0) {  // mm_pdfposteriors_f32
        s = fb_kernels(h);
    } else if (entry == 1) {  // mm_viterbi_f32
        const std::string t = tropical_kernel(h);
        s = t + " + mm_backtrace_kernel";
        if (h->vit_ok) {  // (the instance and the back-trace's plan: what mm_launch_viterbi launches, mm_vit_plan)
            VitPlan pl;
            const int rc = mm_vit_plan(vit_launch_of(h), &pl);
            if (rc) return rc;
            s = "mm_vit_kernel<" + std::to_string(h->vit_n4) + "," + std::to_string(h->vit_n2) + "," + std::to_string(pl.nj) + "> + mm_vit_backtrace_kernel<csr in " +
                (pl.csrl ? "LDS" : "global memory") + ", R=" + std::to_string(pl.R) + "> with " + std::to_string(pl.lds) + " bytes of LDS (" + t +
                " + mm_backtrace_kernel when the int32 back-pointers are asked for)";
        }
    } else if (entry == 3) {  // mm_alpharecursion_f32 / mm_betarecursion_f32
        const bool xa = export_on_pairs(h, 0), xb = export_on_pairs(h, 1);
        const std::string fast = (h->pair_H > 1 ? "mm_fbsx_kernel<2," + std::to_string(h->pair_H) + "> (phase A of one direction over all frames, teams of " + std::to_string(h->pair_H) + " workgroups) + "
                                                : "mm_fbx_kernel<" + std::to_string(mm_pair_nj(h->max_P1)) + "> (phase A of one direction over all frames, two utterances per workgroup) + ") +
                                 "mm_pair_export_kernel, then for marked utterances only the item kernel, ";
        const std::string ia = item_export_kernel(h, "MODE_ALPHA", false), ib = item_export_kernel(h, "MODE_BETA", false);
        s = h->semiring == MM_TROPICAL ? tropical_kernel(h) + " / " + item_export_kernel(h, "MODE_BETA", true)
            : "alpha: " + (xa ? fast + ia : ia) + "; beta: " + (xb ? fast + ib : ib);
    } else if (entry >= 4 && entry <= 6) {  // mm_arcposteriors_f32, mm_samplepaths_f32, mm_expectedcost_f32
        static const char *const who[] = {"mm_arcposteriors_f32", "mm_samplepaths_f32", "mm_expectedcost_f32"};
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, std::string("mm_batch_kernels: ") + who[entry - 4] + " runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, entry == 4 ? ItemEntry::Arcs : entry == 5 ? ItemEntry::Sample : ItemEntry::Cost);
        const std::string ni = std::to_string(pl.NI), vectors = pl.global ? "in global memory" : "in LDS";
        if (entry == 4) {
            s = "mm_log_kernel<MODE_FB," + ni + ",1> (forward) + mm_arc_kernel<" + ni +
                "> (backward, the arcs' sums by their owning lanes) + mm_arc_scatter_kernel; state vectors " + vectors;
        } else if (entry == 5) {
            s = "mm_log_kernel<MODE_FB," + ni + ",1> (forward) + mm_sample_kernel<" + where_of(!pl.stage) +
                "> (backward sampling, one wave per chain; alpha~ rows " + (pl.stage ? "staged in LDS by DMA" : "gathered from global memory") + ")";
        } else {
            const std::string inst = "<" + ni + "," + where_of(pl.global) + ">";
            s = "mm_cost_fwd_kernel" + inst + " (forward: alpha~ and r) + mm_cost_bwd_kernel" + inst + " (backward: beta~ and s, gamma and grad per pdf); state vectors " + vectors;
        }
    } else if (entry == 7) {  // mm_leakyposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_leakyposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Leaky);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        s = "mm_leaky_fwd_kernel" + inst + " (forward: alpha~ with the leak term in the row epilogue) + mm_leaky_bwd_kernel" + inst +
            " (backward: z, then beta = z (+) eps c, gamma per pdf); state vectors " + (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 8) {  // mm_pathentropy_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_pathentropy_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Entropy);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        s = "mm_entropy_fwd_kernel" + inst + " (forward: alpha~ and Hf, entropy and ttl; alone and without a store when neither grad nor gamma is asked for) + mm_entropy_bwd_kernel" +
            inst + " (backward: beta~ and Hb, gamma and grad per pdf); state vectors " + (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 9) {  // mm_filterposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_filterposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Filter);
        s = "mm_filter_kernel<" + std::to_string(pl.NI) + "," + where_of(pl.global) +
            "> (forward alone: filt and incr per frame from the finished vector, state_out and ttl; no frame kept); state vectors " +
            (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 10) {  // mm_windowposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_windowposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Window);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        s = "mm_window_fwd_kernel" + inst + " (forward from the carried start vector: alpha~ stored, state_out and lcommit at the commit frame) + mm_window_bwd_kernel" +
            inst + " (backward from an open or a closed end: gamma per pdf, ttl); state vectors " + (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 11) {  // mm_viterbiwindow_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_viterbiwindow_f32 runs on tropical batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::VitWindow);
        s = "mm_vitwindow_fwd_kernel<" + std::to_string(pl.NI) + "," + where_of(pl.global) +
            "> (tropical forward from the carried start vector: back-pointer rows, pre-emission maxima and the frames' maxima stored) + "
            "mm_vitwindow_trace_kernel<" + where_of(mm_vitwindow_flags_global(h->max_S1p)) +
            "> (best path, surviving sets back to the convergence point, state_out and mcommit at the commit frame); state vectors " +
            (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 12) {  // mm_weightedposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_weightedposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Weighted);
        const std::string ni = std::to_string(pl.NI);
        s = "mm_weights_kernel (the call's weight planes, init vectors and descriptors; not launched when W and W_init are NULL) + mm_log_kernel<MODE_FB," + ni +
            ",1> (forward, on the call's descriptors) + mm_weighted_bwd_kernel<" + ni + "," + where_of(pl.global) +
            "> (backward: the arcs' sums by their owning lanes, gamma per pdf) + mm_weighted_scatter_kernel; state vectors " + (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 13) {  // mm_segmentposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_segmentposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Segment);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        s = "mm_window_fwd_kernel" + inst + " (forward from the carried start vector: alpha~ stored) + mm_segment_bwd_kernel" + inst +
            " (backward from an open, a closed or a carried end: gamma per pdf, ttl, then the item pass behind frame 1: end_out and lend); state vectors " +
            (pl.global ? "in global memory" : "in LDS");
    } else if (entry == 14) {  // mm_arcclassposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_arcclassposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::ArcClass);
        const std::string ni = std::to_string(pl.NI);
        s = "mm_log_kernel<MODE_FB," + ni + ",1> (forward) + mm_arcclass_kernel<" + ni + "," + where_of(pl.global) +
            "> (backward: the classified arcs' terms by rank, a row of class sums per frame); state vectors " + (pl.global ? "in global memory" : "in LDS") +
            (h->cls_image.empty() ? "; no classes set"
                                  : class_lanes_text(h) + (h->cls_max_M > arcclass_cap(pl) ? "; terms in global memory" : "; terms in LDS"));
    } else if (entry == 15) {  // mm_scoredposteriors_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_scoredposteriors_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Scored);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        const int64_t cap = scored_class_cap(pl);
        s = "mm_scored_fwd_kernel" + inst + " (forward: every arc scored by its class's entry of the frame's score row) + mm_scored_bwd_kernel" + inst +
            " (backward: the scored beta~ recursion, the classified arcs' terms by rank, a row of class sums per frame, gamma per pdf); state vectors " +
            (pl.global ? "in global memory" : "in LDS") + "; class cap " + std::to_string(cap);
        if (h->cls_image.empty()) s += "; no classes set";
        else if (h->cls_C > cap) s += "; " + std::to_string(h->cls_C) + " classes exceed the cap";
        else
            s += "; term cap " + std::to_string(scored_term_cap(pl, h->cls_C)) + class_lanes_text(h) +
                 (h->cls_max_M > scored_term_cap(pl, h->cls_C) ? "; terms in global memory" : "; terms in LDS");
    } else if (entry == 16) {  // mm_classcost_f32
        if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_classcost_f32 runs on log-semiring batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::ClassCost);
        const std::string inst = "<" + std::to_string(pl.NI) + "," + where_of(pl.global) + ">";
        const int64_t cap = classcost_class_cap(pl);
        s = "mm_classcost_fwd_kernel" + inst + " (forward: alpha~ and r, every arc with its class's entry of the transition's cost row) + mm_classcost_bwd_kernel" +
            inst + " (backward: beta~ and s with the class costs, gamma and grad per pdf); state vectors " + (pl.global ? "in global memory" : "in LDS") +
            "; class cap " + std::to_string(cap);
        if (h->cls_image.empty()) s += "; no classes set";
        else if (h->cls_C > cap) s += "; " + std::to_string(h->cls_C) + " classes exceed the cap";
    } else if (entry == 17) {  // mm_classpath_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_classpath_f32 runs on tropical batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::ClassPath);
        const int64_t cap = classpath_class_cap(pl);
        s = "mm_classpath_fwd_kernel<" + std::to_string(pl.NI) + "," + where_of(pl.global) +
            "> (tropical forward: every arc scored by its class's entry of the transition's score row, back-pointer and class rows stored) + "
            "mm_classpath_trace_kernel (path and classes by one lane per utterance); state vectors " +
            (pl.global ? "in global memory" : "in LDS") + "; class cap " + std::to_string(cap);
        if (h->sc_image.empty()) s += "; no classes set";
        else if (h->cls_C > cap) s += "; " + std::to_string(h->cls_C) + " classes exceed the cap";
    } else if (entry == 18) {  // mm_lattice_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_lattice_f32 runs on tropical batches only");
        const ItemPlan pl = item_plan(h, ItemEntry::Lattice);
        const std::string where = where_of(lattice_global(h));
        s = "mm_tropical_kernel<" + std::to_string(pl.NI) + "," + where_of(pl.global) + "> (alpha) + " + item_export_kernel(h, "MODE_BETA", true) +
            " (beta) + mm_pick_final_kernel + mm_lattice_prune_kernel<" + where + ",count> (one workgroup per utterance and transition: the through-score of "
            "every stored arc against the beam) + mm_lattice_scan_kernel (offsets and total) + mm_lattice_prune_kernel<" + where +
            ",write> (the kept arcs in entry order); the two rows of a transition " + (lattice_global(h) ? "gathered from global memory" : "in LDS");
    } else if (entry == 19) {  // mm_latticeposteriors_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_latticeposteriors_f32 runs on tropical batches only");
        s = "mm_latpost_fb_kernel<" + std::to_string(latpost_nt(h)) + "> (one workgroup per utterance, serial over the transitions: the forward-backward over "
            "the records of each cell, state vectors in LDS, integer max and 64-bit fixed-point sums) + mm_latpost_gamma_kernel<" +
            std::to_string(MM_LATPOST_GAMMA_NT) + "> (one workgroup per utterance and frame, when gamma is asked for); state cap " + std::to_string(latpost_state_cap());
        if (mm_latpost_lds_bytes(h->max_S1p) > MM_LDS_MAX) s += "; " + std::to_string(h->max_S1p) + " states exceed the cap";
    } else if (entry == 20) {  // mm_latticecost_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_latticecost_f32 runs on tropical batches only");
        s = "mm_latcost_fb_kernel<" + std::to_string(latpost_nt(h)) + "> (one workgroup per utterance, serial over the transitions: mm_latpost_fb_kernel's "
            "forward-backward with the cost recursions beside it, signed 64-bit fixed-point cost sums, " + std::to_string(mm_latcost_lds_bytes(1) - mm_latcost_lds_bytes(0)) +
            " bytes of LDS per state) + mm_latcost_grad_kernel<" + std::to_string(MM_LATPOST_GAMMA_NT) +
            "> (one workgroup per utterance and frame, when grad or gamma is asked for); state cap " + std::to_string(latcost_state_cap());
        if (mm_latcost_lds_bytes(h->max_S1p) > MM_LDS_MAX) s += "; " + std::to_string(h->max_S1p) + " states exceed the cap";
    } else if (entry == 21) {  // mm_latticebest_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_latticebest_f32 runs on tropical batches only");
        s = "mm_latbest_kernel<" + std::to_string(latpost_nt(h)) + "> (one workgroup per utterance, serial over the transitions: the tropical forward-backward "
            "over the records of each cell in one pass and one barrier per step, three rotating state vectors in LDS, integer max, the best path traced in the "
            "backward loop, " + std::to_string(mm_latbest_lds_bytes(1) - mm_latbest_lds_bytes(0)) + " bytes of LDS per state); state cap " + std::to_string(latbest_state_cap());
        if (mm_latbest_lds_bytes(h->max_S1p) > MM_LDS_MAX) s += "; " + std::to_string(h->max_S1p) + " states exceed the cap";
    } else if (entry == 22) {  // mm_latticesample_f32
        if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_kernels: mm_latticesample_f32 runs on tropical batches only");
        s = "mm_latsample_fwd_kernel<" + std::to_string(latpost_nt(h)) + "> (mm_latpost_fb_kernel's forward pass alone: every record's forward value) + "
            "mm_latsample_kernel<" + std::to_string(latpost_nt(h)) + "> (one workgroup per utterance and " + std::to_string(MM_LS_CHUNK) +
            " samples, serial over the transitions backwards: a Gumbel-max draw among the records into each sample's state, a 64-bit occupancy mask per state "
            "and 64-bit integer max in LDS); state cap " + std::to_string(latsample_state_cap());
        if (mm_latsample_lds_bytes(h->max_S1p) > MM_LDS_MAX) s += "; " + std::to_string(h->max_S1p) + " states exceed the cap";
    } else if (entry == 2) {  // mm_pdfposteriors_ex: what its last call on this batch launched
        s = h->gen.last_kernels.empty() ? std::string("mm_generic_kernel (not called yet)") : h->gen.last_kernels;
    } else {
        return fail(MM_ERR_INVALID, "mm_batch_kernels: unknown entry");
    }
    snprintf(buf, n, "%s", s.c_str());
    return MM_OK;
}

static size_t ws_c_bytes(mm_batch_t h, int64_t N) { return align_up(size_t(h->B + 1) * size_t(N + 2) * 8, 256); }

// Where mm_pdfposteriors_f32 and the alpha / beta export keep what they keep in h->ws for N frames: byte offsets, in this order,
// each aligned to 256 bytes.  The stored vectors, the per-frame offsets; longest-first order, redo marks, pair hand-over, the
// per-utterance log Z minima; (split kernels) the float32 teams' exchange area, x_rows bytes of rows then per-pdf partial sums,
// and the float64 teams'; the marks the float64 kernels leave for the log-domain kernels (redo2); the extra region: (quad kernels)
// the emissions shifted by their per-frame maxima [B][N][P], the maxima [B][N] at em_max, or (stream kernels) their area, its
// parts at stream[].
struct WsLayout {
    size_t alpha = 0, c = 0, order = 0, redo = 0, hand = 0, zmin = 0, x = 0, x_rows = 0, xd = 0, xd_rows = 0, redo2 = 0;
    size_t extra = 0, em_max = 0, stream[4] = {0, 0, 0, 0}, total = 0;
};

static WsLayout ws_layout(mm_batch_t h, int64_t N) {
    WsLayout L;
    const size_t B = size_t(h->B), marks = align_up((B + 1) * 4, 256);
    // (the pair kernels keep N + 2 vectors per utterance and one workspace slot more than utterances; + 16 KB: the service waves copy
    // whole LDS regions of a stored row without clamping, dma_row_b128)
    L.c = on_pairs(h) ? align_up((B + 1) * size_t(h->pair_H > 1 ? h->split_s1p : h->max_S1p) * size_t(N + 2) * 4 + 16384, 256)
                      : align_up(size_t(h->total_s1p) * size_t(N + 1) * 4, 256);
    L.order = L.c + ws_c_bytes(h, N);
    L.redo = L.order + marks;
    L.hand = L.redo + marks;
    L.zmin = L.hand + align_up((B + 1) * 2 * mm_pair_hand_bytes(), 256);
    L.x = L.zmin + align_up(B * 6 * 8, 256);
    L.xd = L.redo2 = L.x;
    if (h->pair_H > 1) {
        // what the workgroups of a team send each other: [2 phases][pairs][2 directions][H sets][2 slots][2 * split_s1p] floats of
        // rows, then [pairs][2][H][4 slots][mm_pair_xps] floats of per-pdf partial sums; zeroed before every call
        const size_t H = size_t(h->pair_H), row = 2 * size_t(h->split_s1p) * 4, xps = size_t(mm_pair_xps(h->max_P1, h->pair_H)) * 4;
        L.x_rows = 2 * ((B + 1) / 2) * 2 * H * 2 * row;
        L.xd = L.redo2 = L.x + align_up(L.x_rows + ((B + 1) / 2) * 2 * H * 4 * xps, 256);
        // ... and for the teams of the float64 kernels (one utterance per team: B "pairs"; + 64 KB: the wide pair teams lay their
        // slots of per-pdf sums -- two doubles per pdf, 16 bytes more per slot for 128 pdfs -- over the same area, (B + 1) / 2 teams
        // instead of B)
        if (h->dpair_ok) {
            L.xd_rows = 2 * B * 2 * H * 2 * row;
            L.redo2 = L.xd + align_up(L.xd_rows + B * 2 * H * 4 * xps + 65536, 256);
        }
    }
    L.extra = L.redo2 + marks;
    L.total = L.extra;
    if (h->fb == Fb::Stream) {  // (the backward direction's vectors and offsets, the frames' log Z, the teams' exchange area)
        L.total += mm_stream_extra_bytes(h->B, h->total_s1p, N, L.stream, h->stream_H, h->stream_S1);
        for (size_t &o : L.stream) o += L.extra;
    } else if (h->quad_built) {
        L.em_max = L.extra + align_up(B * size_t(N) * size_t(h->max_P1 - 1) * 4, 256);
        L.total = L.em_max + align_up(B * size_t(N) * 4, 256);
    }
    return L;
}

// Where mm_viterbiwindow_f32 keeps what it keeps in h->ws for N frames (tropical batches): the int32 back-pointer rows, the float32
// rows of pre-emission maxima (both (sum_b S1p_b) x (N + 1)), the frames' maxima [B][N + 2] floats and the end states [B] ints
struct VitWindowWs { size_t best = 0, m = 0, end = 0, total = 0; };
static VitWindowWs vitwindow_ws_layout(mm_batch_t h, int64_t N) {
    VitWindowWs W;
    W.best = align_up(size_t(h->total_s1p) * size_t(N + 1) * 4, 256);
    W.m = 2 * W.best;
    W.end = W.m + align_up(size_t(h->B) * size_t(N + 2) * 4, 256);
    W.total = W.end + align_up(size_t(h->B) * 4, 256);
    return W;
}

// Where mm_classpath_f32 keeps what it keeps in h->ws for N frames (tropical batches): the int32 back-pointer rows and the 16-bit class
// rows (both (sum_b S1p_b) x (N + 1)) and, for a plan with global vectors, the two class rows of every utterance's current frames
struct ClassPathWs { size_t bc = 0, cbuf = 0, total = 0; };
static ClassPathWs classpath_ws_layout(mm_batch_t h, int64_t N, bool global) {
    ClassPathWs W;
    W.bc = align_up(size_t(h->total_s1p) * size_t(N + 1) * 4, 256);
    W.cbuf = W.bc + align_up(size_t(h->total_s1p) * size_t(N + 1) * 2, 256);
    W.total = W.cbuf + (global ? align_up(size_t(h->B) * 2 * size_t(h->max_S1p) * 2, 256) : 0);
    return W;
}

size_t mm_batch_workspace_bytes(mm_batch_t h, int64_t N) {
    if (!h || N < 0) return 0;
    if (h->log_twin) return mm_batch_workspace_bytes(h->log_twin, N) + align_up(size_t(h->B) * size_t(N) * size_t(h->max_P1 - 1) * 4, 256);
    const size_t total = ws_layout(h, N).total;
    return h->semiring == MM_TROPICAL ? std::max(total, vitwindow_ws_layout(h, N).total) : total;
}


// Viterbi on the row-lane form (mm_kernel_vit.hip): one-byte back-pointers [B][N + 1][row], rows padded to 256 bytes, + the
// KB the back-trace's last DMA may read past the end
static size_t vit_bp_row(mm_batch_t h) { return size_t(vit_launch_of(h).bp_row); }
static size_t ws_vit_bytes(mm_batch_t h, int64_t N) {
    if (h->semiring != MM_TROPICAL) return 0;
    return h->vit_ok ? size_t(h->B) * size_t(N + 1) * vit_bp_row(h) + 1024 : align_up(size_t(h->total_states) * size_t(N + 1) * 4, 256);
}

static int ensure_ws(mm_batch_t h, size_t bytes, void *stream = nullptr) {
    if (h->ws_bytes >= bytes) return MM_OK;
    // growing frees the old workspace: never while the caller's stream is capturing (a graph captured earlier on this
    // batch has the old pointers baked in; mm_batch_reserve is the way to size it up front)
    if (capturing(stream)) return fail(MM_ERR_INVALID, "the workspace would have to grow during stream capture: call mm_batch_reserve first");
    if (h->ws) {
        HIP_TRY(hipFree(h->ws));  // synchronises: only on growth
        h->ws = nullptr;
        h->ws_bytes = 0;
        h->last_redo = nullptr;
        h->last_z = nullptr;
    }
    HIP_TRY(hipMalloc(&h->ws, bytes));
    h->ws_bytes = bytes;
    return MM_OK;
}

// (ProbSemiring batches) room for the logarithms of a call's likelihoods [B][N][P]; grown like the workspace: never during a capture
static int ensure_prob_logv(mm_batch_t h, int64_t N, void *stream) {
    const size_t bytes = align_up(size_t(h->B) * size_t(N) * size_t(h->max_P1 - 1) * 4, 256);
    if (h->prob_logv_bytes >= bytes) return MM_OK;
    if (capturing(stream)) return fail(MM_ERR_INVALID, "the workspace would have to grow during stream capture: call mm_batch_reserve first");
    if (h->prob_logv) {
        HIP_TRY(hipFree(h->prob_logv));
        h->prob_logv = nullptr;
        h->prob_logv_bytes = 0;
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->prob_logv), bytes));
    h->prob_logv_bytes = bytes;
    return MM_OK;
}

int mm_batch_reserve(mm_batch_t h, int64_t N) {
    if (!h || N < 1) return fail(MM_ERR_INVALID, "mm_batch_reserve: bad argument");
    if (h->log_twin) {
        const int rc = ensure_prob_logv(h, N, nullptr);
        return rc ? rc : mm_batch_reserve(h->log_twin, N);
    }
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return fail(MM_ERR_INVALID, "mm_batch_reserve: batch lives on another device");
    // (the total-sum rows and the max-marginals share the workspace: [N + 1][total states] words; the Viterbi back-pointers:
    // one-byte rows for the row-lane kernels, int32 rows for the item kernel)
    return ensure_ws(h, std::max({mm_batch_workspace_bytes(h, N), align_up(size_t(h->total_states) * size_t(N + 1) * 4, 256), ws_vit_bytes(h, N)}));
}

static int check_run(mm_batch_t h, const char *who, const float *V, int64_t N, int want_semiring) {
    if (!h) return fail(MM_ERR_INVALID, std::string(who) + ": NULL batch");
    if (!V) return fail(MM_ERR_INVALID, std::string(who) + ": V is NULL");
    if (N < 1 || N > (int64_t(1) << 30)) return fail(MM_ERR_DIM, std::string(who) + ": need N >= 1");
    if (want_semiring >= 0 && h->semiring != want_semiring)
        return fail(MM_ERR_INVALID, std::string(who) + ": batch was built for another semiring");
    if (h->semiring == MM_PROB)
        return fail(MM_ERR_UNSUPPORTED, std::string(who) + ": ProbSemiring batches run through mm_pdfposteriors_f32 (Float32 FSMs) or mm_pdfposteriors_ex");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return fail(MM_ERR_INVALID, std::string(who) + ": batch lives on another device");
    // (every run entry reuses the workspace the redo marks of the last pdfposteriors call live in: mm_batch_last_redo_count
    // must not read what another entry wrote there)
    h->last_redo = nullptr;
    h->last_redo2 = nullptr;
    h->last_z = nullptr;
    return MM_OK;
}

// ProbSemiring batches on the fast kernels: V holds LIKELIHOODS (values of the semiring, as the reference's Array{ProbSemiring} does);
// one pass takes their logarithms, the log twins' kernels do the work, ttl comes back as the probability exp(log Z) -- gamma is a
// probability in both semirings (src/inference.jl:158-160: the quotient, and exp() of it for the log-like semirings only)
static __global__ void mm_prob_log_kernel(const float *V, long long vsb, long long vsn, int N, int P, float *out) {
    const long long row = (long long)blockIdx.x;  // (b, n)
    const float *src = V + (row / N) * vsb + (row % N) * vsn;
    float *dst = out + row * P;
    for (int q = threadIdx.x; q < P; q += blockDim.x) dst[q] = logf(src[q]);  // (log 0 = -inf = zero(LogSemiring))
}
static __global__ void mm_prob_exp_kernel(float *ttl, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) ttl[b] = expf(ttl[b]);
}
static int prob_pdfposteriors(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, float *gamma,
                              int64_t gsb, int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    if (!V || !gamma || !ttl) return fail(MM_ERR_INVALID, "mm_pdfposteriors_f32: V / gamma / ttl is NULL");
    if (N < 1 || N > (int64_t(1) << 30)) return fail(MM_ERR_DIM, "mm_pdfposteriors_f32: need N >= 1");
    if (!h->log_twin)
        return fail(MM_ERR_UNSUPPORTED, "mm_pdfposteriors_f32: this ProbSemiring batch has no log twins (Float64 FSMs, or negative weights): mm_pdfposteriors_ex");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return fail(MM_ERR_INVALID, "mm_pdfposteriors_f32: batch lives on another device");
    int rc = ensure_prob_logv(h, N, stream);
    if (rc) return rc;
    const int P = h->max_P1 - 1;
    hipLaunchKernelGGL(mm_prob_log_kernel, dim3(unsigned(h->B * N)), dim3(P <= 64 ? 64 : (P <= 128 ? 128 : 256)), 0, static_cast<hipStream_t>(stream), V,
                       (long long)vsb, (long long)vsn, int(N), P, h->prob_logv);
    HIP_TRY(hipGetLastError());
    rc = mm_pdfposteriors_f32(h->log_twin, h->prob_logv, int64_t(N) * P, P, lens, N, gamma, gsb, gsn, gsp, ttl, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(mm_prob_exp_kernel, dim3(unsigned((h->B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), ttl, int(h->B));
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

// ---- mm_pdfposteriors_f32, one function per kernel family (h->fb): p holds the call, its marks set by the prologue

// the item kernel for what the kernels before it marked (p.redo), both passes in ONE launch whose workgroups of the other utterances
// leave at once (streamed items: its speed does not matter, the empty launch's does)
static int redo_on_items(mm_batch_t h, const RunParams &p, void *stream) {
    return launch(mm_log_kernel<MODE_FB, 0, 0, false, false>, mm_log_kernel<MODE_FB, 0, 0, false, true>, h, p, ItemEntry::Fb, item_plan(h, ItemEntry::Fb).NW, stream);
}

// the library's own zeroing kernel over `bytes` (a multiple of 16) at d
static int zero_dev(void *d, size_t bytes, void *stream) {
    const size_t zn = bytes / 16;
    hipLaunchKernelGGL(mm_zero_kernel, dim3(unsigned(std::min<size_t>(2048, (zn + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<char *>(d), (unsigned long long)zn);
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

// (split kernels) the team's sets and the float32 teams' exchange area, zeroed (a zero dword = not yet arrived).  The float64 teams'
// area instead when `f64` (a call that goes to the float64 kernels with the whole batch leaves the float32 kernels' area alone); the
// finish kernel zeroes the float64 area of the utterances it leaves marked.  (A kernel of the library's own, not hipMemsetAsync:
// inside a captured hipGraph the runtime's memset node has been seen to overlap the team kernel behind it on replay -- the handshake
// granules of a launch wiped after they were published, every team timing out and every utterance recomputed by the exact kernels:
// round 6, tests/test_gpu_lfmmi.py::test_lfmmi_step_in_one_hip_graph; and the runtime's memset is two fill kernels, this is one)
static int bind_team_x(mm_batch_t h, RunParams &p, char *ws, const WsLayout &L, bool f64, void *stream) {
    const SplitInfo &si = h->fsms[0]->split;
    for (int s = 0; s < h->pair_H; ++s) {
        p.sp_base[s] = si.base[s];
        p.sp_cnt[s] = si.count[s];
    }
    p.xbuf = reinterpret_cast<float *>(ws + L.x);
    p.xps = reinterpret_cast<float *>(ws + L.x + L.x_rows);
    p.x_slot = 2ll * h->split_s1p;
    p.x_psn = mm_pair_xps(h->max_P1, h->pair_H);
    p.x_phase = (long long)(L.x_rows / 8);
    return f64 ? zero_dev(ws + L.xd, L.redo2 - L.xd, stream) : zero_dev(ws + L.x, L.xd - L.x, stream);
}

// the lane kernel decides per utterance whether its float64 range was enough (every workgroup writes its own mark: no zeroing
// pass); what it marks -- the one path of a left-to-right graph through values 1000 log2 below their frames' maxima -- goes to
// the wave kernel (whose workgroups of unmarked utterances leave at once; same workspace layout) or the item kernel
static int fb_lane(mm_batch_t h, RunParams &p, char *ws, const WsLayout &L, void *stream) {
    p.redo = reinterpret_cast<int *>(ws + L.redo);
    h->last_redo = p.redo;
    const int rc = mm_launch_lane(h->B, h->lane_S, p, static_cast<hipStream_t>(stream));
    if (rc || h->dbg.no_redo) return rc;
    if (h->lane_redo_wave) {
        p.pair_zmin = reinterpret_cast<double *>(ws + L.zmin);
        return mm_launch_wave(wave_launch_of(h), p, static_cast<hipStream_t>(stream));
    }
    return redo_on_items(h, p, stream);
}

// the stream kernels (forward launch, backward launch, finish), then -- for the utterances whose range marks stay: values beyond
// the double's range that carry mass, normally none -- the item kernel
static int fb_stream(mm_batch_t h, RunParams &p, char *ws, const WsLayout &L, void *stream) {
    p.pair_zmin = reinterpret_cast<double *>(ws + L.zmin);
    h->last_redo = p.redo;
    h->last_z = p.pair_zmin;
    p.xbuf = reinterpret_cast<float *>(ws + L.stream[0]);    // the backward direction's vectors
    p.xbuf_d = reinterpret_cast<float *>(ws + L.stream[1]);  // ... and offsets (doubles)
    p.xps = reinterpret_cast<float *>(ws + L.stream[2]);     // the frames' {log2 Z, overlap term} (doubles)
    if (h->stream_H > 1) {  // the teams' exchange area: zeroed before every call (a zero dword = not yet arrived)
        p.sx = reinterpret_cast<unsigned *>(ws + L.stream[3]);
        p.sx_slot = (long long)mm_stream_slot(h->stream_S1);
        const int rc = zero_dev(p.sx, mm_stream_exchange_bytes(h->B, h->stream_H, h->stream_S1), stream);
        if (rc) return rc;
    }
    const int rc = mm_launch_stream(h->B, h->n_cus, h->stream_S1, h->max_P1, h->stream_H, p, static_cast<hipStream_t>(stream));
    if (rc || h->dbg.no_redo) return rc;
    return redo_on_items(h, p, stream);
}

static int fb_wave(mm_batch_t h, RunParams &p, char *ws, const WsLayout &L, void *stream) {
    p.pair_zmin = reinterpret_cast<double *>(ws + L.zmin);
    return mm_launch_wave(wave_launch_of(h), p, static_cast<hipStream_t>(stream));
}

// the quad kernels where they are usable, on emissions shifted by their per-frame maxima (see mm_shift_em_kernel), else -- and
// where they turn out not to be (MM_ERR_UNSUPPORTED) -- the item kernel
static int fb_exact(mm_batch_t h, const RunParams &p, char *ws, const WsLayout &L, void *stream) {
    if (h->quad_ok) {
        bool same_P = true;
        for (int64_t b = 1; b < h->B && same_P; ++b) same_P = h->fsms[b]->P1 == h->fsms[0]->P1;
        RunParams q = p;
        float *E = nullptr;
        if (same_P) {
            float *Vs = reinterpret_cast<float *>(ws + L.extra);
            E = reinterpret_cast<float *>(ws + L.em_max);
            hipLaunchKernelGGL(mm_shift_em_kernel, dim3(unsigned(h->B), 8), dim3(256), 0, static_cast<hipStream_t>(stream), p, Vs, E);
            HIP_TRY(hipGetLastError());
            q.V = Vs;
            q.vsb = int64_t(p.N) * int64_t(h->max_P1 - 1);
            q.vsn = h->max_P1 - 1;
        }
        const int rc = launch_quad(h, q, stream);
        if (rc != MM_ERR_UNSUPPORTED) {
            if (!rc && same_P) {
                hipLaunchKernelGGL(mm_shift_ttl_kernel, dim3(unsigned(h->B)), dim3(256), 0, static_cast<hipStream_t>(stream), p, E);
                HIP_TRY(hipGetLastError());
            }
            return rc;
        }
    }
    return launch_log<MODE_FB>(h, p, stream);
}

// the pair, team or row kernels, then -- for the utterances they marked (linear sums outside the trusted range), normally none:
// every workgroup then leaves at once -- the float64 pair kernels (the whole batch, and first, when exact_first), and for what
// THEY mark -- values beyond the double's range that carry mass -- the log-domain kernels
static int fb_linear(mm_batch_t h, RunParams &p, char *ws, const WsLayout &L, bool exact_first, void *stream) {
    h->last_redo = p.redo;
    h->last_exact_first = exact_first;
    int rc;
    if (h->fb == Fb::Rows) {
        rc = launch_rows(h, p, stream);
    } else {
        p.pair_s1p = h->pair_H > 1 ? h->split_s1p : h->max_S1p;
        p.pair_hand = ws + L.hand;
        p.pair_zmin = reinterpret_cast<double *>(ws + L.zmin);
        if (h->fb == Fb::Split) {
            p.xbuf_d = reinterpret_cast<float *>(ws + L.xd);
            p.xps_d = reinterpret_cast<float *>(ws + L.xd + L.xd_rows);
            p.x_phase_d = (long long)(L.xd_rows / 8);
            p.x_H = h->dpair_ok ? h->pair_H : 0;
            rc = bind_team_x(h, p, ws, L, exact_first, stream);
            if (rc) return rc;
        }
        h->last_z = p.pair_zmin;
        rc = exact_first ? MM_OK : launch_pairs(h, p, stream);
    }
    if (rc) return rc;
    if (h->dbg.no_redo && !exact_first) return MM_OK;
    if (h->dpair_ok) {
        // a whole batch (exact_first: every utterance is marked): two utterances per workgroup on the wide pair kernels
        const PairLaunch pl = pair_launch_of(h);
        rc = exact_first && h->wpair_ok ? mm_launch_wpairs(pl, p, static_cast<hipStream_t>(stream)) : mm_launch_dpairs(pl, p, static_cast<hipStream_t>(stream));
        if (rc) return rc;
        h->last_redo2 = p.redo2;
        p.redo = p.redo2;
        if (h->dbg.no_redo || h->dbg.no_fallback) return MM_OK;
        if (!h->quad_ok) return redo_on_items(h, p, stream);
    }
    return fb_exact(h, p, ws, L, stream);
}

int mm_pdfposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                         float *gamma, int64_t gsb, int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    if (h && h->semiring == MM_PROB) return prob_pdfposteriors(h, V, vsb, vsn, lens, N, gamma, gsb, gsn, gsp, ttl, stream);
    int rc = check_run(h, "mm_pdfposteriors_f32", V, N, MM_LOG);
    if (rc) return rc;
    if (!gamma || !ttl) return fail(MM_ERR_INVALID, "mm_pdfposteriors_f32: gamma/ttl is NULL");
    // more utterances than CUs and different lengths: hand the workgroups out longest first; the pair kernels also
    // pair the utterances in that order (the two of a pair run the same number of frames)
    const bool ordered = lens && (h->B > h->n_cus || on_pairs(h)) && h->B <= 8192;
    const WsLayout L = ws_layout(h, N);
    rc = ensure_ws(h, L.total, stream);
    if (rc) return rc;
    char *const ws = static_cast<char *>(h->ws);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    p.x_sleep = h->dbg.x_sleep;
    // (the backward agent's phase-B steps are ~10 % dearer than the forward agent's on the pair kernels -- cycle stamps, config 3:
    // 4990 against 4520 --, the phase-A steps alike: the cut that levels both launches lies at 0.48 of the frames; the steps of
    // the team kernels are bound by the exchange, the same in both directions)
    p.split_q10 = h->dbg.split_q10 > 0 ? h->dbg.split_q10 : (h->pair_H == 1 ? MM_PAIR_SPLIT_Q10 : 512);
    p.x_timeout = x_timeout(N);
    p.lt_floor = h->lt_floor;
    p.clear_marks = h->keep_marks ? 0 : 1;
    p.g_scale = h->g_scale;
    p.g_acc = h->g_acc ? 1 : 0;
    p.ws_alpha = reinterpret_cast<float *>(ws + L.alpha);
    p.ws_c = reinterpret_cast<double *>(ws + L.c);
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    p.ttl = ttl;
    p.xcsr = h->xcsr;
    int *const order = ordered ? reinterpret_cast<int *>(ws + L.order) : nullptr;
    p.order = order;
    const bool marks = h->fb == Fb::Rows || on_pairs(h) || h->fb == Fb::Stream;
    // Which kernels first?  The float32 pair kernels, unless the inputs of the last finished call were beyond them for some of
    // its utterances (a sharp acoustic model marks every utterance) AND starting with the float64 kernels costs no more rounds
    // of workgroups than the float32 kernels followed by the float64 kernels for that many utterances would -- a launch lasts as
    // long as its rounds (one workgroup per compute unit), whatever the number of workgroups in the last of them: config 3
    // (B = 256: one round of pairs, two of single utterances) with 38 utterances marked is 6.0 ms float32-first, 5.5 ms
    // float64-first; B = 512 with the same 38 stays float32-first.  (Until round 4: "more than a quarter of the utterances".)
    // The float64 kernels keep reporting (how many utterances have an overlap term below the float32 kernels' floor), so the
    // choice follows the data back as well.  Read without synchronising: the count of whatever call finished last.
    bool exact_first = false;
    if (marks) {
        p.redo = reinterpret_cast<int *>(ws + L.redo);
        if (h->dpair_ok) {
            const int64_t M = h->stat_host[0], H = h->pair_H, cus = std::max(1, h->n_cus);
            auto rounds = [&](int64_t wgs) { return (wgs + cus - 1) / cus; };
            // (the wide pair kernels take a whole batch in the float32 kernels' one grid per phase, a third slower: cheaper than the
            // float32 kernels followed by a round of the float64 ones for ANY number of marked utterances)
            const bool by_rounds = M > 0 && (h->wpair_ok || rounds(2 * h->B * H) <= rounds(2 * ((h->B + 1) / 2) * H) + rounds(2 * std::min<int64_t>(M, h->B) * H));
            // (a capture must not bake in the marks of whatever call finished last: the automatic choice is float32-first there)
            exact_first = h->exact_first >= 0 ? h->exact_first != 0 : (by_rounds && !capturing(stream));
            p.redo2 = reinterpret_cast<int *>(ws + L.redo2);
            p.stat_dev = h->stat_dev;
            p.stat_xcd = h->xcd_counting ? 1 : 0;
            p.stat_host = h->stat_host;
            p.stat_seq = ++h->stat_seq;
            p.stat_mode = exact_first ? 1 : 0;
        }
    }
    if (ordered || marks) {
        // (the marks are set here, on the caller's stream, ahead of everything: the forward and the backward agents run
        // concurrently and either may mark an utterance first)
        hipLaunchKernelGGL(mm_prologue_kernel, dim3(unsigned((h->B + 1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           lens, int(h->B), int(N), order, p.redo, p.redo2, exact_first ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    bind_stamps(h, p);
    switch (h->fb) {
    case Fb::Lane: return fb_lane(h, p, ws, L, stream);
    case Fb::Stream: return fb_stream(h, p, ws, L, stream);
    case Fb::Wave: return fb_wave(h, p, ws, L, stream);
    case Fb::Rows:
    case Fb::Pairs:
    case Fb::Split: return fb_linear(h, p, ws, L, exact_first, stream);
    case Fb::Quad:
    case Fb::Item: break;
    }
    return fb_exact(h, p, ws, L, stream);
}

}  // extern "C"
// ---- the entries on the item form beside pdfposteriors: arc posteriors, path sampling, expected cost, leaky posteriors, path entropy,
// filtering posteriors, window posteriors (log batches only)

// What they start with: the semiring refusal, check_run, the entry's own argument checks (`args`), the item forms -- ahead
// of the plan: a batch created without them has max_items = 0 until they are up, and the plan would size the workgroups for no
// items --, then the plan.  Its refusals come with the workspace (item_ws_bind), behind what the entry checks on its derived forms.
template <class Args>
static int item_entry_begin(mm_batch_t h, const char *who, ItemEntry e, const float *V, int64_t N, void *stream, Args args, ItemPlan *pl) {
    if (h && h->semiring != MM_LOG)
        return fail(MM_ERR_UNSUPPORTED, std::string(who) + ": log-semiring batches only (this batch is " +
                                            std::string(h->semiring == MM_TROPICAL ? "tropical" : "ProbSemiring") + ")");
    int rc = check_run(h, who, V, N, MM_LOG);
    if (!rc) rc = args();
    if (!rc) rc = ensure_item_forms(h, stream);
    if (!rc) *pl = item_plan(h, e);
    return rc;
}

// Where they keep what they keep in h->ws for N frames: byte offsets, each aligned to 256 bytes.  The alpha~ store (at 0) and
// the per-frame offsets as the item kernel keeps them (all that Leaky, Window and Segment keep); Arcs: the float64 sums of all backward slots, the state posteriors of
// frame 1; Cost: the r store and its offsets, and for FSMs beyond the LDS the state vectors of both kernels ([B][8 * max S1p]
// floats); Entropy: as Cost, the Hf store in the place of the r store -- and no such store for a value-only call (`store` false).
// total: no less than what mm_pdfposteriors_f32 needs for as many frames.  (mm_batch_reserve does not cover it.)  Filter keeps
// nothing: its offsets stay in registers, total = 0 whatever N -- the workspace is neither grown nor touched.  ArcClass: what Leaky
// keeps, and the two term rows of every utterance when the plan has more ranks than the LDS holds; Scored: the same.
// ClassCost: what Cost keeps.
struct ItemWs { size_t c = 0, acc = 0, post1 = 0, r = 0, o = 0, big = 0, plane[2] = {0, 0}, initp = 0, utts = 0, terms = 0, total = 0; };
// Weighted: the arc entry's areas, then what the call's weights need (wplanes / wiplanes: 0 none given, 1 one vector for the batch
// -- the planes of ONE FSM --, 2 a vector per utterance): the {col, w} planes of both item forms, the dense init vectors, the call's
// descriptors.
static ItemWs item_ws_layout(mm_batch_t h, const ItemPlan &pl, int64_t N, bool store = true, int wplanes = 0, int wiplanes = 0) {
    ItemWs W;
    if (pl.e == ItemEntry::Filter) return W;
    const size_t rows = align_up(size_t(h->total_s1p) * size_t(N + 1) * 4, 256);
    W.c = rows;
    W.total = W.c + ws_c_bytes(h, N);
    if (pl.e == ItemEntry::Arcs || pl.e == ItemEntry::Weighted) {
        W.acc = W.total;
        W.post1 = W.acc + align_up(size_t(h->arc_slots) * 8, 256);
        W.total = W.post1 + align_up(size_t(h->total_s1p) * 4, 256);
        if (pl.e == ItemEntry::Weighted && (wplanes || wiplanes)) {
            const mm_fsm_s &f0 = *h->fsms[0];
            for (int d = 0; d < 2; ++d) {
                W.plane[d] = W.total;
                W.total += align_up(size_t(wplanes == 2 ? h->w_slots[d] : wplanes == 1 ? f0.packed[d].n_slot_rows * 64 : 0) * sizeof(Slot), 256);
            }
            W.initp = W.total;
            W.total += align_up(size_t(wiplanes == 2 ? h->total_s1p : wiplanes == 1 ? f0.S1p : 0) * 4, 256);
            W.utts = W.total;
            W.total += align_up(size_t(h->B) * sizeof(UttDesc), 256);
        }
    } else if (pl.e == ItemEntry::ArcClass || pl.e == ItemEntry::Scored) {
        W.terms = W.total;
        const int64_t cap = pl.e == ItemEntry::Scored ? scored_term_cap(pl, h->cls_C) : arcclass_cap(pl);
        W.total += h->cls_max_M > cap ? align_up(size_t(h->cls_terms) * 2 * sizeof(float), 256) : 0;
    } else if (ws_holds_big(pl.e)) {
        W.r = W.total;
        W.o = W.r + (store ? rows : 0);
        W.big = W.o + ws_c_bytes(h, N);
        W.total = W.big + (pl.global ? align_up(size_t(h->B) * 8 * size_t(h->max_S1p) * 4, 256) : 0);
    }
    W.total = std::max(W.total, mm_batch_workspace_bytes(h, N));
    return W;
}
// refuses what the plan cannot run, grows the workspace to the layout and binds the call to it
static int item_ws_bind(mm_batch_t h, const ItemPlan &pl, const ItemWs &W, RunParams &p, void *stream) {
    int rc = item_plan_check(h, pl);
    if (!rc) rc = ensure_ws(h, W.total, stream);
    if (rc) return rc;
    p.ws_alpha = static_cast<float *>(h->ws);
    p.ws_c = reinterpret_cast<double *>(static_cast<char *>(h->ws) + W.c);
    bind_big(h, pl, p);
    return MM_OK;
}

// The derived forms of a batch (arc forms, sampling forms): per FSM one blob that `pack` fills on the host, uploaded once per FSM
// (f->*blob); per utterance one Dev that `describe` fills, uploaded once per batch (`descs`).  Made on the first call of the entry
// that needs them, like the item forms: never during a stream capture.  A failed upload leaves nothing behind: the next call tries again.
template <class Dev, class Pack, class Describe>
static int ensure_derived_forms(mm_batch_t h, void *stream, const char *what, const char *who, DevMem &descs, DevMem mm_fsm_s::*blob, Pack pack,
                                Describe describe) {
    if (descs) return MM_OK;
    if (capturing(stream))
        return fail(MM_ERR_INVALID, std::string("the ") + what + " forms of this batch are not on the device yet: run " + who + " once outside a stream capture");
    std::vector<Dev> host(size_t(h->B));
    for (int64_t b = 0; b < h->B; ++b) {
        mm_fsm_t f = h->fsms[size_t(b)];
        if (f->nnz > INT32_MAX) return fail(MM_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 arcs in one FSM");
        if (!(f->*blob)) {
            Blob bl;
            pack(f, bl);
            const int rc = upload(bl, f->*blob);
            if (rc) return rc;
        }
        host[size_t(b)] = describe(f);
    }
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(Dev) * host.size()));
    DevMem own(d);
    if (hipMemcpy(d, host.data(), sizeof(Dev) * host.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MM_ERR_HIP, std::string(who) + ": upload of the " + what + " descriptors failed");
    descs = std::move(own);
    return MM_OK;
}
extern "C" {

// ---- arc posteriors (mm_kernel_arcs.hip)
// the slot (slot row * 64 + lane) of the backward item form that holds each caller entry; -1: none
static std::vector<int32_t> pack_k2slot(const mm_fsm_s &f) {
    const Packed &pk = f.packed[1];  // (ensure_item_forms packed it)
    std::vector<int32_t> k2slot(size_t(f.nnz), -1);
    const std::vector<int64_t> &rowptr = f.mat[1].rowptr;
    for (size_t it = 0; it < pk.items.size(); ++it) {
        const ItemMeta &im = pk.items[it];
        const int g = 1 << im.log2g;
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t row = pk.rowinfo[it * 64 + size_t(lane)].row;
            if (row < 0) continue;
            // (pack_rows: lane `sub` of the row's group holds arcs sub, sub + g, ... in slots k = 0, 1, ...)
            int64_t k = 0;
            for (int64_t a = rowptr[size_t(row)] + (lane & (g - 1)); a < rowptr[size_t(row) + 1]; a += g, ++k)
                k2slot[size_t(f.bwd_caller[size_t(a)])] = int32_t((int64_t(im.slot_row) + k) * 64 + lane);
        }
    }
    return k2slot;
}
// The arc forms: per FSM k2slot and the initial states in init_idx order; per utterance an ArcDev with its first slot in the
// float64 sums.
static int ensure_arc_forms(mm_batch_t h, void *stream) {
    int64_t slots = 0;
    const int rc = ensure_derived_forms<ArcDev>(
        h, stream, "arc", "mm_arcposteriors_f32", h->d_arcs, &mm_fsm_s::arc_blob,
        [](mm_fsm_t f, Blob &bl) {
            (void)bl.add(pack_k2slot(*f));  // (at 0)
            (void)bl.add(f->init_order);
        },
        [&](mm_fsm_t f) {
            const char *base = static_cast<const char *>(f->arc_blob.get());
            const size_t o_i = align_up(size_t(f->nnz) * 4, 256);  // (where Blob::add put init_order, behind k2slot)
            const ArcDev a{reinterpret_cast<const int *>(base), reinterpret_cast<const int *>(base + o_i), slots, int(f->nnz), int(f->init_order.size()),
                           int(f->kphony), 0};
            slots += f->packed[1].n_slot_rows * 64;
            h->arc_max_nnz = std::max<int64_t>(h->arc_max_nnz, f->nnz);
            h->arc_max_init = std::max<int64_t>(h->arc_max_init, int64_t(f->init_order.size()));
            return a;
        });
    if (!rc && slots) h->arc_slots = slots;  // (0: they were up already)
    return rc;
}

int mm_arcposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, float *counts,
                         int64_t csb, float *init_counts, int64_t isb, float *ttl, void *stream) {
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_arcposteriors_f32", ItemEntry::Arcs, V, N, stream,
                              [&]() { return counts ? int(MM_OK) : fail(MM_ERR_INVALID, "mm_arcposteriors_f32: counts is NULL"); }, &pl);
    if (rc) return rc;
    rc = ensure_arc_forms(h, stream);
    if (rc) return rc;
    if (csb < h->arc_max_nnz)
        return fail(MM_ERR_DIM, "mm_arcposteriors_f32: c_stride_b " + std::to_string(csb) + " < " + std::to_string(h->arc_max_nnz) + " entries of the largest FSM");
    if (init_counts && isb < h->arc_max_init)
        return fail(MM_ERR_DIM, "mm_arcposteriors_f32: i_stride_b " + std::to_string(isb) + " < " + std::to_string(h->arc_max_init) + " initial states of the largest FSM");
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    char *ws = static_cast<char *>(h->ws);
    ArcParams ap{};
    ap.arcs = static_cast<const ArcDev *>(h->d_arcs.get());
    ap.acc = reinterpret_cast<double *>(ws + W.acc);
    ap.post1 = reinterpret_cast<float *>(ws + W.post1);
    ap.counts = counts;
    ap.csb = csb;
    ap.init_counts = init_counts;
    ap.isb = isb;
    ap.ttl = ttl;
    return mm_launch_arcs(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, ap, static_cast<hipStream_t>(stream));
}

static int check_strides(const std::string &who, const char *name, int64_t sb, int64_t B, int64_t sn, int64_t N, int64_t sp, int64_t P);

// ---- per-frame arc-class posteriors (mm_kernel_arcclass.hip)
// One class plan: the classified entries of FSM f under the class array cls (f->nnz ids in [-1, C)) ranked by (class, entry), a
// record each, and the classes' rank ranges.  An entry without a slot (a row without an item: no path takes it) has no rank.
struct ClassPlanHost {
    std::vector<ClassRec> recs;
    std::vector<int32_t> cptr;
    int cphony = -1;
};
static std::vector<int32_t> pack_slot2k(const mm_fsm_s &f, int d);
// The class plane of item form d under the class array cls: the class id of the entry behind every slot; an entry without a class,
// the phony self-loop and the padding slots carry the id C.  (mm_kernel_scored.hip)
static std::vector<uint16_t> make_class_plane(const mm_fsm_s &f, int d, const int32_t *cls, int32_t C) {
    const std::vector<int32_t> s2k = pack_slot2k(f, d);
    std::vector<uint16_t> plane(s2k.size(), uint16_t(C));
    for (size_t s = 0; s < s2k.size(); ++s)
        if (s2k[s] >= 0 && cls[s2k[s]] >= 0) plane[s] = uint16_t(cls[s2k[s]]);
    return plane;
}
static ClassPlanHost make_class_plan(mm_fsm_s &f, const int32_t *cls, int32_t C) {
    ensure_packed(&f);
    const Packed &pk = f.packed[1];
    const std::vector<int32_t> k2slot = pack_k2slot(f);
    std::vector<int32_t> slot2row(pk.slots.size(), -1);
    for (size_t it = 0; it < pk.items.size(); ++it)
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t row = pk.rowinfo[it * 64 + size_t(lane)].row;
            for (int k = 0; row >= 0 && k < int(pk.items[it].R); ++k) slot2row[(size_t(pk.items[it].slot_row) + size_t(k)) * 64 + size_t(lane)] = row;
        }
    ClassPlanHost pl;
    pl.cptr.assign(size_t(C) + 1, 0);
    for (int64_t k = 0; k < f.nnz; ++k)
        if (cls[k] >= 0 && k2slot[size_t(k)] >= 0) ++pl.cptr[size_t(cls[k]) + 1];
    for (int32_t c = 0; c < C; ++c) pl.cptr[size_t(c) + 1] += pl.cptr[size_t(c)];
    pl.recs.resize(size_t(pl.cptr[size_t(C)]));
    std::vector<int32_t> cur(pl.cptr.begin(), pl.cptr.end() - 1);
    for (int64_t k = 0; k < f.nnz; ++k) {  // (k ascending: a class's ranks follow the caller's entry order)
        const int32_t s = k2slot[size_t(k)];
        if (cls[k] < 0 || s < 0) continue;
        const Slot &sl = pk.slots[size_t(s)];
        pl.recs[size_t(cur[size_t(cls[k])]++)] = ClassRec{slot2row[size_t(s)], int(sl.col), sl.w, int(k)};
    }
    if (f.kphony >= 0) pl.cphony = cls[f.kphony];
    return pl;
}

// The class planes of one (FSM, class array) in the blob of a setter: the forward item form's and, with the class plan `pl` of
// mm_batch_set_arc_classes, the backward form's and the ranks' classes (pl NULL -- mm_batch_set_path_classes --: the forward plane alone,
// the other offsets 0)
struct MadePlanes { size_t o_plane[2], o_rcls; };
static MadePlanes add_class_planes(Blob &sbl, const mm_fsm_s &f, const int32_t *cb, int32_t C, const ClassPlanHost *pl) {
    MadePlanes mp{{0, 0}, 0};
    mp.o_plane[0] = sbl.add(make_class_plane(f, 0, cb, C));
    if (!pl) return mp;
    std::vector<uint16_t> rcls(pl->recs.size());
    for (int32_t c = 0; c < C; ++c)
        for (int32_t r = pl->cptr[size_t(c)]; r < pl->cptr[size_t(c) + 1]; ++r) rcls[size_t(r)] = uint16_t(c);
    mp.o_plane[1] = sbl.add(make_class_plane(f, 1, cb, C));
    mp.o_rcls = sbl.add(rcls);
    return mp;
}
// what both setters refuse, after their own semiring check
static int check_class_args(const std::string &who, mm_batch_t h, const int32_t *cls, const int64_t *offsets, int32_t C) {
    if (C < 1) return fail(MM_ERR_INVALID, who + ": need C >= 1 classes, got " + std::to_string(C));
    const size_t B = size_t(h->B);
    for (size_t b = 0; b < B; ++b) {
        const mm_fsm_s &f = *h->fsms[b];
        if (f.nnz > INT32_MAX) return fail(MM_ERR_UNSUPPORTED, who + ": more than 2^31 - 1 arcs in one FSM");
        if (!offsets && h->fsms[b] != h->fsms[0]) return fail(MM_ERR_INVALID, who + ": one class array (offsets NULL) needs a batch of one shared FSM");
        if (offsets && offsets[b + 1] - offsets[b] != f.nnz)
            return fail(MM_ERR_DIM, who + ": utterance " + std::to_string(b) + " has " + std::to_string(offsets[b + 1] - offsets[b]) + " class ids for " +
                                        std::to_string(f.nnz) + " entries");
        const int32_t *cb = cls + (offsets ? offsets[b] : 0);
        for (int64_t k = 0; k < f.nnz && (offsets || b == 0); ++k)
            if (cb[k] < -1 || cb[k] >= C)
                return fail(MM_ERR_INVALID, who + ": class id " + std::to_string(cb[k]) + " of entry " + std::to_string(k) + " of utterance " + std::to_string(b) +
                                                " is outside [-1, " + std::to_string(C) + ")");
    }
    return MM_OK;
}

int mm_batch_set_arc_classes(mm_batch_t h, const int32_t *cls, const int64_t *offsets, int32_t C) {
    const std::string who = "mm_batch_set_arc_classes";
    if (!h || !cls) return fail(MM_ERR_INVALID, who + ": NULL argument");
    if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, who + ": log-semiring batches only");
    if (const int rc = check_class_args(who, h, cls, offsets, C)) return rc;
    const size_t B = size_t(h->B);
    return no_throw(who.c_str(), [&]() {
        // one plan per distinct (FSM, class array); the image: [B] descriptors, then per plan its records and class pointers
        struct Made { const mm_fsm_s *f; const int32_t *cls; size_t o_recs, o_cptr; int M, cphony; };
        std::vector<Made> made;
        std::vector<ClassDev> descs(B);
        Blob bl;
        (void)bl.add(descs);  // (at 0; filled in below)
        // the class planes of the scored entry, laid out the same way (none for more classes than a 16-bit id holds)
        const bool planes = C <= 65534;
        std::vector<MadePlanes> made_sc;
        std::vector<ScoredDev> sdescs(B);
        Blob sbl;
        (void)sbl.add(sdescs);
        int64_t terms = 0, max_M = 0;
        uint32_t lgl_mask = 0;
        for (size_t b = 0; b < B; ++b) {
            mm_fsm_s &f = *h->fsms[b];
            const int32_t *cb = cls + (offsets ? offsets[b] : 0);
            const Made *m = nullptr;
            for (const Made &c : made)
                if (c.f == &f && (c.cls == cb || std::equal(cb, cb + f.nnz, c.cls))) m = &c;
            if (!m) {
                const ClassPlanHost pl = make_class_plan(f, cb, C);
                const size_t o_recs = bl.add(pl.recs);
                made.push_back(Made{&f, cb, o_recs, bl.add(pl.cptr), int(pl.recs.size()), pl.cphony});
                m = &made.back();
                if (planes) made_sc.push_back(add_class_planes(sbl, f, cb, C, &pl));
            }
            if (planes) {
                const MadePlanes &mp = made_sc[size_t(m - made.data())];
                ScoredDev &sd = sdescs[b];
                sd.plane[0] = reinterpret_cast<const unsigned short *>(mp.o_plane[0]);
                sd.plane[1] = reinterpret_cast<const unsigned short *>(mp.o_plane[1]);
                sd.rcls = reinterpret_cast<const unsigned short *>(mp.o_rcls);
            }
            ClassDev &d = descs[b];
            d.recs = reinterpret_cast<const ClassRec *>(m->o_recs);
            d.cptr = reinterpret_cast<const int *>(m->o_cptr);
            d.term_off = terms;
            d.M = m->M;
            d.C = C;
            d.cphony = m->cphony;
            d.lgl = m->M >= 32ll * C ? 6 : (m->M >= 2ll * C ? 3 : 0);
            lgl_mask |= 1u << d.lgl;
            terms += m->M;
            max_M = std::max<int64_t>(max_M, m->M);
        }
        memcpy(bl.host.data(), descs.data(), sizeof(ClassDev) * B);
        h->cls_image = std::move(bl.host);
        h->d_cls = DevMem();  // (the next mm_arcclassposteriors_f32 call uploads the new plan)
        if (planes) memcpy(sbl.host.data(), sdescs.data(), sizeof(ScoredDev) * B);
        h->sc_image = planes ? std::move(sbl.host) : std::vector<char>();
        h->d_sc = DevMem();  // (... and the next mm_scoredposteriors_f32 call the new planes)
        h->cls_C = C;
        h->cls_max_M = max_M;
        h->cls_terms = terms;
        h->cls_lgl_mask = lgl_mask;
        return int(MM_OK);
    });
}

int mm_batch_arc_class_info(mm_batch_t h, int64_t *cap, int64_t *max_M, int32_t *C) {
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_arc_class_info: NULL batch");
    if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_arc_class_info: log-semiring batches only");
    if (cap) *cap = arcclass_cap(item_plan(h, ItemEntry::ArcClass));
    if (max_M) *max_M = h->cls_image.empty() ? -1 : h->cls_max_M;
    if (C) *C = h->cls_C;
    return MM_OK;
}

// the plan on the device: one allocation, one copy -- made by the first call behind mm_batch_set_arc_classes, never during a capture
static int ensure_class_plan(mm_batch_t h, void *stream) {
    if (h->d_cls) return MM_OK;
    if (capturing(stream))
        return fail(MM_ERR_INVALID, "the class plan of this batch is not on the device yet: run mm_arcclassposteriors_f32 once outside a stream capture");
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, h->cls_image.size()));
    DevMem own(d);
    std::vector<char> img = h->cls_image;  // (the descriptors' offsets become pointers into the allocation)
    ClassDev *descs = reinterpret_cast<ClassDev *>(img.data());
    for (int64_t b = 0; b < h->B; ++b) {
        descs[b].recs = reinterpret_cast<const ClassRec *>(static_cast<char *>(d) + reinterpret_cast<size_t>(descs[b].recs));
        descs[b].cptr = reinterpret_cast<const int *>(static_cast<char *>(d) + reinterpret_cast<size_t>(descs[b].cptr));
    }
    if (hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MM_ERR_HIP, "mm_arcclassposteriors_f32: upload of the class plan failed");
    h->d_cls = std::move(own);
    return MM_OK;
}

int mm_arcclassposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, float *xi, int64_t xsb,
                              int64_t xsn, int64_t xsc, float *ttl, void *stream) {
    const std::string who = "mm_arcclassposteriors_f32";
    ItemPlan pl;
    int rc = item_entry_begin(h, who.c_str(), ItemEntry::ArcClass, V, N, stream, [&]() {
        if (!xi) return fail(MM_ERR_INVALID, who + ": xi is NULL");
        if (h->cls_image.empty()) return fail(MM_ERR_INVALID, who + ": no classes set (mm_batch_set_arc_classes)");
        return check_strides(who, "x", xsb, h->B, xsn, N, xsc, h->cls_C);
    }, &pl);
    if (rc) return rc;
    rc = ensure_class_plan(h, stream);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    const bool tg = h->cls_max_M > arcclass_cap(pl);
    ArcClassParams cp{};
    cp.cls = static_cast<const ClassDev *>(h->d_cls.get());
    cp.terms = reinterpret_cast<float *>(static_cast<char *>(h->ws) + W.terms);
    cp.terms_global = tg ? 1 : 0;
    cp.xi = xi;
    cp.xsb = xsb;
    cp.xsn = xsn;
    cp.xsc = xsc;
    cp.ttl = ttl;
    return mm_launch_arcclass(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, tg ? 0 : size_t(h->cls_max_M) * 2 * sizeof(float), p, cp,
                              static_cast<hipStream_t>(stream));
}

// ---- expected path cost and its gradient (mm_kernel_cost.hip)
// an output laid out by three strides holds every element once: sorted by stride, each reaches past the extent of the one before
static bool strides_hold(int64_t sb, int64_t B, int64_t sn, int64_t N, int64_t sp, int64_t P) {
    std::pair<int64_t, int64_t> d[3] = {{sb, B}, {sn, N}, {sp, P}};
    std::sort(d, d + 3);
    int64_t need = 1;
    for (const auto &e : d) {
        if (e.second <= 1) continue;
        if (e.first < need) return false;
        need = e.first * e.second;
    }
    return true;
}
// the three strides of output `name` of entry `who` hold B x N x P elements, or MM_ERR_DIM with the message
static int check_strides(const std::string &who, const char *name, int64_t sb, int64_t B, int64_t sn, int64_t N, int64_t sp, int64_t P) {
    if (strides_hold(sb, B, sn, N, sp, P)) return MM_OK;
    return fail(MM_ERR_DIM, who + ": " + name + " strides (" + std::to_string(sb) + ", " + std::to_string(sn) + ", " + std::to_string(sp) +
                                ") cannot hold " + std::to_string(B) + " x " + std::to_string(N) + " x " + std::to_string(P) + " elements");
}

int mm_expectedcost_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *cost,
                        int64_t csb, int64_t csn, float *risk, float *grad, float *gamma, int64_t gsb, int64_t gsn, int64_t gsp, float *ttl,
                        void *stream) {
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_expectedcost_f32", ItemEntry::Cost, V, N, stream, [&]() {
        if (!cost || !risk || !grad) return fail(MM_ERR_INVALID, "mm_expectedcost_f32: cost / risk / grad is NULL");
        const int64_t P = h->max_P1 - 1;
        if (csn < P) return fail(MM_ERR_DIM, "mm_expectedcost_f32: c_stride_n " + std::to_string(csn) + " < " + std::to_string(P) + " pdfs");
        if (const int rc = check_strides("mm_expectedcost_f32", "g", gsb, h->B, gsn, N, gsp, P)) return rc;
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    char *ws = static_cast<char *>(h->ws);
    CostParams cp{};
    cp.cost = cost;
    cp.csb = csb;
    cp.csn = csn;
    cp.risk = risk;
    cp.grad = grad;
    cp.gamma = gamma;
    cp.gsb = gsb;
    cp.gsn = gsn;
    cp.gsp = gsp;
    cp.ttl = ttl;
    cp.ws_r = reinterpret_cast<float *>(ws + W.r);
    cp.ws_o = reinterpret_cast<double *>(ws + W.o);
    if (pl.global) {
        cp.ws_big = reinterpret_cast<float *>(ws + W.big);
        cp.big_stride = 8ll * h->max_S1p;
    }
    return mm_launch_cost(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, cp, static_cast<hipStream_t>(stream));
}

// ---- posterior path entropy and its gradient (mm_kernel_entropy.hip)
int mm_pathentropy_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, float *entropy, float *grad,
                       float *gamma, int64_t gsb, int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    ItemPlan pl;
    const bool backward = grad || gamma;  // neither: the forward kernel alone, no frame kept
    int rc = item_entry_begin(h, "mm_pathentropy_f32", ItemEntry::Entropy, V, N, stream, [&]() {
        if (!entropy) return fail(MM_ERR_INVALID, "mm_pathentropy_f32: entropy is NULL");
        const int64_t P = h->max_P1 - 1;
        if (backward) {
            const int rc = check_strides("mm_pathentropy_f32", "g", gsb, h->B, gsn, N, gsp, P);
            if (rc) return rc;
        }
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N, backward);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    char *ws = static_cast<char *>(h->ws);
    EntropyParams ep{};
    ep.entropy = entropy;
    ep.grad = grad;
    ep.gamma = gamma;
    ep.gsb = gsb;
    ep.gsn = gsn;
    ep.gsp = gsp;
    ep.ttl = ttl;
    ep.ws_h = backward ? reinterpret_cast<float *>(ws + W.r) : nullptr;
    ep.ws_o = reinterpret_cast<double *>(ws + W.o);
    if (pl.global) {
        ep.ws_big = reinterpret_cast<float *>(ws + W.big);
        ep.big_stride = 8ll * h->max_S1p;
    }
    return mm_launch_entropy(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, backward, p, ep, static_cast<hipStream_t>(stream));
}

// ---- forward filtering posteriors with a carried state (mm_kernel_filter.hip)
int mm_filterposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *state_in,
                            float *state_out, float *filt, int64_t fsb, int64_t fsn, int64_t fsp, float *incr, int64_t isb, float *ttl,
                            void *stream) {
    // what the arguments alone show comes first (without a batch: the frames' own extent), then the batch's refusals
    if (!state_out && !filt && !incr && !ttl) return fail(MM_ERR_INVALID, "mm_filterposteriors_f32: state_out, filt, incr and ttl are all NULL");
    if (incr && isb < N) return fail(MM_ERR_DIM, "mm_filterposteriors_f32: i_stride_b " + std::to_string(isb) + " < " + std::to_string(N) + " frames");
    {
        const int64_t B = h ? h->B : 1, P = h ? h->max_P1 - 1 : 1;
        if (filt) {
            const int rc = check_strides("mm_filterposteriors_f32", "f", fsb, B, fsn, N, fsp, P);
            if (rc) return rc;
        }
    }
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_filterposteriors_f32", ItemEntry::Filter, V, N, stream, []() { return int(MM_OK); }, &pl);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    FilterParams fp{};
    fp.state_in = state_in;
    fp.state_out = state_out;
    fp.filt = filt;
    fp.fsb = fsb;
    fp.fsn = fsn;
    fp.fsp = fsp;
    fp.incr = incr;
    fp.isb = isb;
    fp.ttl = ttl;
    return mm_launch_filter(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, fp, static_cast<hipStream_t>(stream));
}

// ---- fixed-lag smoothing posteriors: the forward-backward of a window with a carried start and an open end (mm_kernel_window.hip)
int mm_windowposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *state_in,
                            const int32_t *closed, const int32_t *commit, float *state_out, float *lcommit, float *gamma, int64_t gsb,
                            int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    // what the arguments alone show comes first (without a batch: the frames' own extent), then the batch's refusals
    if (!gamma) return fail(MM_ERR_INVALID, "mm_windowposteriors_f32: gamma is NULL");
    {
        const int64_t B = h ? h->B : 1, P = h ? h->max_P1 - 1 : 1;
        if (const int rc = check_strides("mm_windowposteriors_f32", "g", gsb, B, gsn, N, gsp, P)) return rc;
    }
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_windowposteriors_f32", ItemEntry::Window, V, N, stream, []() { return int(MM_OK); }, &pl);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    p.ttl = ttl;
    WindowParams wp{};
    wp.state_in = state_in;
    wp.state_out = state_out;
    wp.closed = closed;
    wp.commit = commit;
    wp.lcommit = lcommit;
    return mm_launch_window(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, wp, static_cast<hipStream_t>(stream));
}

// ---- segment posteriors: the forward-backward of a segment with a carried start and a carried end (mm_kernel_segment.hip)
int mm_segmentposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *state_in,
                             const int32_t *end_mode, const float *end_in, float *end_out, float *lend, float *gamma, int64_t gsb,
                             int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    // what the arguments alone show comes first (without a batch: the frames' own extent), then the batch's refusals
    if (!gamma) return fail(MM_ERR_INVALID, "mm_segmentposteriors_f32: gamma is NULL");
    {
        const int64_t B = h ? h->B : 1, P = h ? h->max_P1 - 1 : 1;
        if (const int rc = check_strides("mm_segmentposteriors_f32", "g", gsb, B, gsn, N, gsp, P)) return rc;
    }
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_segmentposteriors_f32", ItemEntry::Segment, V, N, stream, []() { return int(MM_OK); }, &pl);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    p.ttl = ttl;
    SegmentParams sp{};
    sp.state_in = state_in;
    sp.end_mode = end_mode;
    sp.end_in = end_in;
    sp.end_out = end_out;
    sp.lend = lend;
    return mm_launch_segment(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, sp, static_cast<hipStream_t>(stream));
}

// ---- posteriors with call-time arc weights (mm_kernel_weighted.hip)
// the caller entry behind every slot of item form d (-1: a padding slot, or the phony self-loop -- they keep the FSM's own weight)
static std::vector<int32_t> pack_slot2k(const mm_fsm_s &f, int d) {
    const Packed &pk = f.packed[d];  // (ensure_item_forms packed it)
    std::vector<int32_t> slot2k(size_t(pk.n_slot_rows) * 64, -1);
    const std::vector<int64_t> &rowptr = f.mat[d].rowptr;
    // the caller's entry of every entry of mat[d]: bwd_caller for T_hat; for T_hat' (rows = destinations, sources ascending, ties in
    // T_hat's order: transpose is stable) the walk over T_hat that transpose made
    std::vector<int64_t> caller;
    if (d == 1) {
        caller = f.bwd_caller;
    } else {
        caller.resize(size_t(f.nnz));
        std::vector<int64_t> cur(rowptr.begin(), rowptr.end() - 1);
        const Csr &bwd = f.mat[1];
        for (int64_t i = 0; i < f.S1; ++i)
            for (int64_t a = bwd.rowptr[size_t(i)]; a < bwd.rowptr[size_t(i) + 1]; ++a) caller[size_t(cur[size_t(bwd.col[size_t(a)])]++)] = f.bwd_caller[size_t(a)];
    }
    for (size_t it = 0; it < pk.items.size(); ++it) {
        const ItemMeta &im = pk.items[it];
        const int g = 1 << im.log2g;
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t row = pk.rowinfo[it * 64 + size_t(lane)].row;
            if (row < 0) continue;
            // (pack_rows: lane `sub` of the row's group holds arcs sub, sub + g, ... in slots k = 0, 1, ...)
            int64_t k = 0;
            for (int64_t a = rowptr[size_t(row)] + (lane & (g - 1)); a < rowptr[size_t(row) + 1]; a += g, ++k) {
                const int64_t c = caller[size_t(a)];
                if (c != f.kphony) slot2k[size_t((int64_t(im.slot_row) + k) * 64 + lane)] = int32_t(c);
            }
        }
    }
    return slot2k;
}
// The weight forms: per FSM slot2k of both directions and state2init; per utterance a WeightDev with its first slots in the planes.
// With them the batch's global vectors where only this entry's LDS plan asks for them (as ensure_leak_rows).
static int ensure_weight_forms(mm_batch_t h, const ItemPlan &pl, void *stream) {
    if (pl.global && !h->ws_big) {
        if (capturing(stream))
            return fail(MM_ERR_INVALID, "the global vectors of this batch are not on the device yet: run mm_weightedposteriors_f32 once outside a stream capture");
        if (hipMalloc(&h->ws_big, size_t(h->B) * 4 * size_t(h->max_S1p) * sizeof(float)) != hipSuccess) {
            h->ws_big = nullptr;
            return fail(MM_ERR_HIP, "mm_weightedposteriors_f32: device allocation failed");
        }
    }
    int64_t slots[2] = {0, 0};
    const int rc = ensure_derived_forms<WeightDev>(
        h, stream, "weight", "mm_weightedposteriors_f32", h->d_wforms, &mm_fsm_s::weight_blob,
        [](mm_fsm_t f, Blob &bl) {
            (void)bl.add(pack_slot2k(*f, 0));  // (at 0)
            (void)bl.add(pack_slot2k(*f, 1));
            std::vector<int32_t> s2i(size_t(f->S1), -1);
            for (size_t m = 0; m < f->init_order.size(); ++m) s2i[size_t(f->init_order[m])] = int32_t(m);  // (a state given twice: the last, as mm_fsm_create)
            (void)bl.add(s2i);
        },
        [&](mm_fsm_t f) {
            const char *base = static_cast<const char *>(f->weight_blob.get());
            const int64_t n0 = f->packed[0].n_slot_rows * 64, n1 = f->packed[1].n_slot_rows * 64;
            const size_t o1 = align_up(size_t(n0) * 4, 256), o2 = align_up(o1 + size_t(n1) * 4, 256);  // (where Blob::add put them)
            WeightDev w{};
            w.slot2k[0] = reinterpret_cast<const int *>(base);
            w.slot2k[1] = reinterpret_cast<const int *>(base + o1);
            w.state2init = reinterpret_cast<const int *>(base + o2);
            w.plane_off[0] = slots[0];
            w.plane_off[1] = slots[1];
            w.nslots[0] = int(n0);
            w.nslots[1] = int(n1);
            slots[0] += n0;
            slots[1] += n1;
            return w;
        });
    if (!rc && slots[1]) {  // (0: they were up already)
        h->w_slots[0] = slots[0];
        h->w_slots[1] = slots[1];
    }
    return rc;
}

int mm_weightedposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *Wt, int64_t wsb,
                              const float *Wi, int64_t wisb, float *gamma, int64_t gsb, int64_t gsn, int64_t gsp, float *counts, int64_t csb,
                              float *init_counts, int64_t isb, float *ttl, void *stream) {
    const char *who = "mm_weightedposteriors_f32";
    // what the arguments alone show comes first (without a batch: the frames' own extent), then the batch's refusals
    if (!gamma && !counts && !init_counts && !ttl) return fail(MM_ERR_INVALID, std::string(who) + ": gamma, counts, init_counts and ttl are all NULL");
    if ((Wt && wsb < 0) || (Wi && wisb < 0))
        return fail(MM_ERR_DIM, std::string(who) + ": w_stride_b " + std::to_string(wsb) + " / wi_stride_b " + std::to_string(wisb) + " is negative");
    if (gamma) {
        const int64_t B = h ? h->B : 1, P = h ? h->max_P1 - 1 : 1;
        if (const int rc = check_strides(who, "g", gsb, B, gsn, N, gsp, P)) return rc;
    }
    if (h && h->semiring == MM_LOG) {  // (the batch's own numbers need no device either)
        bool same = true;
        int64_t max_nnz = 0, max_init = 0;
        for (int64_t b = 0; b < h->B; ++b) {
            same &= h->fsms[size_t(b)] == h->fsms[0];
            max_nnz = std::max<int64_t>(max_nnz, h->fsms[size_t(b)]->nnz);
            max_init = std::max<int64_t>(max_init, int64_t(h->fsms[size_t(b)]->init_order.size()));
        }
        if (((Wt && wsb == 0) || (Wi && wisb == 0)) && !same)
            return fail(MM_ERR_INVALID, std::string(who) + ": stride 0 (one weight vector for the batch) needs all " + std::to_string(h->B) + " handles of the batch to be the same FSM");
        if (Wt && wsb > 0 && wsb < max_nnz)
            return fail(MM_ERR_DIM, std::string(who) + ": w_stride_b " + std::to_string(wsb) + " < " + std::to_string(max_nnz) + " entries of the largest FSM");
        if (Wi && wisb > 0 && wisb < max_init)
            return fail(MM_ERR_DIM, std::string(who) + ": wi_stride_b " + std::to_string(wisb) + " < " + std::to_string(max_init) + " initial states of the largest FSM");
        if (counts && csb < max_nnz)
            return fail(MM_ERR_DIM, std::string(who) + ": c_stride_b " + std::to_string(csb) + " < " + std::to_string(max_nnz) + " entries of the largest FSM");
        if (init_counts && isb < max_init)
            return fail(MM_ERR_DIM, std::string(who) + ": i_stride_b " + std::to_string(isb) + " < " + std::to_string(max_init) + " initial states of the largest FSM");
    }
    ItemPlan pl;
    int rc = item_entry_begin(h, who, ItemEntry::Weighted, V, N, stream, []() { return int(MM_OK); }, &pl);
    if (rc) return rc;
    rc = ensure_arc_forms(h, stream);
    if (!rc) rc = ensure_weight_forms(h, pl, stream);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N, true, Wt ? (wsb == 0 ? 1 : 2) : 0, Wi ? (wisb == 0 ? 1 : 2) : 0);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    char *ws = static_cast<char *>(h->ws);
    WeightedParams wp{};
    wp.arcs = static_cast<const ArcDev *>(h->d_arcs.get());
    wp.wforms = static_cast<const WeightDev *>(h->d_wforms.get());
    wp.utts_own = h->d_utts;
    wp.utts_call = (Wt || Wi) ? reinterpret_cast<UttDesc *>(ws + W.utts) : nullptr;
    wp.W = Wt;
    wp.wsb = wsb;
    wp.W_init = Wi;
    wp.wisb = wisb;
    wp.plane[0] = reinterpret_cast<Slot *>(ws + W.plane[0]);
    wp.plane[1] = reinterpret_cast<Slot *>(ws + W.plane[1]);
    wp.init_plane = reinterpret_cast<float *>(ws + W.initp);
    wp.acc = reinterpret_cast<double *>(ws + W.acc);
    wp.post1 = reinterpret_cast<float *>(ws + W.post1);
    wp.counts = counts;
    wp.csb = csb;
    wp.init_counts = init_counts;
    wp.isb = isb;
    wp.ttl = ttl;
    // (the forward launch is the arc entry's: the item kernel's plan of the same placement)
    const size_t lds_fwd = size_t(lds_plan(pl.global ? 0 : h->max_S1p, (h->max_P1 + 3) & ~3, true).total) * 4;
    return mm_launch_weighted(h->B, pl.NW, pl.NI, pl.global, lds_fwd, pl.lds_bytes, p, wp, static_cast<hipStream_t>(stream));
}

// ---- posteriors with per-frame arc-class scores (mm_kernel_scored.hip)
int mm_batch_score_class_cap(mm_batch_t h, int64_t *cap) {
    if (!h || !cap) return fail(MM_ERR_INVALID, "mm_batch_score_class_cap: NULL argument");
    if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_score_class_cap: log-semiring batches only");
    *cap = scored_class_cap(item_plan(h, ItemEntry::Scored));
    return MM_OK;
}

// the class planes on the device: one allocation, one copy -- made by the first call behind mm_batch_set_arc_classes, never during a
// capture (as ensure_class_plan)
static int ensure_score_planes(mm_batch_t h, void *stream, const char *who = "mm_scoredposteriors_f32") {
    if (h->d_sc) return MM_OK;
    if (capturing(stream))
        return fail(MM_ERR_INVALID, std::string("the class planes of this batch are not on the device yet: run ") + who + " once outside a stream capture");
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, h->sc_image.size()));
    DevMem own(d);
    std::vector<char> img = h->sc_image;  // (the descriptors' offsets become pointers into the allocation)
    ScoredDev *descs = reinterpret_cast<ScoredDev *>(img.data());
    auto at = [&](const unsigned short *off) { return reinterpret_cast<const unsigned short *>(static_cast<char *>(d) + reinterpret_cast<size_t>(off)); };
    for (int64_t b = 0; b < h->B; ++b) {
        descs[b].plane[0] = at(descs[b].plane[0]);
        descs[b].plane[1] = at(descs[b].plane[1]);  // (a plan of mm_batch_set_path_classes has the forward plane alone: nobody reads the others)
        descs[b].rcls = at(descs[b].rcls);
    }
    if (hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MM_ERR_HIP, std::string(who) + ": upload of the class planes failed");
    h->d_sc = std::move(own);
    return MM_OK;
}

int mm_scoredposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *U, int64_t usb,
                            int64_t usn, int64_t usc, float *gamma, int64_t gsb, int64_t gsn, int64_t gsp, float *xi, int64_t xsb, int64_t xsn,
                            int64_t xsc, float *ttl, void *stream) {
    const std::string who = "mm_scoredposteriors_f32";
    // what the arguments alone show comes first (without a batch: the frames' own extent), then the batch's refusals
    if (!gamma && !xi && !ttl) return fail(MM_ERR_INVALID, who + ": gamma, xi and ttl are all NULL");
    if (gamma) {
        const int64_t B = h ? h->B : 1, P = h ? h->max_P1 - 1 : 1;
        if (const int rc = check_strides(who, "g", gsb, B, gsn, N, gsp, P)) return rc;
    }
    ItemPlan pl;
    int rc = item_entry_begin(h, who.c_str(), ItemEntry::Scored, V, N, stream, [&]() {
        if (h->cls_image.empty()) return fail(MM_ERR_INVALID, who + ": no classes set (mm_batch_set_arc_classes)");
        if (U)
            if (const int rc = check_strides(who, "u", usb, h->B, usn, N, usc, h->cls_C)) return rc;
        if (xi)
            if (const int rc = check_strides(who, "x", xsb, h->B, xsn, N, xsc, h->cls_C)) return rc;
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    const int64_t cap = scored_class_cap(pl);
    if (h->cls_C > cap || h->sc_image.empty())
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->cls_C) + " classes exceed the cap of " + std::to_string(cap) +
                                            " classes whose score rows fit the LDS beside the kernel's plan (mm_batch_score_class_cap)");
    rc = ensure_class_plan(h, stream);
    if (!rc) rc = ensure_score_planes(h, stream);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    const bool tg = h->cls_max_M > scored_term_cap(pl, h->cls_C);
    ScoredParams sp{};
    sp.cls = static_cast<const ClassDev *>(h->d_cls.get());
    sp.sc = static_cast<const ScoredDev *>(h->d_sc.get());
    sp.U = U;
    sp.usb = usb;
    sp.usn = usn;
    sp.usc = usc;
    sp.C = h->cls_C;
    sp.urow = mm_scored_urow(h->cls_C);
    sp.terms = reinterpret_cast<float *>(static_cast<char *>(h->ws) + W.terms);
    sp.terms_global = tg ? 1 : 0;
    sp.xi = xi;
    sp.xsb = xsb;
    sp.xsn = xsn;
    sp.xsc = xsc;
    sp.ttl = ttl;
    return mm_launch_scored(h->B, pl.NW, pl.NI, pl.global, scored_lds_bytes(pl, h->cls_C), tg ? 0 : size_t(h->cls_max_M) * 2 * sizeof(float), p, sp,
                            static_cast<hipStream_t>(stream));
}

// ---- expected arc-class cost and its gradient (mm_kernel_classcost.hip)
int mm_batch_cost_class_cap(mm_batch_t h, int64_t *cap) {
    if (!h || !cap) return fail(MM_ERR_INVALID, "mm_batch_cost_class_cap: NULL argument");
    if (h->semiring != MM_LOG) return fail(MM_ERR_UNSUPPORTED, "mm_batch_cost_class_cap: log-semiring batches only");
    *cap = classcost_class_cap(item_plan(h, ItemEntry::ClassCost));
    return MM_OK;
}

int mm_classcost_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *A, int64_t asb,
                     int64_t asn, int64_t asc, const float *D, int64_t dsb, int64_t dsn, float *risk, float *grad, float *gamma, int64_t gsb,
                     int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    const std::string who = "mm_classcost_f32";
    ItemPlan pl;
    int rc = item_entry_begin(h, who.c_str(), ItemEntry::ClassCost, V, N, stream, [&]() {
        if (!A || !risk || !grad) return fail(MM_ERR_INVALID, who + ": A / risk / grad is NULL");
        if (h->cls_image.empty()) return fail(MM_ERR_INVALID, who + ": no classes set (mm_batch_set_arc_classes)");
        const int64_t P = h->max_P1 - 1;
        if (const int rc = check_strides(who, "a", asb, h->B, asn, N, asc, h->cls_C)) return rc;
        if (D && dsn < P) return fail(MM_ERR_DIM, who + ": d_stride_n " + std::to_string(dsn) + " < " + std::to_string(P) + " pdfs");
        if (const int rc = check_strides(who, "g", gsb, h->B, gsn, N, gsp, P)) return rc;
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    const int64_t cap = classcost_class_cap(pl);
    if (h->cls_C > cap || h->sc_image.empty())
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->cls_C) + " classes exceed the cap of " + std::to_string(cap) +
                                            " classes whose cost rows fit the LDS beside the kernel's plan (mm_batch_cost_class_cap)");
    // (the refusal of ensure_score_planes, in this entry's name)
    if (!h->d_sc && capturing(stream))
        return fail(MM_ERR_INVALID, "the class planes of this batch are not on the device yet: run " + who + " once outside a stream capture");
    rc = ensure_score_planes(h, stream);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    char *ws = static_cast<char *>(h->ws);
    ClassCostParams cp{};
    cp.sc = static_cast<const ScoredDev *>(h->d_sc.get());
    cp.A = A;
    cp.asb = asb;
    cp.asn = asn;
    cp.asc = asc;
    cp.C = h->cls_C;
    cp.urow = mm_scored_urow(h->cls_C);
    cp.D = D;
    cp.dsb = dsb;
    cp.dsn = dsn;
    cp.risk = risk;
    cp.grad = grad;
    cp.gamma = gamma;
    cp.gsb = gsb;
    cp.gsn = gsn;
    cp.gsp = gsp;
    cp.ttl = ttl;
    cp.ws_r = reinterpret_cast<float *>(ws + W.r);
    cp.ws_o = reinterpret_cast<double *>(ws + W.o);
    if (pl.global) {
        cp.ws_big = reinterpret_cast<float *>(ws + W.big);
        cp.big_stride = 8ll * h->max_S1p;
    }
    return mm_launch_classcost(h->B, pl.NW, pl.NI, pl.global, classcost_lds_bytes(pl, h->cls_C), p, cp, static_cast<hipStream_t>(stream));
}

// ---- pdf posteriors of the leaky HMM (mm_kernel_leaky.hip)
// rho(j) = (+)_k alpha_hat(k) T_hat(k, j) over the rows of T_hat' (the phony final column included), summed in double
static std::vector<float> pack_leak_rows(const mm_fsm_s &f) {
    const Csr &m = f.mat[0];  // row j: the arcs into j
    const float NINF = -std::numeric_limits<float>::infinity();
    std::vector<float> rho(size_t(f.S1), NINF);
    for (int64_t j = 0; j < f.S1; ++j) {
        double mx = -std::numeric_limits<double>::infinity();
        for (int64_t k = m.rowptr[size_t(j)]; k < m.rowptr[size_t(j) + 1]; ++k)
            mx = std::max(mx, double(m.val[size_t(k)]) + double(f.init[size_t(m.col[size_t(k)])]));
        if (!(mx > -std::numeric_limits<double>::infinity())) continue;
        double sum = 0.0;
        for (int64_t k = m.rowptr[size_t(j)]; k < m.rowptr[size_t(j) + 1]; ++k)
            sum += std::exp2(double(m.val[size_t(k)]) + double(f.init[size_t(m.col[size_t(k)])]) - mx);
        rho[size_t(j)] = float(mx + std::log2(sum));
    }
    return rho;
}
// ... and, with them, the batch's global vectors where only this entry's LDS plan (5 floats per state against the item kernel's 4)
// asks for them: mm_batch_create allocates h->ws_big for the other entries' plans alone, so a batch that never calls this entry
// holds what it held
static int ensure_leak_rows(mm_batch_t h, const ItemPlan &pl, void *stream) {
    if (pl.global && !h->ws_big) {
        if (capturing(stream))
            return fail(MM_ERR_INVALID, "the global vectors of this batch are not on the device yet: run mm_leakyposteriors_f32 once outside a stream capture");
        if (hipMalloc(&h->ws_big, size_t(h->B) * 4 * size_t(h->max_S1p) * sizeof(float)) != hipSuccess) {
            h->ws_big = nullptr;
            return fail(MM_ERR_HIP, "mm_leakyposteriors_f32: device allocation failed");
        }
    }
    return ensure_derived_forms<LeakDev>(
        h, stream, "leak", "mm_leakyposteriors_f32", h->d_leak, &mm_fsm_s::leak_blob, [](mm_fsm_t f, Blob &bl) { (void)bl.add(pack_leak_rows(*f)); },
        [](mm_fsm_t f) { return LeakDev{static_cast<const float *>(f->leak_blob.get())}; });
}

int mm_leakyposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, float leak, float *gamma,
                           int64_t gsb, int64_t gsn, int64_t gsp, float *ttl, void *stream) {
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_leakyposteriors_f32", ItemEntry::Leaky, V, N, stream, [&]() {
        if (!gamma || !ttl) return fail(MM_ERR_INVALID, "mm_leakyposteriors_f32: gamma / ttl is NULL");
        if (!(leak >= 0.f) || !std::isfinite(leak)) return fail(MM_ERR_INVALID, "mm_leakyposteriors_f32: the leak coefficient must be finite and >= 0");
        const int64_t P = h->max_P1 - 1;
        if (const int rc = check_strides("mm_leakyposteriors_f32", "g", gsb, h->B, gsn, N, gsp, P)) return rc;
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    rc = ensure_leak_rows(h, pl, stream);
    if (rc) return rc;
    const ItemWs W = item_ws_layout(h, pl, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, W, p, stream);
    if (rc) return rc;
    p.gamma = gamma;
    p.gsb = gsb;
    p.gsn = gsn;
    p.gsp = gsp;
    p.ttl = ttl;
    LeakParams lp{};
    lp.rows = static_cast<const LeakDev *>(h->d_leak.get());
    lp.leps2 = leak > 0.f ? std::log2(leak) : -std::numeric_limits<float>::infinity();
    return mm_launch_leaky(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, p, lp, static_cast<hipStream_t>(stream));
}

// ---- posterior path sampling (mm_kernel_sample.hip)
// T_hat' by destination over the real states plus the omega column as lists of SampleRec (source, log2 weight, the source's own
// list), parallel entries of one (source, destination) merged by log-add -- the draw and the reported probability are over STATE
// sequences; *fin_start, *fin_deg: the list of the phony final state
static std::vector<SampleRec> pack_sample_recs(const mm_fsm_s &f, int *fin_start, int *fin_deg) {
    const Csr &m = f.mat[0];  // row j: the arcs into j, sources ascending
    const int64_t S1 = f.S1, fin = S1 - 1;
    const float NINF = -std::numeric_limits<float>::infinity();
    std::vector<int32_t> start(size_t(S1) + 1, 0);
    std::vector<SampleRec> recs;
    recs.reserve(size_t(f.nnz));
    for (int64_t j = 0; j < S1; ++j) {
        start[size_t(j)] = int32_t(recs.size());
        for (int64_t k = m.rowptr[size_t(j)]; k < m.rowptr[size_t(j) + 1];) {
            const int32_t i = m.col[size_t(k)];
            double mx = -std::numeric_limits<double>::infinity(), sum = 0.0;
            int64_t e = k;
            for (; e < m.rowptr[size_t(j) + 1] && m.col[size_t(e)] == i; ++e) mx = std::max(mx, double(m.val[size_t(e)]));
            for (int64_t q = k; q < e; ++q)
                if (m.val[size_t(q)] > NINF) sum += std::exp2(double(m.val[size_t(q)]) - mx);
            // (the phony final state is never a source: its self-loop is not part of any path of len_b frames)
            if (sum > 0.0 && i != fin) recs.push_back(SampleRec{i, float(mx + std::log2(sum)), 0, 0});
            k = e;
        }
    }
    start[size_t(S1)] = int32_t(recs.size());
    for (SampleRec &r : recs) {
        r.start = start[size_t(r.src)];
        r.deg = start[size_t(r.src) + 1] - r.start;
    }
    *fin_start = start[size_t(fin)];
    *fin_deg = start[size_t(S1)] - start[size_t(fin)];
    return recs;
}
// The sampling forms: per FSM its SampleRec lists, per utterance a SampleDev.
static int ensure_sample_forms(mm_batch_t h, void *stream) {
    return ensure_derived_forms<SampleDev>(
        h, stream, "sampling", "mm_samplepaths_f32", h->d_samp, &mm_fsm_s::samp_blob,
        [](mm_fsm_t f, Blob &bl) { (void)bl.add(pack_sample_recs(*f, &f->samp_fin_start, &f->samp_fin_deg)); },  // (at 0)
        [](mm_fsm_t f) { return SampleDev{static_cast<const SampleRec *>(f->samp_blob.get()), f->samp_fin_start, f->samp_fin_deg}; });
}

int mm_samplepaths_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, int64_t nsamples, int64_t seed,
                       int32_t *paths, int64_t psb, int64_t psk, float *logprob, int64_t lsb, float *ttl, void *stream) {
    ItemPlan pl;
    int rc = item_entry_begin(h, "mm_samplepaths_f32", ItemEntry::Sample, V, N, stream, [&]() {
        if (!paths) return fail(MM_ERR_INVALID, "mm_samplepaths_f32: paths is NULL");
        if (nsamples < 1) return fail(MM_ERR_INVALID, "mm_samplepaths_f32: nsamples " + std::to_string(nsamples) + " < 1");
        if (nsamples > INT32_MAX) return fail(MM_ERR_UNSUPPORTED, "mm_samplepaths_f32: more than 2^31 - 1 samples");
        if (psk < N) return fail(MM_ERR_DIM, "mm_samplepaths_f32: path_stride_k " + std::to_string(psk) + " < N = " + std::to_string(N));
        if (psb / nsamples < psk)
            return fail(MM_ERR_DIM, "mm_samplepaths_f32: path_stride_b " + std::to_string(psb) + " < nsamples * path_stride_k");
        if (logprob && lsb < nsamples) return fail(MM_ERR_DIM, "mm_samplepaths_f32: lp_stride_b " + std::to_string(lsb) + " < nsamples = " + std::to_string(nsamples));
        return int(MM_OK);
    }, &pl);
    if (rc) return rc;
    rc = ensure_sample_forms(h, stream);
    if (rc) return rc;
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    rc = item_ws_bind(h, pl, item_ws_layout(h, pl, N), p, stream);
    if (rc) return rc;
    SampleParams sp{};
    sp.forms = static_cast<const SampleDev *>(h->d_samp.get());
    sp.paths = paths;
    sp.psb = psb;
    sp.psk = psk;
    sp.logprob = logprob;
    sp.lsb = lsb;
    sp.ttl = ttl;
    sp.K = int(nsamples);
    sp.key0 = unsigned(uint64_t(seed));
    sp.key1 = unsigned(uint64_t(seed) >> 32);
    return mm_launch_sample(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, pl.stage, h->max_S1p, h->n_cus, p, sp, static_cast<hipStream_t>(stream));
}

// alpha / beta export on the pair kernels (mm_pairs_tu.hip: mm_fbx_kernel + mm_pair_export_kernel): one shared graph in the pair
// form whose every state takes part (the packer drops states that cannot be reached or cannot reach the final state -- their
// posteriors are zero, their alpha / beta are not), log semiring, up to 250 pdfs
static bool export_on_pairs(mm_batch_t h, int dir) {
    if (!on_pairs(h)) return false;
    if (!(h->pair_H == 1 ? mm_pair_export_fits(pair_launch_of(h)) : mm_split_export_fits(pair_launch_of(h)))) return false;
    return h->fsms[0]->export_ok[dir];
}

static int run_export(mm_batch_t h, int mode, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                      float *out, int64_t out_stride_n, void *stream) {
    const char *who = mode == MODE_ALPHA ? "mm_alpharecursion_f32" : "mm_betarecursion_f32";
    int rc = check_run(h, who, V, N, -1);
    if (rc) return rc;
    if (!out) return fail(MM_ERR_INVALID, std::string(who) + ": out is NULL");
    if (out_stride_n < h->total_states) return fail(MM_ERR_DIM, std::string(who) + ": out_stride_n < total states");
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    p.out = out;
    p.out_stride_n = out_stride_n;
    // (inputs whose vectors leave float32's range in most utterances -- the reference's WSJ denominator in the forward direction: its
    // initial-context states decay 2 log2 per frame against the rest, and the reference's alpha holds them as finite logarithms -- go
    // straight to the item kernel while the last finished export of the direction marked more than half of its utterances (read from
    // pinned host memory without synchronising, like the exact policy of mm_pdfposteriors_f32); every 32nd call tries again)
    bool linear_first = export_on_pairs(h, mode == MODE_ALPHA ? 0 : 1);
    // (mm_batch_set_exact_policy pins this choice too: F32_FIRST = always the linear-domain kernels first, F64_FIRST = always the item
    // kernel alone -- with a fixed policy the launches of a call, and the last bits of its result, are a function of the call)
    if (linear_first && h->exact_first == 1) linear_first = false;
    else if (linear_first && h->stat_host && h->exact_first < 0) {
        const int dirx = mode == MODE_ALPHA ? 0 : 1;
        const bool probe = (++h->export_calls[dirx] & 31u) == 0u;
        if (!capturing(stream) && !probe && 2 * int64_t(h->stat_host[2 + dirx]) > h->B) linear_first = false;
    }
    if (linear_first) {
        // phase A of ONE direction over all N + 1 frames with two utterances per workgroup (linear domain, float32), the layout
        // pass, then -- for the utterances whose values left float32's range (marked; sharp emissions) -- the item kernel
        const WsLayout L = ws_layout(h, N);
        rc = ensure_ws(h, L.total, stream);
        if (rc) return rc;
        char *const ws = static_cast<char *>(h->ws);
        p.ws_alpha = reinterpret_cast<float *>(ws + L.alpha);
        p.ws_c = reinterpret_cast<double *>(ws + L.c);
        p.redo = reinterpret_cast<int *>(ws + L.redo);
        p.pair_s1p = h->pair_H > 1 ? h->split_s1p : h->max_S1p;
        p.pair_hand = ws + L.hand;
        p.pair_zmin = reinterpret_cast<double *>(ws + L.zmin);
        p.split_q10 = 512;
        p.lt_floor = h->lt_floor;
        p.x_sleep = h->dbg.x_sleep;
        p.x_timeout = x_timeout(N);
        hipLaunchKernelGGL(mm_prologue_kernel, dim3(unsigned((h->B + 1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           (const int *)nullptr, int(h->B), int(N), (int *)nullptr, p.redo, (int *)nullptr, 0);
        HIP_TRY(hipGetLastError());
        if (h->pair_H > 1) {  // the teams' exchange areas (the float32 team kernels': phase A's rows), zeroed like before a pdfposteriors call
            rc = bind_team_x(h, p, ws, L, false, stream);
            if (rc) return rc;
            rc = mm_launch_split_export(pair_launch_of(h), p, mode == MODE_ALPHA ? 0 : 1, static_cast<hipStream_t>(stream));
        } else {
            rc = mm_launch_pair_export(pair_launch_of(h), p, mode == MODE_ALPHA ? 0 : 1, static_cast<hipStream_t>(stream));
        }
        if (rc) return rc;
        if (h->stat_host) {  // how many utterances were marked: what the next export of this direction starts with
            hipLaunchKernelGGL(mm_count_marks_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), p.redo, int(h->B),
                               const_cast<int *>(h->stat_host) + 2 + (mode == MODE_ALPHA ? 0 : 1));
            HIP_TRY(hipGetLastError());
        }
        h->last_redo = p.redo;  // (mm_batch_last_redo_count: how many utterances the item kernel computed instead)
        if (h->dbg.no_redo) return MM_OK;
        p.ws_alpha = nullptr;   // (the item kernel's export modes keep nothing in the workspace)
        p.ws_c = nullptr;
        return mode == MODE_ALPHA ? launch_log<MODE_ALPHA>(h, p, stream) : launch_log<MODE_BETA>(h, p, stream);
    }
    if (h->semiring == MM_TROPICAL) {
        if (mode == MODE_ALPHA) return launch_tropical(h, p, stream);
        const ItemPlan g = item_plan(h, ItemEntry::Export);
        if (g.NI == 0) return launch(mm_log_kernel<MODE_BETA, 0, 0, true, false>, mm_log_kernel<MODE_BETA, 0, 0, true, true>, h, p, g.e, g.NW, stream);
        return launch(mm_log_kernel<MODE_BETA, 8, 0, true, false>, mm_log_kernel<MODE_BETA, 8, 0, true, true>, h, p, g.e, g.NW, stream);
    }
    if (mode == MODE_ALPHA) return launch_log<MODE_ALPHA>(h, p, stream);
    return launch_log<MODE_BETA>(h, p, stream);
}

int mm_alpharecursion_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                          float *out, int64_t out_stride_n, void *stream) {
    return run_export(h, MODE_ALPHA, V, vsb, vsn, lens, N, out, out_stride_n, stream);
}

int mm_betarecursion_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                         float *out, int64_t out_stride_n, void *stream) {
    return run_export(h, MODE_BETA, V, vsb, vsn, lens, N, out, out_stride_n, stream);
}

int mm_maxstateposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                              float *out, int64_t out_stride_n, void *stream) {
    int rc = check_run(h, "mm_maxstateposteriors_f32", V, N, MM_TROPICAL);
    if (rc) return rc;
    if (!out) return fail(MM_ERR_INVALID, "mm_maxstateposteriors_f32: out is NULL");
    if (out_stride_n < h->total_states) return fail(MM_ERR_DIM, "mm_maxstateposteriors_f32: out_stride_n < total states");
    // tropical alpha into `out`, tropical beta into the workspace, then mu = alpha (*) beta (/) best in place
    const size_t beta_bytes = align_up(size_t(h->total_states) * size_t(N + 1) * 4, 256);
    rc = ensure_ws(h, beta_bytes + align_up(size_t(h->B) * 4, 256), stream);
    if (rc) return rc;
    float *beta = static_cast<float *>(h->ws);
    float *best = reinterpret_cast<float *>(static_cast<char *>(h->ws) + beta_bytes);
    rc = run_export(h, MODE_ALPHA, V, vsb, vsn, lens, N, out, out_stride_n, stream);
    if (rc) return rc;
    rc = run_export(h, MODE_BETA, V, vsb, vsn, lens, N, beta, h->total_states, stream);
    if (rc) return rc;
    const int bt = 64;
    hipLaunchKernelGGL(mm_pick_final_kernel, dim3(unsigned((h->B + bt - 1) / bt)), dim3(bt), 0, static_cast<hipStream_t>(stream),
                       h->d_utts, int(h->B), out, (long long)out_stride_n, int(N), best);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mm_maxmarginal_kernel, dim3(unsigned(h->B), unsigned(N + 1)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       h->d_utts, out, (long long)out_stride_n, beta, (long long)h->total_states, best);
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

// ---- RCCL (resolved at run time: the communicator belongs to the RCCL of the calling process) ----
namespace {
typedef int (*nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
enum { MM_NCCL_SUM = 0, MM_NCCL_FLOAT32 = 7, MM_NCCL_FLOAT64 = 8 };  // rccl.h: ncclSum, ncclFloat32, ncclFloat64
// The RCCL the caller's communicators belong to: handed over with mm_set_rccl (a dlopen handle), else whatever the
// process exposes globally.  The library never opens an RCCL of its own: an ncclComm_t made by one build of RCCL passed
// to another is undefined behaviour.
void *g_rccl_handle = nullptr;
std::mutex g_rccl_lock;
void *rccl_symbol(const char *name) {
    std::lock_guard<std::mutex> guard(g_rccl_lock);
    if (g_rccl_handle)
        if (void *f = dlsym(g_rccl_handle, name)) return f;
    return dlsym(RTLD_DEFAULT, name);
}
__global__ void mm_sum_f64_kernel(const float *x, long long n, double *out) {
    __shared__ double part[16];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) s += (double)x[i];
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (unsigned w = 0; w < blockDim.x / 64; ++w) t += part[w];  // (fixed order: the same sum on every run)
        *out = t;
    }
}
}  // namespace

int mm_set_rccl(void *dl_handle) {
    std::lock_guard<std::mutex> guard(g_rccl_lock);
    g_rccl_handle = dl_handle;
    return MM_OK;
}

int mm_allreduce_logz(void *comm, const float *ttl, int64_t B_local, double *sum, void *stream) {
    if (!comm || !sum || B_local < 0 || (B_local > 0 && !ttl)) return fail(MM_ERR_INVALID, "mm_allreduce_logz: bad argument");
    const nccl_allreduce_fn allreduce = reinterpret_cast<nccl_allreduce_fn>(rccl_symbol("ncclAllReduce"));
    if (!allreduce) return fail(MM_ERR_UNSUPPORTED, "mm_allreduce_logz: RCCL is not visible in this process: call mm_set_rccl with the handle of the RCCL `comm` came from");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mm_sum_f64_kernel, dim3(1), dim3(1024), 0, st, ttl, (long long)B_local, sum);
    HIP_TRY(hipGetLastError());
    if (allreduce(sum, sum, 1, MM_NCCL_FLOAT64, MM_NCCL_SUM, comm, st) != 0) return fail(MM_ERR_HIP, "mm_allreduce_logz: ncclAllReduce failed");
    return MM_OK;
}

int mm_allgather_ttl(void *comm, const float *ttl, int64_t B_max, float *all, void *stream) {
    if (!comm || !ttl || !all || B_max < 1) return fail(MM_ERR_INVALID, "mm_allgather_ttl: bad argument");
    const nccl_allgather_fn allgather = reinterpret_cast<nccl_allgather_fn>(rccl_symbol("ncclAllGather"));
    if (!allgather) return fail(MM_ERR_UNSUPPORTED, "mm_allgather_ttl: RCCL is not visible in this process: call mm_set_rccl with the handle of the RCCL `comm` came from");
    if (allgather(ttl, all, size_t(B_max), MM_NCCL_FLOAT32, comm, static_cast<hipStream_t>(stream)) != 0)
        return fail(MM_ERR_HIP, "mm_allgather_ttl: ncclAllGather failed");
    return MM_OK;
}

int mm_totalsum_f32(mm_batch_t h, int64_t n, int cumulative, float *out, void *stream) {
    static const float dummy = 0.f;
    int rc = check_run(h, "mm_totalsum_f32", &dummy, n, -1);
    if (rc) return rc;
    if (!out) return fail(MM_ERR_INVALID, "mm_totalsum_f32: out is NULL");
    // v_k and the running total live in the extended system (src/fsm.jl:19-28): the final state's self
    // loop of weight one makes it the accumulator of omega . v_k; n + 1 frames of the alpha recursion
    rc = ensure_ws(h, align_up(size_t(h->total_states) * size_t(n + 1) * 4, 256), stream);
    if (rc) return rc;
    RunParams p{};
    p.utts = h->d_utts;
    p.N = int(n);
    p.B = int(h->B);
    p.out = static_cast<float *>(h->ws);
    p.out_stride_n = h->total_states;
    p.free_run = cumulative ? 2 : 1;
    rc = h->semiring == MM_TROPICAL ? launch_tropical(h, p, stream) : launch_log<MODE_ALPHA>(h, p, stream);
    if (rc) return rc;
    const int bt = 64;
    hipLaunchKernelGGL(mm_pick_final_kernel, dim3(unsigned((h->B + bt - 1) / bt)), dim3(bt), 0,
                       static_cast<hipStream_t>(stream), h->d_utts, int(h->B), p.out, p.out_stride_n, int(n), out);
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

int mm_viterbi_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N,
                   int32_t *path, int64_t path_stride_b, float *score, int32_t *bp, int64_t bp_stride_n,
                   void *stream) {
    int rc = check_run(h, "mm_viterbi_f32", V, N, MM_TROPICAL);
    if (rc) return rc;
    if (!path || !score) return fail(MM_ERR_INVALID, "mm_viterbi_f32: path/score is NULL");
    if (path_stride_b < N) return fail(MM_ERR_DIM, "mm_viterbi_f32: path_stride_b < N");
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    if (!bp) {
        // (int32 rows for the item kernel, or one-byte rows padded to 256 bytes for the row-lane kernels: what this batch runs)
        rc = ensure_ws(h, ws_vit_bytes(h, N), stream);
        if (rc) return rc;
        bp = static_cast<int32_t *>(h->ws);
        bp_stride_n = h->total_states;
        p.stop_at_len = 1;  // nobody reads the back-pointers of the frames beyond len_b + 1
    } else if (bp_stride_n < h->total_states) {
        return fail(MM_ERR_DIM, "mm_viterbi_f32: bp_stride_n < total states");
    }
    p.bp = bp;
    p.bp_stride_n = bp_stride_n;
    p.path = path;
    p.path_stride_b = path_stride_b;
    p.score = score;
    bind_stamps(h, p);
    if (h->vit_ok && p.stop_at_len) {  // (internal back-pointers: the compact form)
        const VitLaunch vl = vit_launch_of(h);
        RunParams q = p;
        q.bp_stride_n = vl.bp_row;
        return mm_launch_viterbi(vl, q, static_cast<hipStream_t>(stream));
    }
    rc = launch_tropical(h, p, stream);
    if (rc) return rc;
    const int bt = 64;
    hipLaunchKernelGGL(mm_backtrace_kernel, dim3(unsigned((h->B + bt - 1) / bt)), dim3(bt), 0,
                       static_cast<hipStream_t>(stream), p);
    HIP_TRY(hipGetLastError());
    return MM_OK;
}

// ---- windowed best paths: the Viterbi recursion of a window with a carried start and an open end (mm_kernel_vitwindow.hip)
int mm_viterbiwindow_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *state_in,
                         const int32_t *closed, const int32_t *commit, int commit_converged, float *state_out, float *mcommit,
                         int32_t *ncommit, int32_t *path, int64_t path_stride_b, float *score, int32_t *converged, void *stream) {
    // what the arguments alone show comes first, then the batch's refusals
    if (!path || !score) return fail(MM_ERR_INVALID, "mm_viterbiwindow_f32: path/score is NULL");
    if (path_stride_b < N) return fail(MM_ERR_DIM, "mm_viterbiwindow_f32: path_stride_b < N");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, std::string("mm_viterbiwindow_f32: tropical batches only (this batch is ") +
                                            (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, "mm_viterbiwindow_f32", V, N, MM_TROPICAL);
    if (!rc) rc = ensure_item_forms(h, stream);
    if (rc) return rc;
    const ItemPlan pl = item_plan(h, ItemEntry::VitWindow);
    rc = item_plan_check(h, pl);
    if (!rc) rc = ensure_ws(h, mm_batch_workspace_bytes(h, N), stream);
    if (rc) return rc;
    const VitWindowWs W = vitwindow_ws_layout(h, N);
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    bind_big(h, pl, p);
    if (h->ws_big) {  // (the trace kernel's flags of FSMs beyond its LDS)
        p.ws_big = h->ws_big;
        p.big_stride = 4ll * h->max_S1p;
    }
    p.path = path;
    p.path_stride_b = path_stride_b;
    p.score = score;
    VitWindowParams wp{};
    wp.state_in = state_in;
    wp.state_out = state_out;
    wp.closed = closed;
    wp.commit = commit;
    wp.commit_converged = commit_converged;
    wp.mcommit = mcommit;
    wp.ncommit = ncommit;
    wp.converged = converged;
    char *ws = static_cast<char *>(h->ws);
    wp.ws_bp = reinterpret_cast<int *>(ws);
    wp.ws_best = reinterpret_cast<float *>(ws + W.best);
    wp.ws_m = reinterpret_cast<float *>(ws + W.m);
    wp.ws_end = reinterpret_cast<int *>(ws + W.end);
    return mm_launch_vitwindow(h->B, pl.NW, pl.NI, pl.global, pl.lds_bytes, h->max_S1p, p, wp, static_cast<hipStream_t>(stream));
}

// ---- best paths with arc classes under per-frame arc-class scores (mm_kernel_classpath.hip)
// The plan of a tropical batch: the 16-bit class plane of the forward item form of every distinct (FSM, class array), in the
// batch's sc_image / d_sc / cls_C (mm_batch_set_arc_classes, which fills them for log batches, refuses tropical ones).
int mm_batch_set_path_classes(mm_batch_t h, const int32_t *cls, const int64_t *offsets, int32_t C) {
    const std::string who = "mm_batch_set_path_classes";
    if (!h || !cls) return fail(MM_ERR_INVALID, who + ": NULL argument");
    if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only");
    if (const int rc = check_class_args(who, h, cls, offsets, C)) return rc;
    if (C > 65534) return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(C) + " classes exceed the 65534 a 16-bit class id holds");
    const size_t B = size_t(h->B);
    return no_throw(who.c_str(), [&]() {
        struct Made { const mm_fsm_s *f; const int32_t *cls; MadePlanes mp; };
        std::vector<Made> made;
        std::vector<ScoredDev> sdescs(B);
        Blob sbl;
        (void)sbl.add(sdescs);  // (at 0; filled in below)
        for (size_t b = 0; b < B; ++b) {
            mm_fsm_s &f = *h->fsms[b];
            const int32_t *cb = cls + (offsets ? offsets[b] : 0);
            const Made *m = nullptr;
            for (const Made &c : made)
                if (c.f == &f && (c.cls == cb || std::equal(cb, cb + f.nnz, c.cls))) m = &c;
            if (!m) {
                ensure_packed(&f);
                made.push_back(Made{&f, cb, add_class_planes(sbl, f, cb, C, nullptr)});
                m = &made.back();
            }
            ScoredDev &sd = sdescs[b];
            sd.plane[0] = reinterpret_cast<const unsigned short *>(m->mp.o_plane[0]);
            sd.plane[1] = reinterpret_cast<const unsigned short *>(m->mp.o_plane[1]);
            sd.rcls = reinterpret_cast<const unsigned short *>(m->mp.o_rcls);
        }
        memcpy(sbl.host.data(), sdescs.data(), sizeof(ScoredDev) * B);
        h->sc_image = std::move(sbl.host);
        h->d_sc = DevMem();  // (the next mm_classpath_f32 call uploads the new planes)
        h->cls_C = C;
        return int(MM_OK);
    });
}

int mm_batch_path_class_info(mm_batch_t h, int32_t *C, int64_t *cap) {
    if (!h) return fail(MM_ERR_INVALID, "mm_batch_path_class_info: NULL batch");
    if (h->semiring != MM_TROPICAL) return fail(MM_ERR_UNSUPPORTED, "mm_batch_path_class_info: tropical batches only");
    if (C) *C = h->sc_image.empty() ? 0 : h->cls_C;
    if (cap) *cap = classpath_class_cap(item_plan(h, ItemEntry::ClassPath));
    return MM_OK;
}

int mm_classpath_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *U, int64_t usb,
                     int64_t usn, int64_t usc, int32_t *path, int64_t path_stride_b, int32_t *classes, int64_t classes_stride_b, float *score,
                     void *stream) {
    const std::string who = "mm_classpath_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!path || !score) return fail(MM_ERR_INVALID, who + ": path/score is NULL");
    if (path_stride_b < N) return fail(MM_ERR_DIM, who + ": path_stride_b < N");
    if (classes && classes_stride_b < N) return fail(MM_ERR_DIM, who + ": classes_stride_b < N");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    const bool planned = !h->sc_image.empty();
    if ((U || classes) && !planned) return fail(MM_ERR_INVALID, who + ": no classes set (mm_batch_set_path_classes)");
    if (U)
        if ((rc = check_strides(who, "u", usb, h->B, usn, N, usc, h->cls_C))) return rc;
    rc = ensure_item_forms(h, stream);
    if (rc) return rc;
    const ItemPlan pl = item_plan(h, ItemEntry::ClassPath);
    const int64_t cap = classpath_class_cap(pl);
    if (U && h->cls_C > cap)
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->cls_C) + " classes exceed the cap of " + std::to_string(cap) +
                                            " classes whose score rows fit the LDS beside the kernel's plan (mm_batch_path_class_info)");
    if (pl.global && !h->ws_big) {  // (mm_batch_create allocates them for the other entries' plans alone, as ensure_weight_forms)
        if (capturing(stream))
            return fail(MM_ERR_INVALID, "the global vectors of this batch are not on the device yet: run " + who + " once outside a stream capture");
        if (hipMalloc(&h->ws_big, size_t(h->B) * 4 * size_t(h->max_S1p) * sizeof(float)) != hipSuccess) {
            h->ws_big = nullptr;
            return fail(MM_ERR_HIP, who + ": device allocation failed");
        }
    }
    rc = item_plan_check(h, pl);
    if (!rc && planned) rc = ensure_score_planes(h, stream, who.c_str());
    const ClassPathWs W = classpath_ws_layout(h, N, pl.global);
    if (!rc) rc = ensure_ws(h, std::max(W.total, mm_batch_workspace_bytes(h, N)), stream);
    if (rc) return rc;
    RunParams p = run_params(h, V, vsb, vsn, lens, N);
    bind_big(h, pl, p);
    p.path = path;
    p.path_stride_b = path_stride_b;
    p.score = score;
    ClassPathParams cp{};
    cp.sc = planned ? static_cast<const ScoredDev *>(h->d_sc.get()) : nullptr;
    cp.U = U;
    cp.usb = usb;
    cp.usn = usn;
    cp.usc = usc;
    cp.C = planned ? h->cls_C : 0;
    cp.urow = mm_scored_urow(cp.C);
    cp.classes = classes;
    cp.csb = classes_stride_b;
    char *ws = static_cast<char *>(h->ws);
    cp.ws_bp = reinterpret_cast<int *>(ws);
    cp.ws_bc = reinterpret_cast<unsigned short *>(ws + W.bc);
    cp.ws_cbuf = reinterpret_cast<unsigned short *>(ws + W.cbuf);
    cp.cbuf_stride = 2ll * h->max_S1p;
    // (a plan without scores and without classes asked for: the plain step)
    const int mode = U ? 2 : (classes ? 1 : 0);
    return mm_launch_classpath(h->B, pl.NW, pl.NI, pl.global, mode, classpath_lds_bytes(pl, cp.C, U != nullptr), p, cp, static_cast<hipStream_t>(stream));
}

// ---- beam-pruned best-path lattices (mm_kernel_lattice.hip)
// The arc table of a tropical batch: the entries of every distinct FSM in the caller's order as three planes -- source (the phony
// self-loop: -1), destination, weight --, from T_hat by source (mat[1]) and the caller's entry behind each of its entries
// (bwd_caller); the utterances' LatticeDev descriptors in front.  One allocation, one copy, made by the first call -- never during a
// capture (as ensure_score_planes).
static int ensure_lattice_arcs(mm_batch_t h, void *stream) {
    if (h->d_lat) return MM_OK;
    if (capturing(stream))
        return fail(MM_ERR_INVALID, "the arc table of this batch is not on the device yet: run mm_lattice_f32 once outside a stream capture");
    return no_throw("mm_lattice_f32", [&]() {
        const size_t B = size_t(h->B);
        struct Made { const mm_fsm_s *f; size_t o_src, o_dst, o_w; };
        std::vector<Made> made;
        std::vector<LatticeDev> descs(B);
        Blob bl;
        (void)bl.add(descs);  // (at 0; filled in below)
        for (size_t b = 0; b < B; ++b) {
            const mm_fsm_s &f = *h->fsms[b];
            if (f.nnz > int64_t(INT32_MAX) - 4096) return fail(MM_ERR_UNSUPPORTED, "mm_lattice_f32: more stored entries than a 32-bit entry index holds");
            const Made *m = nullptr;
            for (const Made &c : made)
                if (c.f == &f) m = &c;
            if (!m) {
                std::vector<int32_t> src(size_t(f.nnz)), dst(size_t(f.nnz));
                std::vector<float> w(size_t(f.nnz));
                const Csr &bwd = f.mat[1];
                for (int64_t i = 0; i < f.S1; ++i)
                    for (int64_t a = bwd.rowptr[size_t(i)]; a < bwd.rowptr[size_t(i) + 1]; ++a) {
                        const size_t k = size_t(f.bwd_caller[size_t(a)]);
                        const int32_t j = bwd.col[size_t(a)];
                        src[k] = (i == f.S1 - 1 && j == f.S1 - 1) ? -1 : int32_t(i);
                        dst[k] = j;
                        w[k] = bwd.val[size_t(a)];
                    }
                const size_t o_src = bl.add(src), o_dst = bl.add(dst);
                made.push_back(Made{&f, o_src, o_dst, bl.add(w)});
                m = &made.back();
            }
            descs[b] = LatticeDev{reinterpret_cast<const int *>(m->o_src), reinterpret_cast<const int *>(m->o_dst), reinterpret_cast<const float *>(m->o_w), int(f.nnz), 0};
        }
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, bl.host.size()));
        DevMem own(d);
        for (LatticeDev &ld : descs) {  // (offsets into the image until here)
            ld.src = reinterpret_cast<const int *>(static_cast<char *>(d) + reinterpret_cast<size_t>(ld.src));
            ld.dst = reinterpret_cast<const int *>(static_cast<char *>(d) + reinterpret_cast<size_t>(ld.dst));
            ld.w = reinterpret_cast<const float *>(static_cast<char *>(d) + reinterpret_cast<size_t>(ld.w));
        }
        memcpy(bl.host.data(), descs.data(), sizeof(LatticeDev) * B);
        if (hipMemcpy(d, bl.host.data(), bl.host.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(MM_ERR_HIP, "mm_lattice_f32: upload of the arc table failed");
        h->d_lat = std::move(own);
        return int(MM_OK);
    });
}

// Where mm_lattice_f32 keeps what it keeps in h->ws for N frames: the tropical alpha and beta rows ((sum_b S1_b) x (N + 1) floats
// each, the export layout), the int64 offsets [B * N + 1] and best [B]
struct LatticeWs { size_t beta = 0, offs = 0, best = 0, total = 0; };
static LatticeWs lattice_ws_layout(mm_batch_t h, int64_t N) {
    LatticeWs W;
    W.beta = align_up(size_t(h->total_states) * size_t(N + 1) * 4, 256);
    W.offs = 2 * W.beta;
    W.best = W.offs + align_up((size_t(h->B) * size_t(N) + 1) * 8, 256);
    W.total = W.best + align_up(size_t(h->B) * 4, 256);
    return W;
}

int mm_lattice_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const float *beam, int32_t *counts,
                   int64_t counts_stride_b, int64_t *total, float *best, int32_t *arc, float *score, int64_t cap, void *stream) {
    const std::string who = "mm_lattice_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!beam || !counts || !total) return fail(MM_ERR_INVALID, who + ": beam/counts/total is NULL");
    if (counts_stride_b < N) return fail(MM_ERR_DIM, who + ": counts_stride_b < N");
    if ((arc == nullptr) != (score == nullptr)) return fail(MM_ERR_INVALID, who + ": arc and score are both given or both NULL");
    if (cap < 0 || (!arc && cap != 0)) return fail(MM_ERR_INVALID, who + ": cap must be >= 0, and 0 with arc NULL (the count-only call)");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    if (h->B * N > int64_t(INT32_MAX)) return fail(MM_ERR_UNSUPPORTED, who + ": B * N exceeds 2^31 - 1 workgroups");
    rc = ensure_item_forms(h, stream);
    if (!rc) rc = ensure_lattice_arcs(h, stream);
    const LatticeWs W = lattice_ws_layout(h, N);
    if (!rc) rc = ensure_ws(h, std::max(W.total, mm_batch_workspace_bytes(h, N)), stream);
    if (rc) return rc;
    char *const ws = static_cast<char *>(h->ws);
    float *const alpha = reinterpret_cast<float *>(ws), *const beta = reinterpret_cast<float *>(ws + W.beta);
    float *const bestw = reinterpret_cast<float *>(ws + W.best);
    // the two recursions as mm_maxstateposteriors_f32 runs them, then best = alpha_{N+1}(f)
    rc = run_export(h, MODE_ALPHA, V, vsb, vsn, lens, N, alpha, h->total_states, stream);
    if (rc) return rc;
    rc = run_export(h, MODE_BETA, V, vsb, vsn, lens, N, beta, h->total_states, stream);
    if (rc) return rc;
    const int bt = 64;
    hipLaunchKernelGGL(mm_pick_final_kernel, dim3(unsigned((h->B + bt - 1) / bt)), dim3(bt), 0, static_cast<hipStream_t>(stream), h->d_utts, int(h->B),
                       alpha, (long long)h->total_states, int(N), bestw);
    HIP_TRY(hipGetLastError());
    if (best) {
        hipLaunchKernelGGL(mm_pick_final_kernel, dim3(unsigned((h->B + bt - 1) / bt)), dim3(bt), 0, static_cast<hipStream_t>(stream), h->d_utts,
                           int(h->B), alpha, (long long)h->total_states, int(N), best);
        HIP_TRY(hipGetLastError());
    }
    const RunParams p = run_params(h, V, vsb, vsn, lens, N);
    LatticeParams lp{};
    lp.arcs = static_cast<const LatticeDev *>(h->d_lat.get());
    lp.alpha = alpha;
    lp.beta = beta;
    lp.row_stride = h->total_states;
    lp.beam = beam;
    lp.best = bestw;
    lp.counts = counts;
    lp.csb = counts_stride_b;
    lp.offs = reinterpret_cast<long long *>(ws + W.offs);
    lp.arc = arc;
    lp.score = score;
    lp.cap = cap;
    return mm_launch_lattice(h->B, lattice_global(h), h->max_S1p, p, lp, reinterpret_cast<long long *>(total), static_cast<hipStream_t>(stream));
}

// ---- lattice posteriors (mm_kernel_latpost.hip): the log-semiring forward-backward over the records of a lattice
int mm_latticeposteriors_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const int64_t *offsets,
                             const int32_t *arc, int64_t nrec, const float *extra, float *post, float *logz, float *gamma, int64_t gsb, int64_t gsn,
                             void *stream) {
    const std::string who = "mm_latticeposteriors_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!offsets || !logz) return fail(MM_ERR_INVALID, who + ": offsets/logz is NULL");
    if (nrec < 0) return fail(MM_ERR_INVALID, who + ": nrec must be >= 0");
    if (nrec > 0 && (!arc || !post)) return fail(MM_ERR_INVALID, who + ": arc/post is NULL with nrec > 0");
    if (gamma && (gsn < 1 || gsb < N * gsn)) return fail(MM_ERR_DIM, who + ": gamma_stride_n < 1 or gamma_stride_b < N * gamma_stride_n");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    if (gamma && gsn < h->max_P1 - 1) return fail(MM_ERR_DIM, who + ": gamma_stride_n < P");
    if (h->B * N > int64_t(INT32_MAX)) return fail(MM_ERR_UNSUPPORTED, who + ": B * N exceeds 2^31 - 1 workgroups");
    if (mm_latpost_lds_bytes(h->max_S1p) > MM_LDS_MAX)
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->max_S1p) + " states (padded) exceed the " + std::to_string(latpost_state_cap()) +
                                            " whose vectors fit the LDS (16 bytes per state)");
    if (gamma && mm_latpost_gamma_lds_bytes(h->max_P1) > MM_LDS_MAX) return fail(MM_ERR_UNSUPPORTED, who + ": too many pdfs for the LDS: " + std::to_string(h->max_P1));
    const int nt = latpost_nt(h);
    if (nt != 256 && nt != 512 && nt != 1024) return fail(MM_ERR_INVALID, who + ": MM_LATPOST_NT must be 256, 512 or 1024");
    rc = ensure_item_forms(h, stream);
    if (!rc) rc = ensure_lattice_arcs(h, stream);
    if (rc) return rc;
    const RunParams p = run_params(h, V, vsb, vsn, lens, N);
    LatPostParams lp{};
    lp.arcs = static_cast<const LatticeDev *>(h->d_lat.get());
    lp.offs = reinterpret_cast<const long long *>(offsets);
    lp.arc = arc;
    lp.nrec = nrec;
    lp.extra = extra;
    lp.post = post;
    lp.logz = logz;
    lp.gamma = gamma;
    lp.gsb = gsb;
    lp.gsn = gsn;
    return mm_launch_latpost(h->B, nt, h->max_S1p, h->max_P1, p, lp, static_cast<hipStream_t>(stream));
}

// ---- lattice expected cost (mm_kernel_latpost.hip, the instance with costs): the risk of a lattice's paths and its gradient
int mm_latticecost_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const int64_t *offsets,
                       const int32_t *arc, int64_t nrec, const float *extra, const float *cost, float *risk, float *diff, float *post, float *logz,
                       float *grad, float *gamma, int64_t gsb, int64_t gsn, void *stream) {
    const std::string who = "mm_latticecost_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!offsets || !logz || !risk) return fail(MM_ERR_INVALID, who + ": offsets/logz/risk is NULL");
    if (nrec < 0) return fail(MM_ERR_INVALID, who + ": nrec must be >= 0");
    if (nrec > 0 && (!arc || !post || !cost || !diff)) return fail(MM_ERR_INVALID, who + ": arc/cost/diff/post is NULL with nrec > 0");
    if ((grad || gamma) && (gsn < 1 || gsb < N * gsn)) return fail(MM_ERR_DIM, who + ": stride_n < 1 or stride_b < N * stride_n");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    if ((grad || gamma) && gsn < h->max_P1 - 1) return fail(MM_ERR_DIM, who + ": stride_n < P");
    if (h->B * N > int64_t(INT32_MAX)) return fail(MM_ERR_UNSUPPORTED, who + ": B * N exceeds 2^31 - 1 workgroups");
    if (mm_latcost_lds_bytes(h->max_S1p) > MM_LDS_MAX)
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->max_S1p) + " states (padded) exceed the " + std::to_string(latcost_state_cap()) +
                                            " whose vectors fit the LDS (" + std::to_string(mm_latcost_lds_bytes(1) - mm_latcost_lds_bytes(0)) + " bytes per state)");
    if ((grad || gamma) && mm_latcost_grad_lds_bytes(h->max_P1) > MM_LDS_MAX)
        return fail(MM_ERR_UNSUPPORTED, who + ": too many pdfs for the LDS: " + std::to_string(h->max_P1));
    const int nt = latpost_nt(h);
    if (nt != 256 && nt != 512 && nt != 1024) return fail(MM_ERR_INVALID, who + ": MM_LATPOST_NT must be 256, 512 or 1024");
    rc = ensure_item_forms(h, stream);
    if (!rc) rc = ensure_lattice_arcs(h, stream);
    if (rc) return rc;
    const RunParams p = run_params(h, V, vsb, vsn, lens, N);
    LatPostParams lp{};
    lp.arcs = static_cast<const LatticeDev *>(h->d_lat.get());
    lp.offs = reinterpret_cast<const long long *>(offsets);
    lp.arc = arc;
    lp.nrec = nrec;
    lp.extra = extra;
    lp.post = post;
    lp.logz = logz;
    lp.gamma = gamma;
    lp.gsb = gsb;
    lp.gsn = gsn;
    LatCostParams lc{};
    lc.cost = cost;
    lc.risk = risk;
    lc.diff = diff;
    lc.grad = grad;
    return mm_launch_latcost(h->B, nt, h->max_S1p, h->max_P1, p, lp, lc, static_cast<hipStream_t>(stream));
}

// ---- lattice best paths (mm_kernel_latbest.hip): the tropical forward-backward over the records of a lattice, and the best path
int mm_latticebest_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const int64_t *offsets,
                       const int32_t *arc, int64_t nrec, const float *extra, float *best, float *score, int64_t *rec, int64_t rsb, int32_t *path,
                       int64_t psb, void *stream) {
    const std::string who = "mm_latticebest_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!offsets || !best) return fail(MM_ERR_INVALID, who + ": offsets/best is NULL");
    if (nrec < 0) return fail(MM_ERR_INVALID, who + ": nrec must be >= 0");
    if (nrec > 0 && (!arc || !score)) return fail(MM_ERR_INVALID, who + ": arc/score is NULL with nrec > 0");
    if (rec && rsb < N) return fail(MM_ERR_DIM, who + ": rec_stride_b < N");
    if (path && psb < N) return fail(MM_ERR_DIM, who + ": path_stride_b < N");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    if (mm_latbest_lds_bytes(h->max_S1p) > MM_LDS_MAX)
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->max_S1p) + " states (padded) exceed the " + std::to_string(latbest_state_cap()) +
                                            " whose vectors fit the LDS (" + std::to_string(mm_latbest_lds_bytes(1) - mm_latbest_lds_bytes(0)) + " bytes per state)");
    const int nt = latpost_nt(h);
    if (nt != 256 && nt != 512 && nt != 1024) return fail(MM_ERR_INVALID, who + ": MM_LATPOST_NT must be 256, 512 or 1024");
    rc = ensure_item_forms(h, stream);
    if (!rc) rc = ensure_lattice_arcs(h, stream);
    if (rc) return rc;
    const RunParams p = run_params(h, V, vsb, vsn, lens, N);
    LatPostParams lp{};
    lp.arcs = static_cast<const LatticeDev *>(h->d_lat.get());
    lp.offs = reinterpret_cast<const long long *>(offsets);
    lp.arc = arc;
    lp.nrec = nrec;
    lp.extra = extra;
    lp.post = score;
    lp.logz = best;
    LatBestParams lb{};
    lb.rec = reinterpret_cast<long long *>(rec);
    lb.rsb = rsb;
    lb.path = path;
    lb.psb = psb;
    return mm_launch_latbest(h->B, nt, h->max_S1p, p, lp, lb, static_cast<hipStream_t>(stream));
}

// ---- lattice path sampling (mm_kernel_latsample.hip): the forward pass of the lattice posteriors, then record sequences drawn
// backwards from the lattice's posterior
int mm_latticesample_f32(mm_batch_t h, const float *V, int64_t vsb, int64_t vsn, const int32_t *lens, int64_t N, const int64_t *offsets,
                         const int32_t *arc, int64_t nrec, const float *extra, int64_t nsamples, int64_t seed, float *fwd, int64_t *rec, int64_t rsb,
                         int64_t rsk, int32_t *path, int64_t psb, int64_t psk, float *logprob, int64_t lsb, float *logz, void *stream) {
    const std::string who = "mm_latticesample_f32";
    // what the arguments alone show comes first, then the batch's refusals
    if (!offsets || !logz) return fail(MM_ERR_INVALID, who + ": offsets/logz is NULL");
    if (nrec < 0) return fail(MM_ERR_INVALID, who + ": nrec must be >= 0");
    if (nrec > 0 && (!arc || !fwd)) return fail(MM_ERR_INVALID, who + ": arc/fwd is NULL with nrec > 0");
    if (nsamples < 1) return fail(MM_ERR_INVALID, who + ": nsamples must be >= 1");
    if (!rec && !path) return fail(MM_ERR_INVALID, who + ": rec and path are both NULL");
    if (rec && (rsk < N || rsb < nsamples * rsk)) return fail(MM_ERR_DIM, who + ": rec_stride_k < N or rec_stride_b < nsamples * rec_stride_k");
    if (path && (psk < N || psb < nsamples * psk)) return fail(MM_ERR_DIM, who + ": path_stride_k < N or path_stride_b < nsamples * path_stride_k");
    if (logprob && lsb < nsamples) return fail(MM_ERR_DIM, who + ": lp_stride_b < nsamples");
    if (nsamples > int64_t(MM_LS_CHUNK) * MM_LS_MAX_CHUNKS)
        return fail(MM_ERR_UNSUPPORTED, who + ": more than " + std::to_string(int64_t(MM_LS_CHUNK) * MM_LS_MAX_CHUNKS) + " samples in one call");
    if (h && h->semiring != MM_TROPICAL)
        return fail(MM_ERR_UNSUPPORTED, who + ": tropical batches only (this batch is " + (h->semiring == MM_LOG ? "log-semiring" : "ProbSemiring") + ")");
    int rc = check_run(h, who.c_str(), V, N, MM_TROPICAL);
    if (rc) return rc;
    if (mm_latsample_lds_bytes(h->max_S1p) > MM_LDS_MAX)
        return fail(MM_ERR_UNSUPPORTED, who + ": " + std::to_string(h->max_S1p) + " states (padded) exceed the " + std::to_string(latsample_state_cap()) +
                                            " whose vectors fit the LDS (16 bytes per state)");
    const int nt = latpost_nt(h);
    if (nt != 256 && nt != 512 && nt != 1024) return fail(MM_ERR_INVALID, who + ": MM_LATPOST_NT must be 256, 512 or 1024");
    rc = ensure_item_forms(h, stream);
    if (!rc) rc = ensure_lattice_arcs(h, stream);
    if (rc) return rc;
    const RunParams p = run_params(h, V, vsb, vsn, lens, N);
    LatPostParams lp{};
    lp.arcs = static_cast<const LatticeDev *>(h->d_lat.get());
    lp.offs = reinterpret_cast<const long long *>(offsets);
    lp.arc = arc;
    lp.nrec = nrec;
    lp.extra = extra;
    lp.post = fwd;
    lp.logz = logz;
    LatSampleParams ls{};
    ls.nsamples = nsamples;
    ls.key0 = unsigned(uint64_t(seed));
    ls.key1 = unsigned(uint64_t(seed) >> 32);
    ls.rec = reinterpret_cast<long long *>(rec);
    ls.rsb = rsb;
    ls.rsk = rsk;
    ls.path = path;
    ls.psb = psb;
    ls.psk = psk;
    ls.logprob = logprob;
    ls.lsb = lsb;
    return mm_launch_latsample(h->B, nt, h->max_S1p, p, lp, ls, static_cast<hipStream_t>(stream));
}

}  // extern "C"
