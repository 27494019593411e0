// Stand-alone: packs graphs as the engine packs them for the pair and team kernels (mm_rows.cpp: make_rows, make_rows_split)
// and prints the end mask of every compute wave -- where, in the arc window of pair_agent (mm_kernel_pairs.hip), its segments
// end.  Built and run by tests/test_pair_window_cases.py, which writes the graphs (the pruned matrices of mm_fsm_create) and
// checks that the masks reach every path of the window: the GPU tests of tests/test_gpu_pair_window.py run these graphs.
//
//   pair_window_cases <graph file> pair      the pair forms (one workgroup per direction, window of 44 arc slots)
//   pair_window_cases <graph file> team      the forms of a team of 2 (window of 36)
//
// graph file (text): S1 P1, then for the forward (rows of T_hat') and the backward (rows of T_hat) matrix: nnz, S1 + 1 row
// pointers, nnz columns, nnz log2 weights; then S1 pdfs.
//
// The options are the engine's (mm_engine.hip: pair_pack_opts, split_pack_opts) without any debug switch, written out here.
// Prints one line per wave: "<graph> <form> dir <d> set <h> KA <ka> wave <w> segments <n> endmask <hex>"; exits 0 iff all packed.
#include "mm_rows.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mm;

struct Csr {
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<float> val;
};

static bool read_csr(std::FILE *f, int64_t S1, Csr &m) {
    long long nnz = 0;
    if (std::fscanf(f, "%lld", &nnz) != 1) return false;
    m.rowptr.resize(size_t(S1) + 1);
    m.col.resize(size_t(nnz));
    m.val.resize(size_t(nnz));
    for (auto &x : m.rowptr) {
        long long v;
        if (std::fscanf(f, "%lld", &v) != 1) return false;
        x = v;
    }
    for (auto &x : m.col) {
        int v;
        if (std::fscanf(f, "%d", &v) != 1) return false;
        x = v;
    }
    for (auto &x : m.val)
        if (std::fscanf(f, "%f", &x) != 1) return false;
    return m.rowptr[size_t(S1)] == nnz;
}

// pair_pack_opts(dbg = none, dir, lag = true)
static RowPackOpts pair_opts(int dir) {
    RowPackOpts opt;
    opt.rs = 8192;    // MM_ROW_RS
    opt.ka_max = 44;  // MM_PAIR_KA
    opt.pair = true;
    opt.pdf_halves = true;
    for (float &x : opt.group_speed) x = 1.f;
    if (dir == 1) {
        opt.finish_cost = 24;
        const float sp[4] = {1.08f, 1.04f, 0.97f, 0.92f};
        for (int i = 0; i < 4; ++i) opt.group_speed[i] = sp[i];
    }
    opt.ka_choices[0] = 44;
    return opt;
}

// split_pack_opts(dbg = none, H = 2)
static void team_opts(RowPackOpts &opt, RowPackOpts &optb) {
    opt = RowPackOpts();
    opt.rs = 12288;   // mm_split_rs(2)
    opt.ka_max = 36;  // mm_split_ka(2)
    opt.nwc_max = 14; // MM_SPLIT_NWC
    opt.pair = true;
    opt.pdf_halves = true;
    for (float &x : opt.group_speed) x = 1.f;
    opt.ka_choices[0] = 36;
    opt.every_cap = false;
    optb = opt;
    optb.finish_cost = 24;
}

static void say(const char *name, const char *form, int dir, int set, const RowGraph &g) {
    for (int w = 0; w < g.NWC; ++w) {
        const RowSched &sc = g.sched[size_t(w)];
        std::printf("%s %s dir %d set %d KA %d wave %d segments %u endmask %llx\n", name, form, dir, set, g.KA, w, sc.nslots & 0xffffu,
                    (unsigned long long)sc.endmask);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long S1 = 0;
    int P1 = 0;
    Csr m[2];
    if (std::fscanf(f, "%lld %d", &S1, &P1) != 2 || !read_csr(f, S1, m[0]) || !read_csr(f, S1, m[1])) return 2;
    std::vector<int32_t> s2p(size_t(S1), 0);
    for (auto &x : s2p) {
        int v;
        if (std::fscanf(f, "%d", &v) != 1) return 2;
        x = v;
    }
    std::fclose(f);
    const char *name = std::strrchr(argv[1], '/') ? std::strrchr(argv[1], '/') + 1 : argv[1];
    const std::vector<int32_t> none;
    if (!std::strcmp(argv[2], "pair")) {  // pack_both
        RowGraph g[2];
        if (!make_rows(S1, m[0].rowptr, m[0].col, m[0].val, s2p, P1, false, none, pair_opts(0), g[0]) ||
            !make_rows(S1, m[1].rowptr, m[1].col, m[1].val, s2p, P1, true, g[0].pos, pair_opts(1), g[1])) {
            std::printf("%s: does not fit the pair forms\n", name);
            return 1;
        }
        for (int d = 0; d < 2; ++d) say(name, "pair", d, 0, g[d]);
    } else if (!std::strcmp(argv[2], "team")) {
        RowPackOpts opt, optb;
        team_opts(opt, optb);
        std::vector<RowGraph> gs;
        SplitInfo info;
        if (!make_rows_split(2, S1, m[0].rowptr, m[0].col, m[0].val, m[1].rowptr, m[1].col, m[1].val, s2p, P1, opt, optb, gs, info)) {
            std::printf("%s: does not fit the forms of a team of 2\n", name);
            return 1;
        }
        for (int d = 0; d < 2; ++d)
            for (int h = 0; h < 2; ++h) say(name, "team", d, h, gs[size_t(d * 2 + h)]);
    } else return 2;
    return 0;
}
