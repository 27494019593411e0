// Stand-alone check of the row packer's plans (mm_rows.cpp: make_rows), built and run by tests/test_pair_plan.py.
// What the Python test aids cannot see: the segments of every wave, the arc slots they own, the lanes a given row got.
//
//   pair_plan_check edge            the edge of the single-lane rule (rows of ka_max - 1, ka_max, ka_max + 1 arcs)
//   pair_plan_check random <seed>   a graph of random row lengths, both finish costs
//   pair_plan_check exchange        the teams' window of 36 slots, a graph that fits its waves only after an exchange
//
// The options are built here (every cap, group speeds of 1), not by the engine.  The shipped team forms set every_cap = false
// and so never exchange: `exchange` is the only check of that path at their window.
//
// Prints one line per check and exits 0 iff all hold.
#include "mm_rows.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace mm;

static int KA_MAX = 44;  // the pair kernels' register window (MM_PAIR_KA); `exchange`: the teams' (mm_split_ka)
static int failures = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

struct Csr {
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col, pdf;
    std::vector<float> val;
    int64_t n = 0;
};

// row r reads deg[r] distinct rows, spread over the whole vector
static Csr make_graph(const std::vector<int> &deg, int P1) {
    Csr m;
    m.n = int64_t(deg.size());
    m.rowptr.push_back(0);
    for (int64_t r = 0; r < m.n; ++r) {
        for (int k = 0; k < deg[size_t(r)]; ++k) {
            m.col.push_back(int32_t((r + 1 + int64_t(k) * 7) % m.n));
            m.val.push_back(-0.25f * float(1 + (r + k) % 9));
        }
        m.rowptr.push_back(int64_t(m.col.size()));
        m.pdf.push_back(int32_t(r % P1));
    }
    return m;
}

static RowPackOpts pair_opts(int finish_cost) {
    RowPackOpts opt;
    opt.rs = 16384;
    opt.ka_max = KA_MAX;
    opt.pair = true;
    opt.pdf_halves = true;
    for (float &x : opt.group_speed) x = 1.f;
    opt.finish_cost = finish_cost;
    opt.ka_choices[0] = KA_MAX;
    return opt;
}

struct Where {
    int wave = -1, seg = -1, lanes = 0, A = 0;
};

// Walks the schedule as a kernel does.  Checks the limits of every wave; where[p] = the segment that finishes position p.
static void walk(const RowGraph &g, const char *what, std::vector<Where> &where) {
    where.assign(size_t(g.nrows), Where());
    CHECK(g.KA <= KA_MAX && g.KA % 2 == 0, "%s: KA %d", what, g.KA);
    CHECK(g.NWC >= 1 && g.NWC <= 15, "%s: %d waves", what, g.NWC);
    int finished = 0;
    for (int w = 0; w < g.NWC; ++w) {
        const RowSched &sc = g.sched[size_t(w)];
        const int nseg = int(sc.nslots & 0xffffu);
        CHECK(nseg >= 1 && nseg <= MM_ROW_MAX_SLOTS, "%s: wave %d has %d segments", what, w, nseg);
        int seg = 0, first = 0, ends = 0;
        for (int k2 = 0; k2 < 64; ++k2)
            if ((sc.endmask >> k2) & 1) {
                ++ends;
                CHECK(2 * (k2 + 1) <= g.KA, "%s: wave %d ends a segment after arc %d, KA %d", what, w, 2 * (k2 + 1), g.KA);
                if (seg < nseg) {
                    const int lg = int((sc.lg >> (4 * seg)) & 15), lanes = 1 << lg;
                    for (int l = lanes - 1; l < 64; l += lanes) {
                        const uint32_t info = g.slots[(size_t(sc.slot0) + size_t(seg)) * 64 * size_t(g.slot_words) + size_t(l) * size_t(g.slot_words)];
                        const int p = int(info & 0xffffu) / g.scale;
                        if (p == g.trash) continue;
                        CHECK(p >= 0 && p < g.nrows && where[size_t(p)].wave < 0, "%s: position %d finished twice or out of range", what, p);
                        if (p >= 0 && p < g.nrows) where[size_t(p)] = Where{w, seg, lanes, 2 * (k2 + 1) - first};
                        ++finished;
                    }
                }
                first = 2 * (k2 + 1);
                ++seg;
            }
        CHECK(ends == nseg, "%s: wave %d: %d segment ends for %d segments", what, w, ends, nseg);
    }
    CHECK(finished == g.nrows, "%s: %d of %d rows finished", what, finished, g.nrows);
}

// the product through the form against the CSR, in the linear domain
static void check_product(const Csr &m, const RowGraph &g, const char *what) {
    std::vector<float> in(size_t(m.n) + 1, 0.f), out(size_t(m.n) + 1, 0.f);
    for (int64_t r = 0; r < m.n; ++r) in[size_t(g.pos[size_t(r)])] = 0.5f + float((r * 37) % 101) / 101.f;
    eval_rows(g, in.data(), out.data());
    double worst = 0;
    for (int64_t r = 0; r < m.n; ++r) {
        double ref = 0;
        for (int64_t a = m.rowptr[size_t(r)]; a < m.rowptr[size_t(r) + 1]; ++a)
            ref += std::exp2(double(m.val[size_t(a)])) * double(in[size_t(g.pos[size_t(m.col[size_t(a)])])]);
        worst = std::max(worst, std::fabs(double(out[size_t(g.pos[size_t(r)])]) - ref) / std::max(ref, 1e-30));
    }
    // (float32 sums of at most ~50 positive terms: a few ulps each)
    CHECK(worst <= 1e-5, "%s: relative error of the product %.3g", what, worst);
}

static void edge() {
    // 8 x 64 rows of about ka_max arcs and 15 waves.  With the cap at ka_max the 511 rows of <= ka_max arcs make 8 single-lane
    // segments (cost ka_max + finish on 8 waves) and the row of ka_max + 1 arcs takes two lanes.  Every lower cap splits ALL rows:
    // 16 two-lane segments of ka_max / 2 (+) arcs need one wave twice -- dearer than one single-lane segment, or beyond the window
    // -- and 32 four-lane segments are dearer still.  So the plan with the cap at the window wins, and the rule shows at its edge.
    std::vector<int> deg(512, KA_MAX);
    const int r_less = 100, r_full = 200, r_more = 300;
    deg[r_less] = KA_MAX - 1;
    deg[r_more] = KA_MAX + 1;
    const Csr m = make_graph(deg, 40);
    for (int finish : {8, 24}) {
        RowGraph g;
        const std::vector<int32_t> none;
        const bool ok = make_rows(m.n, m.rowptr, m.col, m.val, m.pdf, 40, false, none, pair_opts(finish), g);
        CHECK(ok, "edge graph, finish cost %d: no plan", finish);
        if (!ok) continue;
        std::vector<Where> where;
        walk(g, "edge", where);
        check_product(m, g, "edge");
        const Where a = where[size_t(g.pos[r_less])], b = where[size_t(g.pos[r_full])], c = where[size_t(g.pos[r_more])];
        std::printf("edge, finish cost %d: %d arcs -> %d lane(s) x %d slots, %d arcs -> %d x %d, %d arcs -> %d x %d; cost %d, %d segments\n", finish,
                    KA_MAX - 1, a.lanes, a.A, KA_MAX, b.lanes, b.A, KA_MAX + 1, c.lanes, c.A, g.maxcost, g.nslotrows - 2);
        CHECK(a.lanes == 1 && a.A == KA_MAX, "row of ka_max - 1 arcs: %d lanes x %d", a.lanes, a.A);
        CHECK(b.lanes == 1 && b.A == KA_MAX, "row of ka_max arcs: %d lanes x %d", b.lanes, b.A);
        CHECK(c.lanes == 2 && c.A == (KA_MAX + 1 + 1) / 2 + ((KA_MAX + 1 + 1) / 2) % 2, "row of ka_max + 1 arcs: %d lanes x %d", c.lanes, c.A);
    }
}

static void random_graph(unsigned seed) {
    std::mt19937 rng(seed);
    // row lengths like a denominator graph's: most short, a tail up to and beyond the window
    std::vector<int> deg(1400);
    for (int &d : deg) {
        const unsigned u = rng() % 100;
        d = u < 55 ? 1 + int(rng() % 12) : u < 90 ? 12 + int(rng() % 22) : 34 + int(rng() % 14);
    }
    deg[7] = 300;  // (a row for a whole wave's lanes)
    const Csr m = make_graph(deg, 84);
    for (int finish : {8, 24}) {
        RowGraph g;
        const std::vector<int32_t> none;
        const bool ok = make_rows(m.n, m.rowptr, m.col, m.val, m.pdf, 84, false, none, pair_opts(finish), g);
        CHECK(ok, "random graph %u, finish cost %d: no plan", seed, finish);
        if (!ok) continue;
        std::vector<Where> where;
        walk(g, "random", where);
        check_product(m, g, "random");
        for (int64_t r = 0; r < m.n; ++r) {
            const Where x = where[size_t(g.pos[size_t(r)])];
            CHECK(x.lanes * x.A >= deg[size_t(r)] && x.A <= KA_MAX, "row %d of %d arcs on %d lanes x %d slots", int(r), deg[size_t(r)], x.lanes, x.A);
        }
        std::printf("random %u, finish cost %d: KA %d, %d waves, %d segments, cost %d..%d\n", seed, finish, g.KA, g.NWC, g.nslotrows - 2, g.mincost, g.maxcost);
    }
}

static void exchange() {
    // 3 waves of 36 slots and 13 segments of 64 single-lane rows each, 108 arcs per lane in all: the graph fits only if no slot
    // stays free ({12 12 12}, {10 10 10 6}, {8 8 6 6 4 4} is one way).  Every row is below 12 arcs, so ONE cap is planned.
    // Longest-first by cost fills the waves evenly and leaves the last segment of 4 no wave with 4 free slots; one exchange
    // of a longer and a shorter segment between two waves makes the room.
    KA_MAX = 36;
    std::vector<int> deg;
    for (int A : {12, 12, 12, 10, 10, 10, 8, 8, 6, 6, 6, 4, 4})
        for (int r = 0; r < 64; ++r) deg.push_back(r % 3 == 0 ? A : A - 1);  // (A - 1 arcs round up to A slots)
    const Csr m = make_graph(deg, 40);
    for (int finish : {8, 24}) {
        RowPackOpts opt = pair_opts(finish);
        opt.nwc_max = 3;
        RowGraph g;
        const std::vector<int32_t> none;
        const bool ok = make_rows(m.n, m.rowptr, m.col, m.val, m.pdf, 40, false, none, opt, g);
        CHECK(ok, "exchange graph, finish cost %d: no plan", finish);
        if (!ok) continue;
        std::vector<Where> where;
        walk(g, "exchange", where);
        check_product(m, g, "exchange");
        std::printf("exchange, finish cost %d: KA %d, %d waves, %d segments, cost %d..%d, %d exchange(s)\n", finish, g.KA, g.NWC, g.nslotrows - 2, g.mincost,
                    g.maxcost, g.exchanges);
        CHECK(g.exchanges >= 1 && g.KA == 36 && g.NWC == 3 && g.nslotrows - 2 == 13, "%d exchanges, KA %d, %d waves", g.exchanges, g.KA, g.NWC);
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "edge")) edge();
    else if (argc >= 2 && !std::strcmp(argv[1], "exchange")) exchange();
    else if (argc >= 3 && !std::strcmp(argv[1], "random")) random_graph(unsigned(std::atoi(argv[2])));
    else return 2;
    std::printf(failures ? "%d check(s) failed\n" : "all checks hold\n", failures);
    return failures ? 1 : 0;
}
