"""The arc window of the pair kernels (mm_kernel_pairs.hip: pair_two / MM_PAIR_TWO) takes two pairs of arcs -- a quad -- per test
of a wave's end mask, in one chain of packed FMAs that runs on through the second pair as if no segment ended between the two;
what happens when one does is the rare path.  tests/test_gpu_pair_window.py runs the graphs below on the GPU; this test packs the
same graphs on the host (tests/pair_window_cases.cpp + mm_rows.cpp, the engine's options) and asserts that the end masks of their
compute waves, forward and backward, reach every place a segment can end relative to a quad -- so the GPU tests cannot pass by never
taking a path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# name -> (graph, form the GPU test forces, text expected in Batch.kernels())
GRAPHS = {
    "small": (lambda wl: wl.random_fsm(120, 20, 3.0, seed=3), "pair", "mm_fbp_kernel<2,A>, then <2,B>"),  # <2, ., true>: up to 127 states
    # (a wave has more than one segment only where a direction has more than 15 x 64 rows: the headline graph's size)
    "den": (lambda wl: wl.lfmmi_denominator(2000, 84), "pair", "mm_fbp_kernel<2,A>, then <2,B>"),  # <2, ., false>
    "den_p200": (lambda wl: wl.lfmmi_denominator(2000, 200, seed=2), "pair", "mm_fbp_kernel<4,A>, then <4,B>"),  # <4, .>: 129 .. 250 pdfs
    "wide": (lambda wl: wl.wide_row_fsm(700), "pair", "mm_fbp_kernel<2,A>, then <2,B>"),  # rows on 2 .. 64 lanes: group sums
    "den_team": (lambda wl: wl.lfmmi_denominator(2000, 84), "team", "mm_fbs_kernel<2,A,2>, then <2,B,2>"),
}
# the pairs whose quads stand right before the three early exits of the window (MM_PAIR_CASES: lastp >= 14, >= 18, >= 20)
EXIT_QUADS = (12, 16, 18)


def pruned_matrices(g):
    """What mm_fsm_create hands the packer for a log-semiring graph: CSR of T_hat' (forward) and of T_hat (backward) over the
    states + the phony final state, columns ascending, restricted to the useful states, log2 weights; the pdfs."""
    S1 = g.S + 1
    src = np.concatenate([g.src, g.final_idx, [g.S]]).astype(np.int64)
    dst = np.concatenate([g.dst, np.full(g.final_idx.size, g.S), [g.S]]).astype(np.int64)
    w = np.concatenate([g.w, g.final_w, [0.0]]).astype(np.float32) * np.float32(1.4426950408889634)
    assert np.unique(src * S1 + dst).size == src.size
    out_arcs = [[] for _ in range(S1)]
    in_arcs = [[] for _ in range(S1)]
    for i, j in zip(src, dst):
        out_arcs[i].append(j)
        in_arcs[j].append(i)

    def closure(seeds, nbr):
        seen = np.zeros(S1, dtype=bool)
        seen[list(seeds)] = True
        stack = list(seeds)
        while stack:
            for j in nbr[stack.pop()]:
                if not seen[j]:
                    seen[j] = True
                    stack.append(j)
        return seen

    reach, coreach = closure([int(i) for i in g.init_idx], out_arcs), closure([S1 - 1], in_arcs)
    n_extra = int((coreach & ~reach).sum())
    useful = coreach & (reach | (n_extra * 64 <= S1))
    keep = useful[src] & useful[dst] & np.isfinite(w)
    mats = []
    for rows, cols in ((dst, src), (src, dst)):
        o = np.lexsort((cols[keep], rows[keep]))
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=S1))])
        mats.append((rowptr, cols[keep][o], w[keep][o]))
    return S1, g.P + 1, mats, np.concatenate([g.state2pdf, [g.P]]).astype(np.int64)


def write_graph(path, g):
    S1, P1, mats, s2p = pruned_matrices(g)
    with open(path, "w") as f:
        f.write(f"{S1} {P1}\n")
        for rowptr, col, val in mats:
            f.write(f"{col.size}\n" + " ".join(map(str, rowptr)) + "\n" + " ".join(map(str, col)) + "\n" + " ".join(repr(float(x)) for x in val) + "\n")
        f.write(" ".join(map(str, s2p)) + "\n")


def cases_of(ka, nseg, mask):
    """the window's cases that a wave of this end mask takes (KA arc slots: pairs 0 .. KA / 2 - 1, quads of two pairs)"""
    ends = [(mask >> k) & 1 for k in range(ka // 2)]
    assert sum(ends) == nseg and mask >> (ka // 2) == 0
    last = max(k for k in range(ka // 2) if ends[k])
    quads = [(ends[k], ends[k + 1]) for k in range(0, ka // 2, 2)]  # (KA is a multiple of 4 in every shipped window)
    c = set()
    for q, (a, b) in enumerate(quads):
        if a and not b:
            c.add("first pair only")
        if b and not a:
            c.add("second pair only")
        if a and b:
            c.add("both pairs")
        if (a or b) and q + 1 < len(quads) and any(quads[q + 1]):
            c.add("two consecutive quads")
        if (a or b) and 2 * q in EXIT_QUADS:
            c.add(f"quad before the exit at pair {2 * q + 2}")
            if last <= 2 * q + 1:
                c.add(f"last segment ends right before the exit at pair {2 * q + 2}")
    if any(quads[-1]):
        c.add("window's last quad")
    if nseg == 1:
        c.add("single segment")
    return c


ALWAYS = {"first pair only", "second pair only", "both pairs", "two consecutive quads", "window's last quad", "single segment"}
# (all three exits exist in the window of 44, pairs 0 .. 21; a team's window of 36 ends at pair 17 and has the first alone)
PAIR_ONLY = {f"quad before the exit at pair {k + 2}" for k in EXIT_QUADS} | {f"last segment ends right before the exit at pair {k + 2}" for k in EXIT_QUADS}


@pytest.fixture(scope="module")
def window_cases(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/hipcc")
                if c and shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    csrc = os.path.join(ROOT, "markovmodels.jl_amd", "csrc")
    d = tmp_path_factory.mktemp("window_cases")
    exe = str(d / "pair_window_cases")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", csrc, os.path.join(HERE, "pair_window_cases.cpp"), os.path.join(csrc, "mm_rows.cpp"), "-o", exe])
    return exe, d


def test_the_graphs_reach_every_case_of_the_window(window_cases, mm, wl):
    exe, d = window_cases
    seen = {}  # (form, dir) -> cases
    for name, (make, form, _) in GRAPHS.items():
        path = str(d / name)
        g = make(wl)
        write_graph(path, g)
        r = subprocess.run([exe, path, form], capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        mine = {}
        for line in r.stdout.splitlines():
            t = line.split()
            assert t[1] == form and t[6] == "KA" and t[-2] == "endmask"
            ka, direction = int(t[7]), int(t[3])
            assert ka == (44 if form == "pair" else 36)
            c = cases_of(ka, int(t[11]), int(t[-1], 16))
            mine.setdefault(direction, set()).update(c)
            seen.setdefault((form, direction), set()).update(c)
        for direction, c in sorted(mine.items()):
            print(f"{name} ({form}) dir {direction}:", sorted(c))
        # The options and the pruning above are written out a second time here; the engine packs the same forms in its host-only
        # product entries and reports their window, waves and segments: a copy that drifted from the engine shows up here.
        f = wl.to_fsm(mm, g)
        cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
        x = np.zeros(f.S1, dtype=np.float32)
        for direction in (0, 1):
            rows = [t for t in (line.split() for line in r.stdout.splitlines()) if int(t[3]) == direction]
            stats = cf.row_product(x, direction, pair=True)[1] if form == "pair" else cf.split_product(x, direction, 2)[1]
            assert int(stats[0]) == int(rows[0][7]) and int(stats[2]) == sum(int(t[11]) for t in rows), (name, direction, list(stats[:3]))
            if form == "pair":
                assert int(stats[1]) == len(rows), (name, direction, list(stats[:3]))
    union = set().union(*seen.values())
    assert ALWAYS | PAIR_ONLY <= union, sorted((ALWAYS | PAIR_ONLY) - union)
    # The quad's code exists once per kernel and is the same in both phases, so every place of an end relative to a quad must
    # come up in both directions of the pair forms and of the team's forms ...
    places = {"first pair only", "second pair only", "both pairs", "two consecutive quads"}
    for key in (("pair", 0), ("pair", 1), ("team", 0), ("team", 1)):
        assert places <= seen[key], (key, sorted(places - seen[key]))
    # ... and the three exits (a team's window of 36 slots ends at pair 17: it has the first alone) and the window's last quad in
    # both directions of the pair forms
    for direction in (0, 1):
        need = {f"quad before the exit at pair {k + 2}" for k in EXIT_QUADS} | {"window's last quad"}
        assert need <= seen[("pair", direction)], (direction, sorted(need - seen[("pair", direction)]))
