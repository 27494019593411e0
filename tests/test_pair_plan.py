"""The plan search of the row packer (mm_rows.cpp make_rows: every even cap on the arcs of a row per lane up to the register
window, an exchange of two segments before a cap is given up for want of room in one wave): the products of the pair and split forms
stay those of the item form, no plan is dearer than the parent commit's, the backward form of the headline graph is as short
as the cap list makes it, and a plan keeps the limits of the kernels that load it.

tests/golden/pair_plan_parent.json: stats[0:8] of row_product(x, d, pair=True) and split_product(x, d, 2) as the commit
before the longer cap list computed them (null: the graph does not fit the form), key "<graph>/<form>/<direction>"."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAIR_KA, SPLIT_KA = 44, 36  # MM_PAIR_KA, mm_split_ka() of mm_internal.h

GRAPHS = {
    "lfmmi_2000_84": lambda wl: wl.lfmmi_denominator(2000, 84),
    "lfmmi_600_40_s5": lambda wl: wl.lfmmi_denominator(600, 40, seed=5),
    "lfmmi_2000_400_s1": lambda wl: wl.lfmmi_denominator(2000, 400, seed=1),
    "wide_row": lambda wl: wl.wide_row_fsm(),
    "den_wsj": lambda wl: wl.load_npz_graph(os.path.join(HERE, "golden", "den_fsm_wsj.npz")),
    "num_wsj": lambda wl: wl.load_npz_graph(os.path.join(HERE, "golden", "num_fsm_wsj.npz")),
}
PARENT = json.load(open(os.path.join(HERE, "golden", "pair_plan_parent.json")))
_compiled = {}


def compiled(mm, wl, gname):
    """(FSM, compiled FSM, input vector, item-form products of both directions): once per graph"""
    if gname not in _compiled:
        g = GRAPHS[gname](wl)
        f = wl.to_fsm(mm, g)
        cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
        rng = np.random.default_rng(8)
        x = (3 * rng.standard_normal(f.S1)).astype(np.float32)
        x[rng.random(f.S1) < 0.1] = -np.inf
        _compiled[gname] = (f, cf, x, [cf.packed_product(x, d)[0] for d in (0, 1)])
    return _compiled[gname]


def same_product(out, ref):
    m = np.isfinite(ref)
    assert np.array_equal(np.isfinite(out), m) and np.array_equal(out[~m], ref[~m])  # (the -inf entries: exactly)
    assert np.allclose(out[m], ref[m], rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_pair_form_products_and_plan(mm, wl, gname, d):
    f, cf, x, refs = compiled(mm, wl, gname)
    parent = PARENT[f"{gname}/pair/{d}"]
    if parent is None:  # (the reference's WSJ denominator: 52 k arcs do not fit one workgroup's registers, before or after)
        with pytest.raises(mm.MarkovModelsAMDError):
            cf.row_product(x, d, pair=True)
        return
    out, stats = cf.row_product(x, d, pair=True)
    same_product(out, refs[d])
    ka, nwc, nseg, eff, cmax, cmin = stats[:6]
    print(gname, d, "parent", parent[:6], "now", list(stats[:6]))
    assert ka == parent[0] == PAIR_KA
    assert 1 <= nwc <= 15 and nwc <= nseg <= 16 * nwc and 0 < eff <= 1.0
    assert cmax <= parent[4], (gname, d, cmax, parent[4])
    if gname == "lfmmi_2000_84" and d == 1:
        # rows of 33 .. 42 arcs stay on one lane (cap 42): 42 -> 32 finishes per step, the most loaded wave 118 -> 98
        assert nseg <= 34 and cmax <= 100, (nseg, cmax)
    if gname == "lfmmi_2000_84" and d == 0:
        # 43 -> 40 segments, the most loaded wave 72 -> 70 (cap 38; cap 36 gives 41 segments at the same cost and slots, and the
        # tie goes to the fewer segments: the third key of make_rows' choice, which the measured gain of the forward form rests
        # on).  The caps 40, 42 and 44 would give 40, 40 and 39 segments but cannot be dealt at all: 17, 17 and 16 of their
        # segments are >= 22 arcs long and there are 15 waves: two pairs (one pair) of them would have to share a wave's 44
        # slots, and of the shortest -- 22, 22, 24, 24 (22, 24) -- only 22 + 22 does.
        print("forward form of the headline graph:", int(nseg), "segments, most loaded wave", int(cmax))
        assert nseg <= 40 and cmax <= 70, (nseg, cmax)


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_split_form_products_and_plan(mm, wl, gname, d):
    """Teams of 2 (what runs the WSJ denominator), and the same bar on the graphs whose pair form ships.  The team forms keep the
    caps 12, 16, 24, 32 (RowPackOpts::every_cap = false: their kernels measured no gain from more): the parent's plans."""
    f, cf, x, refs = compiled(mm, wl, gname)
    parent = PARENT[f"{gname}/split2/{d}"]
    out, stats = cf.split_product(x, d, 2)
    same_product(out, refs[d])
    print(gname, d, "parent", parent[:6], "now", list(stats[:6]))
    assert stats[0] == parent[0] == SPLIT_KA and f.S1 <= stats[1] <= f.S1 + 2
    assert stats[4] <= parent[4], (gname, d, stats[4], parent[4])
    assert list(stats[:6]) == parent[:6], (gname, d, list(stats[:6]), parent[:6])


def test_plans_are_deterministic(mm, wl):
    """Two packs of one graph give the same form (the run-to-run bit identity of the kernels rests on it)."""
    f, cf, x, refs = compiled(mm, wl, "lfmmi_600_40_s5")
    for d in (0, 1):
        a, sa = cf.row_product(x, d, pair=True)
        b, sb = cf.row_product(x, d, pair=True)
        assert np.array_equal(a, b) and np.array_equal(sa, sb)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tests/pair_plan_check.cpp + the packer, as a host program (no GPU code in either)."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/hipcc")
                if c and shutil.which(c)), None)
    assert cxx, "no C++ compiler"
    csrc = os.path.join(ROOT, "markovmodels.jl_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("plan_check") / "pair_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", csrc, os.path.join(HERE, "pair_plan_check.cpp"),
                           os.path.join(csrc, "mm_rows.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("args", [("edge",), ("exchange",), ("random", "1"), ("random", "2")])
def test_plan_limits_and_the_single_lane_edge(plan_check, args):
    """Walks the schedule of whole forms as a kernel does: at most MM_ROW_MAX_SLOTS segments per wave, no segment beyond the
    KA slots of a lane, KA within the window, every row finished once on lanes that hold all its arcs, the product that of
    the CSR.  `edge`: rows of ka_max - 1, ka_max and ka_max + 1 arcs in a graph whose cheapest plan has the cap at the window
    take 1, 1 and 2 lanes.  `exchange`: the teams' window of 36 slots and a graph whose last segment finds a wave only after two
    others traded places (RowGraph::exchanges >= 1).

    The walk packs with options of its own (every cap, group speeds of 1, no backward lag), not with those the engine builds.
    The shipped team forms set RowPackOpts::every_cap = false, which also switches the exchange off, so they never take that
    path: the `exchange` case, at the teams' window of 36 slots but with every_cap set, is the only check of what the exchange
    leaves behind at that window.  The pair forms (window of 44) are the ones that can reach it in the library."""
    r = subprocess.run([plan_check, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
