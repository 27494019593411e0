"""The inputs of tests/test_gpu_exact_instances.py (tests/exact_cases.py), checked without a GPU from the float64 oracle and numpy
alone -- none of the library's kernels runs here.

What the GPU tests rely on:
  * an utterance has a path through its graph exactly when it has 2 or more frames, on every graph and length list of
    exact_cases.all_cases(), so that "only utterances of fewer than 2 frames are left out of a comparison" is a fact about the
    inputs; every case has an utterance of the full N frames;
  * the sharp emissions are beyond float32's range within a frame (see test_sharp_emissions_are_beyond_float32 for what holds at
    which pdf count).

And that the comparison the GPU tests use (check_gamma of test_gpu_parity.py, on the float32 cast of a float64 result) would see
the faults the shapes are there for.  "Visible": check_gamma raises for the mutated reference and passes for the reference itself.
  * the service wave's last pass over the pdfs dropped (pdfs 64 (NJ - 1) .. P - 1 read as 0) -- wherever that pass holds a pdf;
  * the two utterances of a pair swapped;
  * on the sharp inputs, float32's exponent range in place of the tier's: every alpha * beta term more than 126 log2 below its
    frame's scale (the largest alpha times the largest beta of the frame, what a linear-domain kernel scales a frame by) flushed
    to 0, the frame normalised by what is left."""
import numpy as np
import pytest

import arc_reference as ar
import exact_cases as ec
from test_gpu_parity import check_gamma

_graphs, _refs = {}, {}
CASES = ec.all_cases()
GRAPH_NAMES = list(dict.fromkeys(c[0] for c in CASES))
# graph -> NJ of its float64 instance
NJ = {**{n: t["f64"] for n, t in ec.GROUP_A.items()}, **{f"p1_{p}": t["f64"] for p, t in ec.BOUNDARIES.items()}, **{n: t[0] for n, t in ec.TEAMS.items()}}


def graph(wl, gname):
    if gname not in _graphs:
        _graphs[gname] = ec.GRAPHS[gname](wl)
    return _graphs[gname]


def case_ref(oracle, wl, gname, key, inputs):
    g = graph(wl, gname)
    V, lens = inputs(g)
    return g, V, lens, ec.reference(_refs, oracle, g, (gname,) + key, V, lens)


def visible(g_mut, g_ref, lens):
    ok = lens >= 2
    try:
        check_gamma(g_mut[ok].astype(np.float32), g_ref[ok], lens[ok])
    except AssertionError:
        return True
    return False


def test_the_cases_cover_the_tables():
    assert set(GRAPH_NAMES) == set(ec.GROUP_A) | {f"p1_{p}" for p in (*ec.BOUNDARIES, 507)} | set(ec.TEAMS)
    assert sorted((nj, H) for nj, H, _ in ec.TEAMS.values()) == sorted((nj, H) for H in (2, 4, 8) for nj in (2, 4, 5 if H == 8 else 8))
    assert {(nj, H) for nj, H, wide in ec.TEAMS.values() if wide} == {(2, 2), (4, 2)}
    shapes = ec.SHAPES + ec.TEAM_SHAPES + [ec.BOUNDARY_SHAPE, ec.BEHIND_SHAPE]
    assert max(s[0] for s in shapes) <= 3 and max(s[1] for s in shapes) <= 9 and all(len(s[2]) == s[0] and max(s[2]) == s[1] for s in shapes)
    assert {s[0] for s in ec.SHAPES} == {1, 2, 3} and {s[1] for s in ec.SHAPES} == {2, 3, 4, 5, 6, 9}


@pytest.mark.parametrize("gname", GRAPH_NAMES)
def test_a_path_exactly_from_two_frames(mm, wl, oracle, gname):
    """np.isfinite(ttl) == (lens >= 2) from the oracle, for every case of the graph; an utterance of N frames in each; the pdf
    counts the graph is there for."""
    g = graph(wl, gname)
    if gname in NJ:
        nj, H = NJ[gname], ec.TEAMS.get(gname, (0, 1))[1]
        assert {2: g.P + 1 <= 128, 4: 128 < g.P + 1 <= 250, 5: H == 8 and 250 < g.P + 1 <= 314, 8: H < 8 and 250 < g.P + 1 <= 506}[nj]
    n = 0
    for name, key, inputs in CASES:
        if name != gname:
            continue
        _, V, lens, (g_ref, t_ref) = case_ref(oracle, wl, gname, key, inputs)
        assert V.dtype == np.float32 and V.shape == (len(lens), V.shape[1], g.P)
        assert np.array_equal(np.isfinite(t_ref), lens >= 2), (key, lens, t_ref)
        assert lens.max() == V.shape[1] and V.shape[1] <= 9 and len(lens) <= 3
        assert not np.isnan(g_ref[lens >= 2]).any()
        assert not visible(g_ref, g_ref, lens)  # (the reference itself, cast to float32, meets the bar)
        n += 1
    assert n >= 2


def test_structure_of_the_graphs(wl):
    holes, loop, small = graph(wl, "holes"), graph(wl, "loop"), graph(wl, "small")
    count = np.bincount(holes.state2pdf, minlength=holes.P)
    assert holes.P == 41 and count[40] == 0 and count[3] == 1  # a pdf without a state, a pdf of one state
    assert np.bincount(loop.state2pdf, minlength=loop.P).min() >= 40 and loop.S == 600  # ~60 states per pdf
    assert small.S + 1 <= 127  # (the instances for graphs of up to 127 states: a vector shorter than one pass of the scans)
    for P1 in (128, 250, 506):  # (the odd P: one pdf more than the states use)
        g = graph(wl, f"p1_{P1}")
        assert g.P + 1 == P1 and int(np.max(g.state2pdf)) < g.P - 1
    assert graph(wl, "wsj_size_200").S == graph(wl, "wsj_den").S == 3032


def group_of(gname, key):
    if key[0] in ("partner", "behind"):
        return "B" if key[0] == "partner" else "C"
    return "D" if gname in ec.TEAMS else ("A" if gname in ec.GROUP_A else "boundaries")


def test_sharp_emissions_are_beyond_float32(wl):
    """peaky(rng, shape, 25.0) - 300.0 is a log-softmax of 25 N(0,1), so a frame spans 25 times the range of P normal draws.  In
    every group of tests the sharp inputs span more than 150 nats within a frame, and on every graph more than float32's whole
    exponent range (126 log2 = 87.3 nats).  The 150 nats are asserted per group and not per graph or tensor: six standard
    deviations between the extremes of one frame take a few hundred draws -- over 10 pdfs (the 60-states-per-pdf graph) a frame spans
    77 nats on average and 1 of 100 tensors tried reached 150, over 127 pdfs 4 of 5 tensors of 18 frames did.  Only the frames within
    an utterance's length count.  The figure of every graph is printed."""
    by_graph, by_group = {}, {}
    for gname, key, inputs in CASES:
        if key[0] not in ("sharp", "partner", "behind"):
            continue
        g = graph(wl, gname)
        V, lens = inputs(g)
        sharp = np.flatnonzero(V.reshape(len(lens), -1).max(1) < -250.0)  # (the utterances at the -300 offset)
        assert sharp.size == (len(lens) if key[0] == "sharp" else int(key == ("partner", "sharp") or key[0] == "behind"))
        for b in sharp:
            W = V[b, : lens[b]]
            assert np.isfinite(W).all()
            span = float((W.max(-1) - W.min(-1)).max()) if lens[b] else 0.0
            by_graph[gname] = max(by_graph.get(gname, 0.0), span)
            by_group[group_of(gname, key)] = max(by_group.get(group_of(gname, key), 0.0), span)
    for gname, span in by_graph.items():
        print(f"{gname}: P = {graph(wl, gname).P}, largest span of a frame over the sharp cases {span:.1f} nats")
    print(by_group)
    assert set(by_graph) == set(GRAPH_NAMES) and set(by_group) == {"A", "boundaries", "B", "C", "D"}
    assert min(by_graph.values()) > 126 * np.log(2.0)
    assert min(by_group.values()) > 150.0


# ---- the faults the shapes are there for
@pytest.mark.parametrize("gname", list(NJ))
def test_a_dropped_last_pdf_pass_is_visible(mm, wl, oracle, gname):
    """Where the last pass holds pdfs with states: every plain case sees it dropped (the frames no longer sum to 1).  A sharp case
    sees it only if one of those few pdfs holds a posterior the bar looks at; how many do is printed."""
    g = graph(wl, gname)
    first = 64 * (NJ[gname] - 1)
    held = first < g.P and bool(np.bincount(g.state2pdf, minlength=g.P)[first:].any())
    seen = {"plain": [0, 0], "sharp": [0, 0]}
    for name, key, inputs in CASES:
        if name != gname or key[0] not in ("plain", "sharp"):
            continue
        _, V, lens, (g_ref, _) = case_ref(oracle, wl, gname, key, inputs)
        mut = np.array(g_ref)
        mut[..., first:] = 0
        if not held:  # (10, 12, 40, 41 pdfs at NJ = 2; 128 at NJ = 4; 250 and 400 at NJ = 8: the last pass holds idle lanes only)
            assert np.array_equal(np.nan_to_num(mut), np.nan_to_num(g_ref))
            continue
        seen[key[0]][0] += visible(mut, g_ref, lens)
        seen[key[0]][1] += 1
    print(gname, "NJ", NJ[gname], "pdfs", g.P, "last pass holds pdfs:", held, "cases that see it dropped (seen, all):", seen)
    assert not held or (seen["plain"][0] == seen["plain"][1] >= 1)


def test_the_last_pass_holds_pdfs_at_every_nj(wl):
    """... and at every NJ the last pass of some graph does hold pdfs with states, one workgroup and teams alike."""
    def full(gname):
        g = graph(wl, gname)
        return bool(np.bincount(g.state2pdf, minlength=g.P)[64 * (NJ[gname] - 1):].any())

    for gname in ("p1_128", "wsj_den", "lfmmi_3400_84", "lfmmi_5000_100", "nj4", "p1_250", "wsj_size_200", "lfmmi_3600_200", "lfmmi_5000_200",
                  "lfmmi_6000_300", "p1_506"):
        assert full(gname), gname
    assert {NJ[n] for n in NJ if full(n)} == {2, 4, 5, 8}


@pytest.mark.parametrize("gname", GRAPH_NAMES)
def test_swapped_utterances_of_a_pair_are_visible(mm, wl, oracle, gname):
    n = 0
    for name, key, inputs in CASES:
        if name != gname:
            continue
        _, V, lens, (g_ref, _) = case_ref(oracle, wl, gname, key, inputs)
        if len(lens) < 2 or lens[0] < 2 or lens[1] < 2:
            continue
        mut = np.array(g_ref)
        mut[[0, 1]] = mut[[1, 0]]
        assert visible(mut, g_ref, lens), (gname, key)
        n += 1
    assert n >= 1


def flushed_to_float32_range(oracle, g, V, L):
    """gamma [N, P] of one utterance from the oracle's float64 alpha and beta with every term alpha_s beta_s more than 126 log2 below
    its frame's scale (max alpha * max beta) flushed to 0, and the same without the flush (the oracle's gamma again)."""
    N = V.shape[0]
    _, _, A, Bm = oracle[1].single(ec.oracle_fsm(oracle, g), g.state2pdf, g.P, ar.expand_log(V, L, N), dtype=np.float64, want_ab=True)
    s2p = ar._s2p_full(g)
    out = np.zeros((2, N, g.P))
    for n in range(L):
        t = A[:, n] + Bm[:, n]
        scale = A[:, n].max() + Bm[:, n].max()
        for i, keep in enumerate((t - scale >= -126 * np.log(2.0), np.isfinite(t))):
            if keep.any():
                w = np.where(keep, np.exp(t - t[keep].max()), 0.0)
                out[i, n] = np.bincount(s2p, weights=w / w.sum(), minlength=g.P + 1)[: g.P]
    return out[0], out[1]


@pytest.mark.parametrize("gname", GRAPH_NAMES)
def test_float32_exponent_range_is_visible_on_the_sharp_inputs(mm, wl, oracle, gname):
    """Every utterance of 2 or more frames of the graph's sharp cases; the plain ones as the control: there the flush changes nothing
    the bar sees.  With 2 to 9 frames not every sharp utterance drives the forward and the backward mass 126 log2 apart: the count
    of those that do is printed, and at least one per graph must.  The exception is the 100-state graph of 12 pdfs and 20 arcs per
    state, on which none of the 10 does: it is there for its short vector, and group A sees this fault on its five other graphs."""
    g = graph(wl, gname)
    seen = {"plain": [0, 0], "sharp": [0, 0]}
    for name, key, inputs in CASES:
        if name != gname or key[0] not in ("plain", "sharp"):
            continue
        _, V, lens, (g_ref, _) = case_ref(oracle, wl, gname, key, inputs)
        for b in np.flatnonzero(lens >= 2):
            flushed, whole = flushed_to_float32_range(oracle, g, V[b].astype(np.float64), int(lens[b]))
            assert np.allclose(whole, g_ref[b], rtol=1e-9, atol=1e-300)
            assert not visible(whole[None], g_ref[b : b + 1], lens[b : b + 1])
            seen[key[0]][0] += visible(flushed[None], g_ref[b : b + 1], lens[b : b + 1])
            seen[key[0]][1] += 1
    print(gname, "utterances on which float32's range is visible (seen, all):", seen)
    assert seen["plain"][0] == 0 and (seen["sharp"][0] >= 1 or gname == "small")
