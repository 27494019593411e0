"""The inputs of tests/test_gpu_wave_lane_instances.py, checked without a GPU: the structure of the fixtures of tests/wave_cases.py,
which of them the wave form takes (the host packer: CompiledFSM.wave_product), and -- from the float64 oracle alone -- that the
mistakes those GPU tests are there to catch would show in the comparison they use (check_gamma, unchanged): an emission staged from
the wrong column at the end of the last 64-lane pass, a lane of a row's group that is lost, a pdf whose sum is dropped, a length at
which no path exists, an input the lane kernel's float64 recursion cannot hold."""
import numpy as np
import pytest

import graphs
import stream_cases as sc
import wave_cases as wc
from test_gpu_parity import GAMMA_FLOOR, check_gamma
from test_itemform_inputs import gamma_error_over_bars


def _ref(oracle, g, V, lens, key=None):
    """(gamma, ttl) of the float64 oracle; the utterances without a path (ttl = -inf: the oracle's gamma is 0 / 0 there) as zeros."""
    gam, ttl = wc.reference(oracle, graphs, [g] * V.shape[0], V, lens, key)
    none = ~np.isfinite(ttl)
    assert np.isneginf(ttl[none]).all() and np.isfinite(gam[~none]).all()
    gam = gam.copy()
    gam[none] = 0.0
    return gam, ttl


def _assert_visible(what, mutated, base, lens):
    a, l = gamma_error_over_bars(mutated, base)
    print(f"{what}: abs criterion at {a:.3g} of its bar, log-posterior criterion at {l:.3g} of its bar")
    with pytest.raises(AssertionError):
        check_gamma(mutated, base, lens)
    return a, l


def float32_over_bars(oracle, g, V, lens, key):
    """The float32 mode of the oracle's own recursion against its float64 mode on one case, as ratios to check_gamma's two bars
    (gamma_error_over_bars): what float32 arithmetic in the reference's order of operations loses on this input."""
    def make():
        o, oc = oracle
        g64, t64 = wc.reference(oracle, graphs, [g] * V.shape[0], V, lens, key)
        g32, _ = oc.batch_shared(graphs.to_oracle(o, g, dtype=np.float32), g.state2pdf, g.P, V, lens, dtype=np.float32)
        assert np.isfinite(t64).all()
        return gamma_error_over_bars(np.asarray(g32, dtype=np.float64), g64)
    return wc._memo(("f32bars", key), make)


def _products_agree(mm, wl, g):
    """wave_product against packed_product in both directions, at the bar of test_host_logic.py::test_wave_form_products."""
    cf = wc.compile_graph(mm, wl, g)
    rng = np.random.default_rng(5)
    x = (3 * rng.standard_normal(cf.S1)).astype(np.float32)
    x[rng.random(cf.S1) < 0.1] = -np.inf
    for d in (0, 1):
        ref, _ = cf.packed_product(x, d)
        out, stats = cf.wave_product(x, d)
        m = np.isfinite(ref)
        assert np.array_equal(np.isfinite(out), m), (g.name, d)
        assert np.allclose(out[m], ref[m], rtol=1e-5, atol=2e-5), (g.name, d)
        assert stats[0] <= 16 and stats[1] <= 16
    return cf


def _refused(mm, wl, g):
    cf = wc.compile_graph(mm, wl, g)
    for d in (0, 1):
        with pytest.raises(mm.MarkovModelsAMDError):
            cf.wave_product(np.zeros(cf.S1, dtype=np.float32), d)
    return cf


# ---- the pdf count
@pytest.mark.parametrize("P", wc.P_EDGES)
def test_mass_on_the_edge_pdfs(mm, wl, oracle, P):
    """pdf P - 1 and pdf 64 floor((P - 1) / 64), the two ends of the last 64-lane pass of em_stage / frame_out, reach gamma >= 0.05 in
    some frame; emissions with column P - 1 read from column P - 2 fail check_gamma."""
    g, V, lens = wc.pdf_edge_case(wl, P)
    assert 200 <= g.S <= 999 and g.P == P and wc.wave_segments(mm, wl, g) is not None
    q = wc.last_pass_pdf(P)
    s2p = np.asarray(g.state2pdf)
    assert s2p[0] == P - 1 and (s2p == q).any() and q == {63: 0, 64: 0, 127: 64, 128: 64, 249: 192}[P]
    base = _ref(oracle, g, V, lens)[0]
    top = base[:, :, [P - 1, q]].max(axis=(0, 1))
    print(f"P = {P}: the largest gamma of pdf {P - 1}: {top[0]:.3g}, of pdf {q}: {top[1]:.3g}")
    assert (top >= 0.05).all(), top
    Vm = V.copy()
    Vm[..., P - 1] = V[..., P - 2]
    _assert_visible(f"P = {P}, column {P - 1} staged from column {P - 2}", _ref(oracle, g, Vm, lens)[0], base, lens)


@pytest.mark.parametrize("name", ["perm64", "many_to_one_64", "empty_last_64"])
def test_pdf_63_of_the_lane_maps(wl, oracle, name):
    """The state maps on exactly 64 pdfs: none is the identity; pdf 63 -- whose loop bound is entry 64 of the kernel's table -- reaches
    gamma >= 0.05 in perm64 and many_to_one_64, and is exactly 0 in empty_last_64."""
    g = getattr(wc, name)(wl)
    V, lens = wc.map64_case(wl, g)
    s2p = np.asarray(g.state2pdf)
    n = np.bincount(s2p, minlength=64)
    assert g.P == 64 and g.S <= 64 and not np.array_equal(s2p, np.arange(g.S))
    base = _ref(oracle, g, V, lens)[0]
    top = float(base[:, :, 63].max())
    print(f"{name}: {n[63]} states on pdf 63, its largest gamma: {top:.3g}; {int((n == 0).sum())} pdfs without a state")
    if name == "perm64":
        assert sorted(s2p.tolist()) == list(range(64)) and s2p[0] == 63 and 0 in g.init_idx
    elif name == "many_to_one_64":
        assert g.S == 40 and n[63] == 3 and n[0] == 0 and (n == 0).sum() >= 10 and s2p[0] == 63 and 0 in g.init_idx
    if name == "empty_last_64":
        assert n[63] == 0 and top == 0.0
    else:
        assert top >= 0.05
        Vm = V.copy()
        Vm[..., 63] = V[..., 62]
        _assert_visible(f"{name}, column 63 read from column 62", _ref(oracle, g, Vm, lens)[0], base, lens)


# ---- rows of every lane-group width
@pytest.mark.parametrize("widest", [255, 256])
def test_hub_graph_structure_and_products(mm, wl, widest):
    g = wc.hub_graph(wl, widest)
    assert g.S + 1 <= 1023
    hin, hout = wc.hub_ids()
    din, dout = sc.degrees(g)
    assert din[hin].tolist() == list(wc.HUB_ROWS[:-1]) + [widest] and dout[hout].tolist() == list(wc.HUB_ROWS)
    assert max(din.max(), dout.max()) == widest
    s2p = np.asarray(g.state2pdf)
    hubs = np.concatenate([hin, hout])
    assert np.isin(hubs, g.init_idx).all() and all((s2p == s2p[h]).sum() == 1 for h in hubs)
    _products_agree(mm, wl, g)


def test_lost_arcs_of_hub_rows_are_visible(wl, oracle):
    """hub_graph without the last arc of the hub row of one width in one direction fails check_gamma against the intact graph's
    reference, for every width and direction."""
    g, V, lens = wc.hub_case(wl)
    base = _ref(oracle, g, V, lens)[0]
    seen = []
    for d in (0, 1):
        for width in wc.HUB_ROWS:
            mut = sc.without_last_arcs(g, (width,), (d,))
            lost = g.src.size + g.final_idx.size - mut.src.size - mut.final_idx.size
            assert lost == (sc.degrees(g)[d] == width).sum() and lost >= 1
            a, l = _assert_visible(f"direction {d}, last arc of the rows of {width}", _ref(oracle, mut, V, lens)[0], base, lens)
            assert l > 1.0  # (the log-posterior bar itself, not the absolute one alone)
            seen.append((l, d, width))
    l, d, width = min(seen)
    print(f"the least visible mutant: direction {d}, width {width}, at {l:.3g} of the log-posterior bar")


# ---- pdfs of every group width
@pytest.mark.parametrize("variant", ["base", "five", "five_p130"])
def test_every_pdf_group_carries_mass(mm, wl, oracle, variant):
    g, V, lens = wc.pdf_group_case(wl, variant)
    n = np.bincount(np.asarray(g.state2pdf), minlength=g.P)
    sizes = wc.PDF_GROUPS + ((129,) if variant != "base" else ())
    assert sorted(n[n > 0].tolist()) == sorted(sizes)
    empty = wc.pdf_group_empty(g)
    assert {0, g.P - 1} <= set(empty.tolist()) and ((empty > 0) & (empty < g.P - 1)).any()
    assert wc.pdf_group_lanes(g) == (255 if variant == "base" else 319) and wc.pdf_segments(g) == (4 if variant == "base" else 5)
    assert g.P <= 127 or variant == "five_p130" and g.P >= 128 and n[128:].sum() > 0
    assert wc.wave_segments(mm, wl, g)[0] == 4
    base = _ref(oracle, g, V, lens)[0]
    top = base.max(axis=(0, 1))
    print(f"{variant}: the smallest of the pdfs' largest gammas: {top[n > 0].min():.3g} (a pdf of {n[n > 0][top[n > 0].argmin()]} states)")
    assert (top[n > 0] > GAMMA_FLOOR).all() and (base[:, :, empty] == 0).all()


# ---- which graphs the form takes
def test_which_graphs_fit_the_wave_form(mm, wl):
    """At the value: a row of 256 arcs (64 lanes of 4 arc slots), a pdf of 256 states, 4 and 5 .. 8 pdf segments, 1023 and 1024 states
    (16 full segments); one beyond each is refused -- a row of 257 arcs, a pdf of 257 states, 9 pdf segments, 1025 states."""
    _refused(mm, wl, wc.hub_graph(wl, 257))
    _refused(mm, wl, wc.pdf_group_graph(wl, "pdf257"))
    nine, fits = wc.pdf_group_graph(wl, "nine"), wc.pdf_group_graph(wl, "nine_fits")
    assert wc.pdf_group_lanes(nine) > 512 and wc.pdf_segments(nine) == 9 and nine.S + 1 <= 1023 and nine.P <= 249
    _refused(mm, wl, nine)
    assert np.array_equal(nine.src, fits.src) and np.array_equal(nine.w, fits.w) and wc.pdf_segments(fits) <= 8
    _products_agree(mm, wl, fits)
    for S1 in wc.LIMIT_S1:
        g = wc.limit_chain(wl, S1)
        assert max(d.max() for d in sc.degrees(g)) <= 4
        assert _products_agree(mm, wl, g).S1 == S1
    assert _refused(mm, wl, wc.limit_chain(wl, 1025)).S1 == 1025
    for g in wc.tiny_for_wave(wl):
        assert wc.wave_segments(mm, wl, g) == (2, [1, 1])  # (one segment: three of an agent's four compute waves own none)
    assert wc.wave_segments(mm, wl, wc.sparse20(wl))[0] == 2 and wc.wave_segments(mm, wl, wc.four_segment(wl))[0] == 4
    assert wc.wave_segments(mm, wl, wc.dense_wide(wl))[1] > [8, 8]
    # the pdf count: 255 pdfs (P1 = 256) are the most the form takes
    assert wc.wave_segments(mm, wl, wc.pdf_edge_graph(wl, 255)) is not None
    _refused(mm, wl, wc.pdf_edge_graph(wl, 256))


@pytest.mark.parametrize("S1", wc.LIMIT_S1 + (1025,))
def test_float32_on_the_long_chains(wl, oracle, S1):
    """limit_case runs N = S1 + 8 frames on a left-to-right chain: 519 .. 1033 dependent steps.  The oracle's own recursion in float32
    misses check_gamma's bars against its float64 mode there -- the measure of what the float32 wave kernel can be asked for at
    these lengths (the GPU test takes 4 times these ratios where the kernel needs more than the bars themselves)."""
    g, V, lens = wc.limit_case(wl, S1)
    assert V.shape[1] == S1 + 8 and lens[0] == S1 + 8 and len(lens) == 2
    a, l = float32_over_bars(oracle, g, V, lens, f"W4_chain{S1}")
    print(f"chain{S1}: the oracle in float32 against float64: abs criterion at {a:.3g} of its bar, log-posterior criterion at {l:.3g} of its bar")
    assert a > 1.0


# ---- the lengths
@pytest.mark.parametrize("which", ["wave2", "wave4", "lane16", "lane64"])
def test_lengths_have_a_path_or_none(wl, oracle, which):
    """One utterance per length: the reference's ttl is finite exactly where an accepting path of that many frames exists -- from the
    graph's shortest path on, every length --, and -inf below: there the GPU tests' assertion on exact zeros applies."""
    g = {"wave2": wc.sparse20, "wave4": wc.four_segment, "lane16": lambda w: wc.lane_dense(w, 16), "lane64": lambda w: wc.lane_sparse(w, 64)}[which](wl)
    lens = wc.WAVE_LENS if which.startswith("wave") else wc.LANE_LENS
    V, lens = wc.lengths_case(wl, g, lens, 70)
    gam, ttl = _ref(oracle, g, V, lens, ("lengths", which))
    has = wc.path_lengths(g, int(lens.max()))
    shortest = int(np.flatnonzero(has)[0])
    assert has[shortest:].all()
    print(f"{which}: the shortest path has {shortest} frames; {int((lens < shortest).sum())} lengths without a path")
    assert np.array_equal(np.isfinite(ttl), lens >= shortest) and np.isneginf(ttl[lens < shortest]).all()
    if which == "lane64":
        assert not np.array_equal(np.asarray(g.state2pdf), np.arange(g.S)) and np.bincount(g.state2pdf).max() > 1


# ---- an input beyond the float64 linear recursion
def test_redo_case_is_beyond_the_lane_recursion(wl, oracle):
    """redo_case, utterance 0: the lane kernel's forward recursion emulated in float64 (normalised by the power of two of the last
    vector's maximum, flushed below 2^-1022) ends with Z = 0 -- the values of the one path are flushed --, while the log-domain
    oracle's ttl is finite.  Utterance 1 (N(0, 1.3) emissions) loses nothing."""
    g, V, lens = wc.redo_case(wl)
    assert g.S == 64 and g.P == 64 and V.shape[1] == 64 and V[0].max() - V[0].min() == 250.0
    gam, ttl = _ref(oracle, g, V, lens, "redo")
    Z0, lost0 = wc.lane_forward_emulated(g, V[0], 64)
    Z1, lost1 = wc.lane_forward_emulated(g, V[1], 64)
    print(f"redo case: emulated Z {Z0} with {lost0} values flushed against the oracle's ttl {ttl[0]:.6g}; utterance 1: Z {Z1:.3g}, {lost1} flushed")
    assert Z0 == 0.0 and lost0 >= 1 and np.isfinite(ttl[0]) and ttl[0] < -250.0 * 62
    assert Z1 > 0.0 and lost1 == 0 and np.isfinite(ttl[1])
    assert np.isneginf(ttl[2:]).all()
    # the one path: state t at frame t
    assert np.allclose(gam[0][np.arange(64), np.arange(64)], 1.0)
