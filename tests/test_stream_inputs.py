"""The inputs of tests/test_gpu_stream_instances.py, checked without a GPU: the structure of the fixtures of tests/stream_cases.py,
and -- from the float64 oracle alone -- that the mistakes those GPU tests are there to catch would show in the comparison they use
(check_gamma, unchanged): an emission staged from the wrong column at the end of the last 64-lane pass, a lane of a row's group or a
pass of a whole-wave row that is lost, a state near the form's limit whose offset is cut."""
import numpy as np
import pytest

import arc_reference as ar
import graphs
import stream_cases as sc
from test_gpu_parity import check_gamma
from test_itemform_inputs import gamma_error_over_bars


def _gamma(oracle, g, V, lens):
    return sc.reference(oracle, graphs, [g] * V.shape[0], V, lens)[0]


def _assert_visible(what, mutated, base, lens):
    a, l = gamma_error_over_bars(mutated, base)
    print(f"{what}: abs criterion at {a:.3g} of its bar, log-posterior criterion at {l:.3g} of its bar")
    with pytest.raises(AssertionError):
        check_gamma(mutated, base, lens)


def test_stream_nj_steps():
    assert [sc.stream_nj(P) for P in sc.P_EDGES] == [2, 4, 4, 8, 8, 16, 16]


def test_mid_row_graph_structure(wl):
    g = sc.mid_row_graph(wl)
    assert 900 <= g.S <= 1500 and g.P == 127
    hin, hout = sc.mid_hubs()
    for d, (deg, hubs) in enumerate(zip(sc.degrees(g), (hin, hout))):
        assert (deg[hubs] == sc._HUB_ROWS).all(), (d, deg[hubs])
        for width in sc.EDGE_ROWS:
            assert (deg == width).any(), (d, width)
        assert ((deg >= 33) & (deg <= 64)).sum() >= 8 and ((deg >= 65) & (deg <= 128)).sum() >= 8 and (deg > 128).sum() >= 5
        # teams of 4: the rows go to the sets round-robin by decreasing length -- five whole-wave rows give every set one and one set two
        assert np.sort(deg)[::-1][4] > 128
    # the hubs have pdfs of their own and are initial states
    s2p = np.asarray(g.state2pdf)
    hubs = np.concatenate([hin, hout])
    assert np.isin(hubs, g.init_idx).all() and all((s2p == s2p[h]).sum() == 1 for h in hubs)


def test_empty_pdf_graph_structure(wl):
    g = sc.empty_pdf_graph(wl)
    assert g.S == 320 and g.P == 300
    empty = np.setdiff1d(np.arange(g.P), g.state2pdf)
    assert empty.tolist() == list(sc.EMPTY_PDFS) and len(empty) >= 20 and {0, 150, g.P - 1} <= set(empty.tolist())


@pytest.mark.parametrize("S1", [sc.S1_LIMIT, sc.S1_LIMIT + 1])
def test_limit_graph_structure(mm, wl, S1):
    g = sc.limit_graph(wl, S1)
    cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    assert cf.S1 == S1 and g.P == 1000
    assert g.init_idx.size >= g.S / 4 and 0.25 <= g.final_idx.size / g.S <= 0.35
    assert 3.0 <= g.src.size / g.S <= 4.5  # (mean degree 3 and the chain)


@pytest.mark.parametrize("P", sc.P_EDGES)
def test_the_last_pdf_carries_mass(wl, oracle, P):
    """pdf P - 1 and pdf 64 (NJ - 1) (sc.last_pass_pdf where that pass holds no pdf), the two ends of the last staging pass, reach gamma >= 5e-3 in some frame (the bar of
    test_itemform_inputs.py); emissions with column P - 1 read from column P - 2 fail check_gamma."""
    g, V, lens = sc.case_p(wl, P)
    assert g.S == (1200 if P >= 512 else 600) and g.P == P
    s2p = np.asarray(g.state2pdf)
    q = sc.last_pass_pdf(P)
    assert q == 64 * (sc.stream_nj(P) - 1) or (P in (128, 256, 512) and q == P - 64)
    assert s2p[0] == P - 1 and (s2p == q).any()
    base = _gamma(oracle, g, V, lens)
    top = base[:, :, [P - 1, q]].max(axis=(0, 1))
    print(f"P = {P}: the largest gamma of pdf {P - 1}: {top[0]:.3g}, of pdf {q}: {top[1]:.3g}")
    assert (top >= 5e-3).all(), top
    Vm = V.copy()
    Vm[..., P - 1] = V[..., P - 2]
    _assert_visible(f"P = {P}, column {P - 1} staged from column {P - 2}", _gamma(oracle, g, Vm, lens), base, lens)


def test_lost_arcs_of_grouped_rows_are_visible(wl, oracle):
    """mid_row_graph without the last arc of every row of 33, 64, 65, 128 or 129 arcs (a lane of a group that is not added, a row cut
    at a class boundary) fails check_gamma -- all at once as well as per length and direction; so does a whole-wave sum that keeps
    its first pass only."""
    g, V, lens = sc.case_r(wl)
    base = _gamma(oracle, g, V, lens)
    _assert_visible("last arcs of the rows of 33, 64, 65, 128, 129", _gamma(oracle, sc.without_last_arcs(g, (33, 64, 65, 128, 129)), V, lens), base, lens)
    for d in (0, 1):
        for width in (33, 64, 65, 128, 129):
            mut = sc.without_last_arcs(g, (width,), (d,))
            assert g.src.size + g.final_idx.size - mut.src.size - mut.final_idx.size == (sc.degrees(g)[d] == width).sum()
            _assert_visible(f"direction {d}, last arc of the rows of {width}", _gamma(oracle, mut, V, lens), base, lens)
    mut = sc.first_pass_only(g)
    assert (np.minimum(sc.degrees(mut)[0][: g.S], 65) <= 64 + (sc.degrees(g)[0][: g.S] <= 128)).all()
    _assert_visible("rows of more than 128 arcs cut to 64", _gamma(oracle, mut, V, lens), base, lens)


def test_mass_at_the_state_limit(wl, oracle):
    """limit_graph(16370) with the case's V: at frame 2 of the full-length utterance at least 90 % of the states hold a state posterior
    above 1e-12 (the oracle's state_A * state_B over their sum) -- the gathers of frame 3 read live values at offsets all over the
    16 bits.  A condition on the reference alone."""
    o, oc = oracle
    g, V, lens = sc.case_s(wl, sc.S1_LIMIT)
    Vhat = ar.expand_log(V[0].astype(np.float64), int(lens[0]), V.shape[1])
    _, _, A, B = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64, want_ab=True)
    ab = A[:, 1] + B[:, 1]
    post = np.exp(ab - np.logaddexp.reduce(ab))
    live = (post[: g.S] > 1e-12).mean()
    print(f"limit graph, frame 2: {100 * live:.1f} % of the states above 1e-12")
    assert live >= 0.9
    assert (post[g.S - 64 : g.S] > 1e-12).any() and (post[:64] > 1e-12).any()
