"""The inputs of tests/test_gpu_quad_instances.py, checked without a GPU: that the statements of tests/quad_cases.py about what a case
reaches (quads per direction, the numbering, the kind of every row, the rows on virtual lanes, the rows beyond the register-carried
ones) agree with the host packer where it exposes them (CompiledFSM.quad_product: quads and lanes; the products through the form
against the item form), and -- from the float64 oracle alone -- that the rows, pdfs and frames a case is there for carry posterior
mass above check_gamma's floor, that every utterance meant to have a path has one, and that the inputs of the fallback cases really
spread a frame's vector over more than the 62 nats below which a linear sum takes the exact fallback."""
import numpy as np
import pytest

import graphs
import quad_cases as qc
from test_gpu_parity import GAMMA_FLOOR


def _compile(mm, wl, g):
    return mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))


def _packer_agrees(mm, wl, g, kqs):
    """The graph is trim (the kernel forms then hold every state: the rows are the graph's degrees); for every KQ the packer counts
    the quads and lanes quad_cases states, numbers the rows as quad_cases.numbering does and records for every row the lane ends
    quad_cases.row_records derives (CompiledFSM.quad_layout), and the product through the quad form -- row_short and row_long over
    those lane ends -- equals the item form's (the bar of test_host_logic.py::test_quad_form_products)."""
    assert qc.is_trim(g), g.name
    cf = _compile(mm, wl, g)
    assert cf.S1 == g.S + 1
    rng = np.random.default_rng(5)
    x = (3 * rng.standard_normal(cf.S1)).astype(np.float32)
    x[rng.random(cf.S1) < 0.1] = -np.inf
    nq = qc.quads(g)
    for d in (0, 1):
        ref, _ = cf.packed_product(x, d)
        m = np.isfinite(ref)
        for KQ in kqs:
            out, stats = cf.quad_product(x, d, KQ)
            assert (int(stats[0]), int(stats[1])) == (nq[d], -(-nq[d] // KQ)), (g.name, d, KQ, stats[:2], nq)
            assert np.array_equal(np.isfinite(out), m) and np.allclose(out[m], ref[m], rtol=1e-5, atol=2e-5), (g.name, d, KQ)
            # the placement row by row: the numbering, and every row's record (last quad, lane ends, short or long, pdf)
            order, recs = cf.quad_layout(d, KQ)
            assert np.array_equal(order, qc.numbering(g, d)), (g.name, d, KQ)
            assert np.array_equal(recs.astype(np.int64), qc.row_records(g, d, KQ)), (g.name, d, KQ)
    return cf


def _finite_ttl(oracle, g, V, lens, key, dead=()):
    """The float64 reference of the case; every utterance of at least one frame that is not listed in `dead` has a finite ttl, the
    others -inf."""
    gam, ttl = qc.reference(oracle, graphs, [g] * V.shape[0], V, lens, key)
    lens_ = np.full(V.shape[0], V.shape[1]) if lens is None else np.asarray(lens)
    alive = np.ones(V.shape[0], dtype=bool)
    alive[list(dead)] = False
    assert np.isfinite(ttl[alive]).all() and np.isneginf(ttl[~alive]).all(), (g.name, ttl)
    assert (lens_[alive] >= 1).all()
    return gam, ttl


def _row_mass(oracle, g, V, lens, key):
    """[S + 1] the largest posterior of every state over the batch (the phony final state: 0, it has no frame of its own)."""
    gs = qc.state_posteriors(oracle, graphs, g, V, lens, key)
    return np.append(gs.max(axis=(0, 1)), 0.0)


# ---- 1: every KQ
def test_mixed_graph_reaches_every_instance(mm, wl, oracle):
    """mixed300: both RPT values over all 18 KQ -- RPT 2 at the engine's wave count, RPT 3 with rows in the generic loop at one wave
    (S1 > 3 x 64) --, quads on virtual lanes at one wave for every KQ up to 21, up to 7 rows of several quads among them; the rows of the
    generic loop and the rows on virtual lanes carry mass in both directions."""
    g, V, lens = qc.mixed300_case(wl)
    assert 3 * 64 < g.S + 1 <= 384
    deg = qc.row_lengths(g)
    assert all(len(set(np.unique(d).tolist())) >= 10 and d.max() >= 40 for d in deg)
    _packer_agrees(mm, wl, g, qc.KQ_ALL)
    _finite_ttl(oracle, g, V, lens, "Q1")
    mass = _row_mass(oracle, g, V, lens, "Q1")
    seen = set()
    for kq in qc.KQ_ALL:
        for nwaves in (None, 1):
            for d in (0, 1):
                KQ, NW, RPT = qc.geometry(g, d, kq, nwaves)
                assert KQ == kq and RPT == (2 if nwaves is None else 3) and (nwaves is None or NW == 1)
                seen.add((KQ, RPT, d))
                if nwaves == 1:
                    lay = qc.layout(g, d, KQ)
                    gen = lay.order[qc.generic_positions(lay, RPT, 64)]
                    gen = gen[gen < g.S]
                    assert gen.size >= 64 and (mass[gen] > GAMMA_FLOOR).all(), (kq, d)
                    virt = qc.virtual_positions(lay, KQ, 64)
                    assert (virt.size > 0) == (lay.total > 64 * KQ)
                    vs = lay.order[virt]
                    assert (mass[vs[vs < g.S]] > GAMMA_FLOOR).all(), (kq, d)
                    if kq <= 21:
                        assert virt.size > 0
                    if kq <= 7:  # (rows of several quads among them: a virtual lane's running sum continues)
                        assert (lay.nq[virt] > 1).any(), (kq, d)
    assert len(seen) == 72
    print(f"mixed300: {g.S} states, quads {qc.quads(g)}, the smallest row mass {mass[:-1].min():.3g}")


# ---- 2: virtual lanes
@pytest.mark.parametrize("kq,nq", qc.VIRTUAL_CASES)
def test_chains_at_the_register_window(mm, wl, oracle, kq, nq):
    """A chain of nq states has nq quads in each direction; at one wave of KQ quads per lane the rows beyond quad 64 KQ lie on virtual
    lanes -- none at 64 KQ - 1 and at 64 KQ, one at 64 KQ + 1 -- and each of them carries mass."""
    g, V, lens = qc.virtual_case(wl, nq)
    _packer_agrees(mm, wl, g, (kq,))
    assert qc.quads(g) == (nq, nq)
    _finite_ttl(oracle, g, V, lens, ("Q2", nq))
    mass = _row_mass(oracle, g, V, lens, ("Q2", nq))
    for d in (0, 1):
        assert qc.geometry(g, d, kq, 1)[:2] == (kq, 1)
        lay = qc.layout(g, d, kq)
        virt = qc.virtual_positions(lay, kq, 64)
        assert virt.size == max(0, nq - 64 * kq)
        vs = lay.order[virt]
        assert (mass[vs[vs < g.S]] > GAMMA_FLOOR).all()
    partly = nq > 64 * kq and nq % kq != 0
    print(f"KQ {kq}, {nq} quads: {max(0, nq - 64 * kq)} on virtual lanes, the last virtual lane {'partly filled' if partly else 'full or absent'}")


def test_partly_filled_virtual_lanes_are_among_the_cases():
    assert {(kq, nq > 64 * kq and nq % kq) for kq, nq in qc.VIRTUAL_CASES} >= {(2, 1), (3, 1), (3, 2)}
    for kq in (1, 2, 3):
        assert {nq - 64 * kq for k, nq in qc.VIRTUAL_CASES if k == kq} >= {-1, 0, 1}


def test_dense_graph_overflows_eight_waves(mm, wl, oracle):
    g, V, lens = qc.dense400_case(wl)
    _packer_agrees(mm, wl, g, (15,))
    _finite_ttl(oracle, g, V, lens, "Q2_dense")
    mass = _row_mass(oracle, g, V, lens, "Q2_dense")
    for d in (0, 1):
        assert qc.geometry(g, d, 15)[:2] == (15, 8)
        lay = qc.layout(g, d, 15)
        virt = qc.virtual_positions(lay, 15, 512)
        vs = lay.order[virt]
        assert lay.total > 512 * 15 and (lay.nq[virt] > 1).sum() >= 20 and (mass[vs[vs < g.S]] > GAMMA_FLOOR).all()
        print(f"dense400 direction {d}: {lay.total} quads, {virt.size} rows on virtual lanes")


@pytest.mark.parametrize("S1", qc.MULT32_S1)
def test_quad_form_of_a_multiple_of_32_states(mm, wl, S1):
    """The packer lays the second copy of the linear vector out by the padded state count, and the kernels (and the host evaluation,
    which addresses as they do) by theirs: make_quads took ceil4(S1), the engine ceil4(S1 + 1), and quad_pstride() of the two differs
    exactly where S1 is a multiple of 32 -- every arc placed on the second copy then read another state's value or a zero.  One
    definition now (mm_pack.h padded_states); the products through the form agree at every KQ."""
    g = qc.chain_graph(wl, S1)
    assert _packer_agrees(mm, wl, g, (1, 2, 3, 5, 7, 15)).S1 == S1


# ---- 3: row kinds
@pytest.mark.parametrize("kq", [1, 5])
@pytest.mark.parametrize("extra", qc.HUB_EXTRAS)
def test_hub_rows_have_the_lane_ends_they_are_named_for(mm, wl, oracle, extra, kq):
    """The in-hub's row in the forward layout and the out-hub's row in the backward layout have exactly `extra` lane ends before their
    last quad: row_short with 0, 1 and 2 terms, row_long from 3 on (its four-at-a-time walk: 3, 4 -- one pass --, 5, 8 -- two --,
    9 -- three).  Both hubs carry mass, under a pdf that is theirs alone."""
    g, V, lens = qc.hub_case(wl, extra, kq)
    _packer_agrees(mm, wl, g, (kq,))
    _finite_ttl(oracle, g, V, lens, ("Q3", extra, kq))
    gam, _ = qc.reference(oracle, graphs, [g] * 3, V, lens, ("Q3", extra, kq))
    s2p = np.asarray(g.state2pdf)
    for d, hub in ((0, qc.HUB_IN), (1, qc.HUB_OUT)):
        lay = qc.layout(g, d, kq)
        i = lay.position_of(hub)
        assert lay.extra[i] == extra and lay.kind(i) == ("long" if extra >= 3 else "short"), (d, lay.extra[i], lay.nq[i], lay.q0[i])
        assert (s2p == s2p[hub]).sum() == 1 and hub in g.init_idx
        top = gam[:, :, s2p[hub]].max()
        print(f"{extra} lane ends at KQ {kq}, direction {d}: a row of {lay.nq[i]} quads from quad {lay.q0[i]}; the hub's largest gamma {top:.3g}")
        assert top > 1e-3


@pytest.mark.parametrize("kq", [1, 5])
def test_the_phony_final_row_is_long(mm, wl, oracle, kq):
    g, V, lens = qc.many_finals_case(wl)
    _packer_agrees(mm, wl, g, (kq,))
    _finite_ttl(oracle, g, V, lens, "Q3_finals")
    lay = qc.layout(g, 0, kq)
    i = lay.position_of(g.S)
    assert i == 0 and lay.kind(i) == "long" and lay.nq[i] == 18
    assert qc.layout(g, 1, kq).nq[qc.layout(g, 1, kq).position_of(g.S)] == 1  # (backward: its self loop alone)


@pytest.mark.parametrize("kq", qc.LATE_HUB_KQ)
def test_a_long_row_in_the_backward_generic_loop(mm, wl, oracle, kq):
    """late_hub_graph at one wave: the hub's row is long and lies beyond the RPT x 64 register-carried rows of the backward pass; the
    hub carries mass."""
    g, V, lens = qc.late_hub_case(wl)
    _packer_agrees(mm, wl, g, (kq,))
    _finite_ttl(oracle, g, V, lens, "Q3_late")
    KQ, NW, RPT = qc.geometry(g, 1, kq, 1)
    lay = qc.layout(g, 1, kq)
    i = lay.position_of(qc.LATE_HUB)
    mass = _row_mass(oracle, g, V, lens, "Q3_late")[qc.LATE_HUB]
    print(f"late hub at KQ {kq}: position {i} of {g.S + 1} (generic loop from {RPT * 64 * NW}), {lay.nq[i]} quads, {lay.extra[i]} lane ends, largest posterior {mass:.3g}")
    assert (KQ, NW, RPT) == (kq, 1, 3) and i in qc.generic_positions(lay, RPT, 64) and lay.kind(i) == "long" and mass > 1e-3


# ---- 4: the exact fallback
def _spread(oracle, g, V, lens, key):
    """Per direction: the number of (state, frame) whose value is finite and lies more than 70 nats (the 62.4 of the linear sums and a
    margin for the normaliser's lag of one frame) below its frame's largest; the largest such distance; and per row length of the
    direction {arcs: (such values, those of them whose state posterior in that frame exceeds check_gamma's floor)}."""
    out = []
    post = qc.state_posteriors(oracle, graphs, g, V, lens, key)
    for dname, pick in (("forward", 0), ("backward", 1)):
        count, worst, per = 0, 0.0, {}
        deg = qc.row_lengths(g)[pick][: g.S]
        for b, n in enumerate(lens):
            X = qc.alpha_beta(oracle, graphs, g, V[b], int(n))[pick][: g.S, 1 : n + 1]
            if pick == 1:  # (the backward vector the kernel keeps: beta times the frame's emission)
                X = X + V[b, :n, np.asarray(g.state2pdf)].astype(np.float64)
            live = np.isfinite(X)
            below = np.where(live, X.max(axis=0, keepdims=True) - np.where(live, X, 0.0), 0.0)
            low = below > 70.0
            count += int(low.sum())
            worst = max(worst, float(below.max()))
            seen = low & (post[b, :n].T > GAMMA_FLOOR)
            for k in np.unique(deg):
                a, c = per.get(int(k), (0, 0))
                per[int(k)] = (a + int(low[deg == k].sum()), c + int(seen[deg == k].sum()))
        out.append((dname, count, worst, per))
    return out


def test_deep_graph_spreads_beyond_the_linear_range(mm, wl, oracle):
    g, V, lens = qc.deep_case(wl)
    for kq in {e["kq"] for e in qc.FALLBACK_ENVS.values()}:
        _packer_agrees(mm, wl, g, (kq,))
    assert qc.UNDERFLOW_NATS < 62.5
    for d, deg in enumerate(qc.row_lengths(g)):
        assert set(qc.FALLBACK_ROWS) <= set(deg[: g.S].tolist()), (d, np.unique(deg))
    cf = _compile(mm, wl, g)
    for d in (0, 1):  # rows that are dead in some frame of the longest utterance
        dist = cf.reach_distance(d)[: g.S]
        assert (dist >= 2).sum() >= 50, (d, np.bincount(dist[dist >= 0]))
    _finite_ttl(oracle, g, V, lens, "Q4_deep")
    for dname, count, worst, per in _spread(oracle, g, V, lens, "Q4_deep"):
        print(f"deep graph, {dname}: {count} live values more than 70 nats below their frame's largest (the furthest: {worst:.0f} nats); "
              f"by row length (such values, with posterior mass): { {k: per[k] for k in qc.FALLBACK_ROWS} }")
        assert count >= 100
        # rows of each of the five lengths are among them: every chunking of a fallback body computes values that are alive.  (Few of
        # them carry posterior mass in their own frame -- 70 nats below the frame's largest --; they feed the rows of later frames.)
        assert all(per[k][0] >= 1 for k in qc.FALLBACK_ROWS), per


def test_sharp_emissions_spread_beyond_the_linear_range(mm, wl, oracle):
    g, V, lens = qc.sharp_case(wl)
    _finite_ttl(oracle, g, V, lens, "Q4_sharp")
    for dname, count, worst, _ in _spread(oracle, g, V, lens, "Q4_sharp"):
        print(f"sharp emissions, {dname}: {count} live values more than 70 nats below their frame's largest (the furthest: {worst:.0f} nats)")
        assert count >= 100


# ---- 5: the pdf count
@pytest.mark.parametrize("P", qc.P_EDGES_ONE_WAVE)
def test_pdf_edges_carry_mass(mm, wl, oracle, P):
    """pdf P - 1 (the last lane of the staging's and finish_frame's last pass), the first pdf of that pass, and the pdfs of 1, 8, 9 and 17
    states carry posterior mass above check_gamma's floor; the pdf without a state is exactly 0."""
    g, V, lens = qc.pdf_edge_case(wl, P)
    _packer_agrees(mm, wl, g, (qc.geometry(g, 0)[0],))
    n = np.bincount(np.asarray(g.state2pdf), minlength=P)
    assert n[:5].tolist() == list(qc.PDF_SIZES) + [0] and (n[5:] > 0).all() and g.P == P
    gam, _ = _finite_ttl(oracle, g, V, lens, ("Q5", P))
    top = gam.max(axis=(0, 1))
    q = qc.last_pass_pdf(P)
    print(f"P = {P}: largest gamma of pdf {P - 1}: {top[P - 1]:.3g}, of pdf {q}: {top[q]:.3g}, of the pdfs of 1, 8, 9, 17 states: {top[:4]}")
    assert top[qc.EMPTY_PDF] == 0 and (top[[P - 1, q, 0, 1, 2, 3]] > GAMMA_FLOOR).all()
    for nwaves in (1, 2) if P in qc.P_EDGES_TWO_WAVES else (1,):
        assert all(qc.geometry(g, d, None, nwaves)[1] == nwaves for d in (0, 1))


# ---- 6: the wave count
def test_big_graph_takes_every_wave_count(mm, wl, oracle):
    g, V, lens = qc.big_case(wl)
    _packer_agrees(mm, wl, g, (9, 15))
    _finite_ttl(oracle, g, V, lens, "Q6")
    assert 1900 <= g.S + 1 <= 2048
    want = {(9, 1): 3, (9, 2): 3, (9, 3): 3, (9, 12): 3, (9, 16): 2, (15, 8): 3}
    for kq, nw in qc.WAVE_CASES:
        for d in (0, 1):
            assert qc.geometry(g, d, kq, nw) == (kq, nw, want[(kq, nw)])
    assert qc.geometry(g, 0)[1] == 16  # (without a switch: 16 waves)


# ---- 7: the lengths
def test_lengths_with_and_without_a_path(mm, wl, oracle):
    """Every length from 1 on has a path -- length 1 through the state that is initial and final, which holds all of frame 1's mass --;
    length 0 and the utterance with a frame at -inf are the two deliberately dead ones."""
    g, V, lens = qc.lengths_case(wl)
    assert lens.tolist() == [0, 1, 2, 3, 4, 5, qc.LENGTHS_N, qc.LENGTHS_N]
    _packer_agrees(mm, wl, g, (qc.geometry(g, 0)[0], qc.geometry(g, 1)[0]))
    both = np.intersect1d(g.init_idx, g.final_idx)
    assert both.size == 1
    gam, ttl = _finite_ttl(oracle, g, V, lens, "Q7", dead=qc.LENGTHS_DEAD)
    print(f"lengths {lens.tolist()}: ttl {ttl}")
    pdf = int(np.asarray(g.state2pdf)[both[0]])
    assert np.isfinite(ttl[1]) and abs(gam[1, 0, pdf] - 1.0) < 1e-12 and gam[1, 0].sum() > 1 - 1e-12 and (gam[1, 1:] == 0).all()
    for b in range(2, 7):  # (the frames of the short lengths carry mass on several pdfs)
        assert (gam[b, : lens[b]] > GAMMA_FLOOR).sum(axis=1).min() >= 2
    _finite_ttl(oracle, g, V[:7], None, "Q7_none")
