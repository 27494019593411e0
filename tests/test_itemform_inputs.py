"""The inputs of tests/test_gpu_itemform.py, checked without a GPU: the float64 references alone on the cases of its groups B
(a graph beyond 16-bit state indices) and D (wide rows), and the conditions those tests rest on -- a truncated state index or a
row cut short is only visible where the reference itself puts mass there.  Below, the same for tests/test_gpu_itemform_entries.py:
by each entry's own float64 reference, called as that file calls the entry, a lost arc of a wide row, a state index cut to 16 bits
and the emissions of the last pdfs are visible to the comparisons it uses."""
import dataclasses
import json
import os

import numpy as np
import pytest

import arc_reference as ar
import cost_reference as cr
import entropy_reference as er
import filter_reference as fr
import graphs
import leaky_reference as lr
import segment_reference as sr
import test_gpu_itemform as ti
import test_gpu_itemform_entries as tn
import test_gpu_weightedposteriors as tw
import vitwindow_reference as vr
import window_reference as wr
from test_gpu_parity import GAMMA_FLOOR, RTOL_LOGPOST, check_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arc_identities(rc, L, N):
    # N transitions per utterance (the phony final state's self-loop takes the frames beyond the length), one initial state.
    # (The reference combines the oracle's float64 alpha / beta with the float32 weight of the product's FSM: every term of the
    # sum is off by at most one float32 rounding of its arc's weight, 2^-24 relative.)
    assert abs(rc["counts"].sum() - N) <= 2.0 ** -24 * N, (rc["counts"].sum(), N)
    assert abs(rc["init"].sum() - 1.0) <= 1e-9, rc["init"].sum()
    assert np.isfinite(rc["logz"]) and (rc["counts"] >= 0).all()


def test_graph_beyond_16_bit_indices(mm, wl, oracle):
    case = ti.case_random_big(wl)
    gs, V, cost, lens, _ = case
    g, N = gs[0], V.shape[1]
    assert g.S == 70000 and g.S + 2 > 65534 and g.n_arcs == 301333
    ti.assert_high_states_carry_mass(oracle, case)
    f = wl.to_fsm(mm, g)
    i, j, _ = ar.fsm_entries(f)
    o, oc = oracle
    for b, L in enumerate(lens):
        c, init, z = ar.reference(o, oc, g, f, V[b].astype(np.float64), int(L), N)
        _arc_identities({"counts": c, "init": init, "logz": z}, int(L), N)
        # arcs with a state beyond 16 bits at either end carry counts well above arc_reference.check's absolute bar
        high = ((i >= ti.HIGH) & (i < g.S)) | ((j >= ti.HIGH) & (j < g.S))
        assert c[high].sum() >= 1e-2 * L and (c[high] > 1e-4).any()
        # the cost reference on the same input: finite, the same log Z, posteriors that sum to one
        risk, grad, gamma, z2 = cr.reference(o, oc, g, f, V[b].astype(np.float64), cost[b].astype(np.float64), int(L), N)
        assert np.isfinite(risk) and np.isfinite(grad).all() and abs(z2 - z) <= 1e-9 * abs(z)
        assert np.allclose(gamma[:L].sum(axis=1), 1.0, atol=1e-9)


def test_best_paths_of_the_big_graph_pass_high_states(wl, oracle):
    """test_beyond_16_bit_indices_tropical asserts that a Viterbi path passes a state >= 65 536: it does, by the oracle."""
    o, oc = oracle
    gs, V, _, lens, _ = ti.case_random_big(wl)
    of = graphs.to_oracle(o, gs[0], "tropical", np.float32)
    paths = [oc.viterbi(of, gs[0].state2pdf, gs[0].P, V[b], int(L), dtype=np.float32)[0] for b, L in enumerate(lens)]
    assert any((np.asarray(p) >= ti.HIGH).any() for p in paths), paths


@pytest.mark.parametrize("big_first", [True, False])
def test_mixed_batch_inputs(wl, oracle, big_first):
    case = ti.case_mixed(wl, big_first)
    assert [g.S for g in case[0]] == ([70000, 40] if big_first else [40, 70000]) and all(g.P == 40 for g in case[0])
    ti.assert_high_states_carry_mass(oracle, case)


@pytest.mark.parametrize("name", ["wide", "ergodic300", "lexicon"])
def test_wide_row_inputs(mm, wl, oracle, name):
    gs, V, cost, lens, _ = ti.case_wide(wl, name)
    N = V.shape[1]
    for b, L in enumerate(lens):
        rc = ti.row_counts(mm, wl, oracle, gs[b], V[b].astype(np.float64), int(L), N)
        _arc_identities(rc, int(L), N)
        if name == "wide":
            assert rc["in"][:2] == (5, 650) and rc["out"][:2] == (7, 642)
            # every arc of the two wide rows above 1e-6: the relative part of arc_reference.check's bar binds on all of them
            f = wl.to_fsm(mm, gs[b])
            i, j, _ = ar.fsm_entries(f)
            assert (rc["counts"][(j == 5) & (i < gs[b].S)] > 1e-6).all() and (rc["counts"][(i == 7) & (j < gs[b].S)] > 1e-6).all()
        elif name == "ergodic300":
            assert rc["in"][1] == 300 and rc["out"][1] == 300
        ti.assert_wide_rows_carry_counts(name, rc, b)


def test_cost_floor_table_covers_the_new_cases():
    """profiles/expectedcost_floor.json (tools/measure_cost_floor.py) has the item-form cost cases, none above the floor the
    gradient's bar was derived from."""
    with open(os.path.join(ROOT, "profiles", "expectedcost_floor.json")) as fh:
        table = json.load(fh)
    names = {r["case"] for r in table["rows"]}
    for want in ("lfmmi600", "70000 states", "70000 + 40 states", "40 + 70000 states", "65530 states", "65531 states",
                 "wide rows", "ergodic300", "lexicon3000"):
        assert want in names, (want, sorted(names))
    assert max(r["grad_err_over_G"] for r in table["rows"]) <= cr.GRAD_F32_FLOOR
    assert table["worst_grad_err_over_G"] <= cr.GRAD_F32_FLOOR


# ---- the inputs of tests/test_gpu_itemform_entries.py: what its comparisons can see, from the references alone
LOG_ENTRIES = ["leaky", "entropy", "filter", "window", "segment"]


def entry_gamma(entry, mm, wl, oracle, g, V, b, lens, modes):
    """gamma [N, P] of utterance b of a batch as tests/test_gpu_itemform_entries.run_entry gives it to `entry`: the float64
    reference of that entry with that test's arguments (window: closed / open alternating, commit at half the length; segment: the
    end modes, state and end vectors of segment_args)."""
    N, L, Vb = V.shape[1], int(lens[b]), V[b].astype(np.float64)
    if entry == "leaky":
        return lr.reference(g, Vb, L, N, tn.LEAK)[0]
    if entry == "entropy":
        o, oc = oracle
        return er.reference(o, oc, g, wl.to_fsm(mm, g), Vb, L, N)[2]
    if entry == "filter":
        return fr.reference(g, Vb, L, N)[0]
    if entry == "window":
        closed, commit = tn.window_args(lens)
        return wr.reference(g, Vb, L, N, None, bool(closed[b]), int(commit[b]))[0]
    assert entry == "segment"
    m, states, end = tn.segment_args([g] * len(lens), lens, modes)
    return sr.reference(g, Vb, L, N, states[b], int(m[b]), end[b])[0]


def gamma_error_over_bars(g, g_ref):
    """check_gamma's two criteria as ratios: max |g - g_ref| over 2e-5, and the worst log-posterior error over its bar (inf where
    the reference has mass and g has none)."""
    a = float(np.abs(g - g_ref).max() / 2e-5)
    m = g_ref > GAMMA_FLOOR
    with np.errstate(divide="ignore"):
        lg, lr_ = np.log(g[m]), np.log(g_ref[m])
    return a, float(np.max(np.abs(lg - lr_) / (RTOL_LOGPOST * np.maximum(np.abs(lr_), 1.0))))


def assert_visible(entry, what, mutated, base, L):
    a, l = gamma_error_over_bars(mutated, base)
    print(f"{entry}, {what}: abs criterion at {a:.3g} of its bar, log-posterior criterion at {l:.3g} of its bar")
    with pytest.raises(AssertionError):
        check_gamma(mutated[None], base[None], [L])
    return a, l


def widest_rows(g):
    """The widest-in and the widest-out real state of a GraphSpec (its arcs are the real ones: ti.row_counts finds the same two)."""
    return int(np.argmax(np.bincount(g.dst, minlength=g.S))), int(np.argmax(np.bincount(g.src, minlength=g.S)))


def without_last_arcs(g, s, direction, k):
    """g without the last k stored arcs into (`in`) or out of (`out`) state s; nothing is renormalised."""
    keep = np.ones(g.src.size, dtype=bool)
    keep[np.flatnonzero((g.dst if direction == "in" else g.src) == s)[-k:]] = False
    return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], w=g.w[keep])


@pytest.mark.parametrize("name", tn.WIDE_NAMES)
@pytest.mark.parametrize("entry", LOG_ENTRIES)
def test_a_lost_arc_of_a_wide_row_is_visible(mm, wl, oracle, entry, name):
    """A long-row branch that drops the last arc, or the last 64, of the widest row of either direction: each utterance's gamma
    then fails check_gamma against the unmutated reference, for each entry as the GPU test calls it."""
    gs, V, lens = tn.drop_cost(ti.case_wide(wl, name))
    g = gs[0]
    s_in, s_out = widest_rows(g)
    if name == "wide":
        assert (s_in, s_out) == (5, 7)
    worst = [np.inf, np.inf]
    for b in range(len(gs)):
        base = entry_gamma(entry, mm, wl, oracle, g, V, b, lens, tn.WIDE_MODES[name])
        for direction, s in (("in", s_in), ("out", s_out)):
            for k in (1, 64):
                mut = entry_gamma(entry, mm, wl, oracle, without_last_arcs(g, s, direction, k), V, b, lens, tn.WIDE_MODES[name])
                a, l = assert_visible(entry, f"{name}, utterance {b}, {k} arc(s) lost {direction} state {s}", mut, base, int(lens[b]))
                if k == 1:
                    worst = [min(worst[0], a), min(worst[1], l)]
    print(f"{entry}, {name}: one arc lost, the least visible case: abs criterion {worst[0]:.3g}, log-posterior criterion {worst[1]:.3g} of the bar")


@pytest.mark.parametrize("entry", LOG_ENTRIES)
def test_a_state_index_cut_to_16_bits_is_visible(mm, wl, oracle, entry):
    """The 70 000-state graph with every dst >= 65 536 reduced by 65 536."""
    gs, V, lens = tn.drop_cost(ti.case_random_big(wl))
    g = gs[0]
    cut = dataclasses.replace(g, dst=np.where(g.dst >= ti.HIGH, g.dst - ti.HIGH, g.dst))
    for b in range(len(gs)):
        base = entry_gamma(entry, mm, wl, oracle, g, V, b, lens, (2, 1))
        assert_visible(entry, f"70000 states, utterance {b}, indices cut to 16 bits", entry_gamma(entry, mm, wl, oracle, cut, V, b, lens, (2, 1)), base, int(lens[b]))


def _commit_frame(g, V, L, c, closed):
    """(D_c, the restatement of the whole window): D_c [S + 1] the float32 scores of frame c, by the restatement's own steps."""
    sys = vr.system(g)
    with np.errstate(invalid="ignore"):
        d = (vr.start_vector(g, None, sys) + vr._lhs(g, V, L, 1, np.float32)).astype(np.float32)
        for n in range(2, c + 1):
            d = (vr._step(sys, d, g.S + 1)[0] + vr._lhs(g, V, L, n, np.float32)).astype(np.float32)
    return d, vr.reference(g, V, L, V.shape[0], None, closed, c, False, np.float32, sys)


@pytest.mark.parametrize("name", tn.WIDE_NAMES)
def test_vitwindow_sees_the_arc_its_back_pointer_picks(wl, name):
    """viterbiwindow on the wide graphs: the widest-in state's state_out at the commit frame is finite, and without the arc the
    back-pointer picks for it the value changes -- state_out is compared bit for bit."""
    gs, V, lens = tn.drop_cost(ti.case_wide(wl, name))
    gs, V = tn.tropical_inputs(gs, V)
    g = gs[0]
    s_in, _ = widest_rows(g)
    closed, commit = tn.window_args(lens)
    for b in range(len(gs)):
        L, c = int(lens[b]), int(commit[b])
        d, ref = _commit_frame(g, V[b], L, c, bool(closed[b]))
        into = np.flatnonzero(g.dst == s_in)
        val = d[g.src[into]] + g.w[into].astype(np.float32)
        pick = into[val == val.max()]
        pick = pick[np.argmin(g.src[pick])]  # (the lowest source among the maximisers)
        assert np.isfinite(ref.score) and np.isfinite(ref.state_out[s_in]) and ref.ncommit == c
        assert ref.state_out[s_in] == np.float32(val.max() - ref.mcommit)
        keep = np.ones(g.src.size, dtype=bool)
        keep[pick] = False
        mut = dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], w=g.w[keep])
        out = vr.reference(mut, V[b], L, V.shape[1], None, bool(closed[b]), c, False, np.float32)
        print(f"{name}, utterance {b}: state_out[{s_in}] at frame {c}: {ref.state_out[s_in]} through the arc from {g.src[pick]}, {out.state_out[s_in]} without it")
        assert out.state_out[s_in] != ref.state_out[s_in]


def test_vitwindow_best_paths_of_the_big_graph_pass_high_states(wl):
    """As test_best_paths_of_the_big_graph_pass_high_states for viterbi, on the entries test's rounded inputs: a best path passes a
    state >= 65 536, and every utterance's state_out (compared bit for bit over all 70 001 entries) is finite on such states."""
    gs, V, lens = tn.drop_cost(ti.case_random_big(wl))
    gs, V = tn.tropical_inputs(gs, V)
    closed, commit = tn.window_args(lens)
    refs = tn.vitwindow_references(gs, V, lens, closed, commit)
    assert all(np.isfinite(r.score) for r in refs)
    assert any((r.path[: int(L)] >= ti.HIGH).any() for r, L in zip(refs, lens)), [r.path for r in refs]
    assert all((np.isfinite(r.state_out[ti.HIGH : gs[0].S])).any() for r in refs)


# ---- group P: the last pdfs carry mass
def _boundary_gammas(entry, mm, wl, oracle, case):
    """Per utterance gamma [N, P] of the reference `entry` is compared against in test_pdf_count_at_the_block_size."""
    gs, V, cost, lens, _ = case
    g, N = gs[0], V.shape[1]
    o, oc = oracle
    if entry in ("pdfposteriors", "arcs", "sample", "arcclass", "scored", "classcost"):  # (the oracle's posteriors: what _pdf_check and
        # _size_check compare against; the arc-class entry's xi by destination pdf is gamma one frame on, the scored entry is run with
        # U NULL as well as with scores, and the class costs do not touch gamma)
        return list(oc.batch_shared(graphs.to_oracle(o, g), g.state2pdf, g.P, V, lens, dtype=np.float64)[0])
    if entry == "cost":
        f = wl.to_fsm(mm, g)
        return [cr.reference(o, oc, g, f, V[b].astype(np.float64), cost[b].astype(np.float64), int(lens[b]), N)[2] for b in range(2)]
    if entry == "weighted":
        fs = [wl.to_fsm(mm, g)] * 2
        W, Wi = tw._noisy(np.random.default_rng(89), fs)
        return [r[0] for r in tw._refs(gs, fs, V, lens, W, Wi)]
    return [entry_gamma(entry, mm, wl, oracle, g, V, b, lens, (2, 1)) for b in range(2)]


@pytest.mark.parametrize("P", [511, 512, 513, 1023, 1024, 1025, 127, 128, 129])
def test_the_last_pdfs_carry_mass(mm, wl, oracle, P):
    """Each of the pdfs P-4 .. P-1 reaches gamma >= 5e-3 in some frame of some utterance, by every entry's own reference: an
    emission staged wrongly at the end of the block is then visible to check_gamma (2e-5 absolute).  viterbiwindow has no
    posterior: for it, an emission of -inf on any one of those pdfs changes an output of some utterance."""
    S = 200 if P < 200 else 700
    case = tn.case_pdf_boundary(wl, S, P)
    gs, V, _, lens, _ = case
    assert (np.asarray(gs[0].state2pdf[:8]) == P - 1 - np.arange(8)).all()
    entries = [e for e in tn.ALL_ENTRIES if e != "vitwindow" and ((e in tn.UNCAPPED) == (P > 1000) or P < 200)]
    for entry in entries:
        gam = _boundary_gammas(entry, mm, wl, oracle, case)
        top = np.max([x[:, P - 4 :].max(axis=0) for x in gam], axis=0)
        print(f"{entry}, P = {P}: the largest gamma of the pdfs P-4 .. P-1: {np.array2string(top, precision=3)}")
        assert (top >= 5e-3).all(), (entry, top)
    if P > 1000 or P < 200:
        tg, tV = tn.tropical_inputs(gs, V)
        closed, commit = tn.window_args(lens)
        refs = tn.vitwindow_references(tg, tV, lens, closed, commit)
        for q in range(P - 4, P):
            Vq = tV.copy()
            Vq[:, :, q] = -np.inf
            out = [vr.reference(tg[b], Vq[b], int(lens[b]), tV.shape[1], None, bool(closed[b]), int(commit[b]), False, np.float32) for b in range(2)]
            assert any(not (np.array_equal(o_.path, r.path) and o_.score == r.score and np.array_equal(o_.state_out, r.state_out)) for o_, r in zip(out, refs)), q
