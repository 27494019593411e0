"""The inputs of tests/test_gpu_itemform.py, checked without a GPU: the float64 references alone on the cases of its groups B
(a graph beyond 16-bit state indices) and D (wide rows), and the conditions those tests rest on -- a truncated state index or a
row cut short is only visible where the reference itself puts mass there."""
import json
import os

import numpy as np
import pytest

import arc_reference as ar
import cost_reference as cr
import test_gpu_itemform as ti

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
    import graphs

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
