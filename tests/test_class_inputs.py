"""The inputs of tests/test_gpu_class_entries.py (tests/class_cases.py), checked without a GPU: from the float64 references alone,
each comparison the GPU tests use would see the fault its fixture is there for.  "Visible" means that arcclass_reference.check (for
classcost: classcost_reference.check; for gamma: check_gamma) raises when it is given the mutated float64 result, cast to float32,
against the true reference:

  shape layouts   a class's first or last rank dropped, one lane's share of it dropped, its last member summed into the next class
                  (a class pointer off by one);
  count layouts   the score / cost of the last class read as 0, or as the value of class NT - 1 (the clamp of score_load_raw);
  high states     a row or a column index of a term record reduced mod 65 536.

And the structure the fixtures promise: sizes, bands of the lanes rule, class counts, where the phony self-loop stands."""
import json
import os

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr
import class_cases as cc
import classcost_reference as ccr
import scored_reference as sr
import test_gpu_classcost as tgc
import test_gpu_itemform as ti
import test_gpu_scoredposteriors as tgs
from test_gpu_parity import check_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def base(mm, wl, oracle):
    """The base graph, its FSM, V, lens and per utterance (x [nnz, N], log Z): every entry's posterior at every transition."""
    g = cc.base_graph(wl)
    f = wl.to_fsm(mm, g)
    V, lens = cc.base_inputs(g)
    return g, f, V, lens, [cc.entry_posteriors(oracle, g, f, V[b].astype(np.float64), int(lens[b]), cc.N) for b in range(2)]


def visible(xi_mut, xi_ref, z, exact):
    """Does arcclass_reference.check refuse the mutated result?  Returns its worst |error| / (1e-4 xi_ref + 1e-6) as well."""
    over = float((np.abs(xi_mut.astype(np.float32).astype(np.float64) - xi_ref) / (1e-4 * xi_ref + 1e-6)).max())
    try:
        acr.check(xi_mut.astype(np.float32), z, xi_ref, z, exact)
    except AssertionError:
        return True, over
    return False, over


# ---- structure
def test_base_graph_and_block_size(mm, wl, base):
    g, f, V, lens, _ = base
    info = mm.compile(f, mm.statemap(g.state2pdf, g.P)).info()
    assert f.nnz == 9704 and info["packed_items"] == [60, 63]
    assert 64 * min(8, min(16, max(info["packed_items"]) + 1)) == cc.NT  # (item_plan: 8 waves for the three entries)
    assert cc.ranked_entries(f).size == f.nnz - 1  # every entry but the phony self-loop


@pytest.mark.parametrize("phony", cc.PHONY_VARIANTS)
@pytest.mark.parametrize("lanes", cc.LANES)
def test_shape_layout_structure(base, lanes, phony):
    g, f, _, _, _ = base
    cls, C, facts = cc.shape_layout(f, lanes, cc.SHAPE_SEED, phony)
    st, per = lanes, 64 // lanes
    size = np.bincount(cls[cls >= 0], minlength=C)
    M = int(size.sum())
    assert M == facts["M"] and cc.lanes_for(M, C) == lanes, (M, C)
    if lanes == 1:
        assert M < 2 * C
    elif lanes == 8:
        assert 2 * C <= M < 32 * C
    else:
        assert M >= 32 * C
    # more than one trip of the c0 loop of an 8-wave block, the last trip partial; within its last wave a partial group of classes
    assert C > 8 * per and C % (8 * per) != 0 and (per == 1 or C % per != 0)
    assert size[0] == 0 and size[C - 1] == 0
    want = [n for n in cc.edge_sizes(lanes) if n]
    assert [facts["edge"][c] for c in sorted(facts["edge"])] == want and [int(size[c]) for c in sorted(facts["edge"])] == want
    assert {st - 1, st, st + 1, 4 * st - 1, 4 * st, 4 * st + 1, 5 * st, 8 * st + 3} - {0} <= set(want)
    kp = cc.phony_entry(f)
    big = cc.SHAPE_BIG[lanes]
    if phony == "own":
        assert cls[kp] == facts["phony_class"] and size[facts["phony_class"]] == 1 and size[facts["large"]] == big
    elif phony == "large":
        assert cls[kp] == facts["large"] and size[facts["phony_class"]] == 0 and size[facts["large"]] == big + 1
    else:
        assert cls[kp] == -1 and size[facts["phony_class"]] == 0 and size[facts["large"]] == big
    assert size[facts["large"]] > 4 * max(want)
    others = np.delete(size, list(facts["edge"]) + [facts["large"], facts["phony_class"]])
    assert others.max() <= (1 if lanes == 1 else 0)
    # a class's ranks (its members in entry order) are scattered over the rows of the graph: neighbouring ranks read different rows
    rows = np.asarray(ar.fsm_entries(f)[0])
    for c, n in facts["edge"].items():
        if n >= 8:
            assert (np.diff(rows[cls == c]) != 0).mean() >= 0.9 and np.unique(rows[cls == c]).size >= min(n, 100) // 2


def test_threshold_and_rank_layout_structure(base):
    g, f, _, _, _ = base
    C = cc.THRESHOLD_C
    got = []
    for M in cc.threshold_values(C):
        cls = cc.threshold_layout(f, C, M)
        assert (cls >= 0).sum() == M and cls.max() < C and cls[cc.phony_entry(f)] == -1
        got.append(cc.lanes_for(M, C))
    assert got == [1, 8, 8, 64]
    for nt in (cc.NT, cc.NT_TWO_WAVES):
        assert cc.rank_values(nt) == (nt - 1, nt, nt + 1, 8 * nt - 1, 8 * nt, 8 * nt + 1)
        for M in cc.rank_values(nt):
            cls = cc.rank_layout(f, M)
            size = np.bincount(cls[cls >= 0], minlength=5)
            assert size.sum() == M and size.size == 5 and (size > 0).all()


@pytest.mark.parametrize("nt", [cc.NT, cc.NT_TWO_WAVES])
def test_count_layout_structure(base, nt):
    g, f, _, _, _ = base
    assert {(C + 1) % 4 for C in cc.count_values(nt)} == {0, 1, 2, 3}
    assert min(cc.count_values(nt)) < nt < max(cc.count_values(nt))
    for C in cc.count_values(nt):
        cls = cc.count_layout(f, C)
        size = np.bincount(cls, minlength=C)
        assert cls.min() >= 0 and size.size == C and (size[C - 3 :] >= 3).all() and (size > 0).all()


# ---- shape layouts: what a wrong class sum looks like
@pytest.mark.parametrize("lanes", cc.LANES)
def test_shape_layout_faults_are_visible(base, lanes):
    """Every non-empty edge class: without its first rank, without its last rank, without one lane's share (the ranks = st - 1 mod
    st; 8 and 64 lanes), and the class behind it with that class's last member added: each is refused on one utterance at least."""
    g, f, V, lens, post = base
    cls, C, facts = cc.shape_layout(f, lanes, cc.SHAPE_SEED, "own")
    n_mut, least = 0, np.inf
    per_utt = []
    for b in range(2):
        x, z = post[b]
        xi = cc.class_sums(x, cls, C)
        per_utt.append((x, z, xi, cc.structural(cls, C, f, int(lens[b]), cc.N)))
    for c, n in facts["edge"].items():
        mem = np.flatnonzero(cls == c)  # (entry order: the class's ranks)
        muts = {"first rank dropped": (c, -1.0, mem[:1]), "last rank dropped": (c, -1.0, mem[-1:]),
                "last member summed into the next class": (c + 1, 1.0, mem[-1:])}
        if lanes > 1 and n >= lanes:
            muts["one lane's share dropped"] = (c, -1.0, mem[lanes - 1 :: lanes])
        for what, (row, sign, ks) in muts.items():
            seen, over = False, 0.0
            for x, z, xi, exact in per_utt:
                m = xi.copy()
                m[row] += sign * x[ks].sum(axis=0)
                s, o = visible(m, xi, z, exact)
                seen, over = seen or s, max(over, o)
            n_mut += 1
            least = min(least, over)
            assert seen, (lanes, c, n, what, over)
    print(f"{lanes} lane(s) per class: {n_mut} mutations, each refused; the least visible at {least:.3g} of the bar")


# ---- count layouts: the last class's score / cost
def _scores_of(C, b):
    """U of utterance b as test_gpu_class_entries.run_scored draws it (N(0, 1), a few -inf)."""
    return tgs._scores(40, 2, cc.N, C)[b].astype(np.float64)


@pytest.mark.parametrize("nt", [cc.NT, cc.NT_TWO_WAVES])
def test_count_layout_last_class_score_is_visible(base, nt):
    """scoredposteriors: U of class C - 1 read as 0, and (C > NT) read as class NT - 1's: gamma or xi is refused."""
    g, f, V, lens, _ = base
    for C in cc.count_values(nt):
        cls = cc.count_layout(f, C)
        muts = ["zero"] + (["clamped"] if C > nt else [])
        for what in muts:
            seen = False
            for b in range(2):
                L = int(lens[b])
                U = _scores_of(C, b)
                Um = U.copy()
                Um[:, C - 1] = 0.0 if what == "zero" else U[:, nt - 1]
                g0, x0, z0, e0 = sr.reference(g, f, cls, C, U, V[b].astype(np.float64), L, cc.N)
                g1, x1, z1, _ = sr.reference(g, f, cls, C, Um, V[b].astype(np.float64), L, cc.N)
                try:
                    acr.check(x1.astype(np.float32), z1, x0, z0, e0)
                    check_gamma(g1.astype(np.float32)[None], g0[None], [L])
                except AssertionError:
                    seen = True
            assert seen, (nt, C, what)


@pytest.mark.parametrize("nt", [cc.NT, cc.NT_TWO_WAVES])
def test_count_layout_last_class_cost_is_visible(base, nt):
    """classcost: A of class C - 1 read as 0, and (C > NT) read as class NT - 1's: risk or grad is refused."""
    g, f, V, lens, _ = base
    for C in cc.count_values(nt):
        cls = cc.count_layout(f, C)
        A, D = tgc._costs(40, 2, cc.N, C, g.P)
        for what in ["zero"] + (["clamped"] if C > nt else []):
            seen = False
            for b in range(2):
                L = int(lens[b])
                Ab, Db = A[b].astype(np.float64), D[b].astype(np.float64)
                Am = Ab.copy()
                Am[:, C - 1] = 0.0 if what == "zero" else Ab[:, nt - 1]
                ref = ccr.reference(g, f, cls, V[b].astype(np.float64), Ab, Db, L, cc.N)
                mut = ccr.reference(g, f, cls, V[b].astype(np.float64), Am, Db, L, cc.N)
                try:
                    ccr.check(np.float32(mut[0]), mut[1].astype(np.float32), mut[3], ref, Ab, Db, L)
                except AssertionError:
                    seen = True
            assert seen, (nt, C, what)


# ---- the 70 000-state graph: classes of the arcs beyond 16 bits
def test_high_state_classes_carry_mass_and_a_16_bit_index_is_visible(mm, wl, oracle):
    gs, V, _, lens, _ = ti.case_random_big(wl)
    g = gs[0]
    f = wl.to_fsm(mm, g)
    cls, C = cc.high_layout(g, f)
    assert C == cc.HIGH_C == 82
    i, j, _ = ar.fsm_entries(f)
    high = ((i >= cc.HIGH) & (i < g.S)) | ((j >= cc.HIGH) & (j < g.S))
    assert ((cls >= 41) == high).all() and high.sum() > 0 and (~high).sum() > 0
    size = np.bincount(cls, minlength=C)
    top = np.zeros(C)
    seen = {"row": False, "col": False}
    for b in range(2):
        L, Vb = int(lens[b]), V[b].astype(np.float64)
        x, z = cc.entry_posteriors(oracle, g, f, Vb, L, V.shape[1])
        xi = cc.class_sums(x, cls, C)
        ref, z2, exact = acr.reference(*oracle, g, f, cls, C, Vb, L, V.shape[1])
        assert np.abs(xi - ref).max() <= 1e-12 and abs(z - z2) <= 1e-9 * abs(z)
        top = np.maximum(top, xi.max(axis=1))
        for what in seen:
            xm, _ = cc.entry_posteriors(oracle, g, f, Vb, L, V.shape[1], cut=what)
            s, over = visible(cc.class_sums(xm, cls, C), ref, z2, exact)
            print(f"utterance {b}: {what} indices of the records cut to 16 bits: {over:.3g} of the bar")
            seen[what] = seen[what] or s
    print("the largest xi of the high classes:", np.array2string(top[41:], precision=2))
    assert (top[41:][size[41:] > 0] > 10 * 1e-6).all(), top[41:]
    assert (size[41 : 41 + g.P] > 0).all()
    assert seen["row"] and seen["col"], seen


# ---- the float32 floor of the new classcost cases
def test_classcost_floor_table_covers_the_new_cases(mm, wl):
    """profiles/classcost_floor.json (tools/measure_classcost_floor.py) has every classcost input of tests/test_gpu_class_entries.py,
    measured on the CPU; none above the floor the gradient's bar was derived from."""
    import test_gpu_class_entries as tce

    with open(os.path.join(ROOT, "profiles", "classcost_floor.json")) as fh:
        table = json.load(fh)
    names = {r["case"] for r in table["rows"]}
    want = tce.classcost_case_names()
    assert len(want) == len(set(want)) and len(want) >= 20
    for name in want:
        assert name in names, (name, sorted(names))
    assert max(r["grad_err_over_G"] for r in table["rows"]) <= ccr.GRAD_F32_FLOOR
    assert table["worst_grad_err_over_G"] <= ccr.GRAD_F32_FLOOR
