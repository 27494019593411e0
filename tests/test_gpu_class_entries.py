"""The three arc-class entries -- arcclassposteriors, scoredposteriors, classcost -- at the class shapes, class counts and instances
their own test files leave alone, on the MI355X against the float64 references the entries already have:

  S. every width of the class pass (1, 8, 64 lanes per class) on layouts whose class sizes are chosen against the pass's stride and
     its four-way unrolled loop, several trips of its class loop with a partial last one, the phony self-loop in a class of its
     own, inside the large class and without a class; each width again on a two-wave block;
  T. the number of ranks on either side of the two thresholds between the widths (2 C, 32 C), and at the block size and at
     MM_CLASS_UNROLL blocks (the term loop's two loops), at 512 and at 128 threads;
  C. the class count at the block size, C = NT - 2 .. NT + 2 (the staging of the score / cost row: `tid < C`, `C > NT`, the four
     paddings of C + 1), at 512 and at 128 threads;
  H. the 70 000-state graph alone and in one batch with a 40-state graph in either order: <0,global> with no environment switch,
     classes of their own for the arcs with a state beyond 16 bits at either end, term rows in global memory at two different
     offsets, two widths of the class pass in one launch;
  W. rows of hundreds of arcs (`ergodic300`, `lexicon`) at the production plan and streamed.
  (P, the pdf count at the block size, is test_gpu_itemform_entries.test_pdf_count_at_the_block_size: boundary_entry below.)

Every test asserts by name, from kernels() of the batch that ran, the instance, the term-row placement and (arcclass, scored) the
lanes per class, and prints that text and its worst error over the bar.  No comparison here has a bar of its own: they are
arcclass_reference.check, check_gamma and classcost_reference.check (with GRAD_ABS_A) through the _check / _run_case helpers of the
three entries' test files.  A reference is computed once per utterance and shared within the module (shared_references).  The
layouts are tests/class_cases.py; tests/test_class_inputs.py shows from the references alone that the faults these shapes are
there for would be seen."""
import contextlib
import re
import types

import numpy as np
import pytest

import arcclass_reference as acr
import class_cases as cc
import classcost_reference as ccr
import scored_reference as sr
import test_gpu_arcclassposteriors as ta
import test_gpu_classcost as tc
import test_gpu_itemform as ti
import test_gpu_scoredposteriors as ts
from test_gpu_parity import _with_env

pytestmark = pytest.mark.gpu

STREAMED = ti.STREAMED
TWO_WAVES = {"MM_DEBUG": "1", "MM_NWAVES": "2"}
ENVS = {cc.NT: {}, cc.NT_TWO_WAVES: TWO_WAVES}
RESIDENT = (8, "lds")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# ---- the references: one per utterance, computed once and shared among the tests of this module (never modified)
_REFS = {}


def _key(x):
    if x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating)):
        return x
    if isinstance(x, np.ndarray):
        return (x.shape, str(x.dtype), hash(np.ascontiguousarray(x).tobytes()))
    if hasattr(x, "state2pdf"):  # a GraphSpec
        return (x.name, x.S, x.P, _key(np.asarray(x.state2pdf)), _key(np.asarray(x.w)))
    if isinstance(x, types.ModuleType) or hasattr(x, "colptr"):  # the oracle's modules; the FSM (made from the graph)
        return None
    raise TypeError(type(x))


@contextlib.contextmanager
def shared_references():
    """Inside, the three float64 references the entries' _check helpers call answer a repeated question from the store."""
    saved = [(m, m.reference) for m in (acr, sr, ccr)]

    def memo(mod, fn):
        def reference(*args):
            key = (mod.__name__,) + tuple(_key(a) for a in args)
            if key not in _REFS:
                _REFS[key] = fn(*args)
            return _REFS[key]

        return reference

    for m, fn in saved:
        m.reference = memo(m, fn)
    try:
        yield
    finally:
        for m, fn in saved:
            m.reference = fn


# ---- what kernels() must say
def says(k):
    """The instance names and everything from the class cap / lanes on: what the test's output shows of kernels()."""
    tail = min((k.index(s) for s in ("; class", "; terms in") if s in k), default=len(k))
    return " + ".join(re.findall(r"mm_\w+_kernel<[^>]*>", k)) + k[tail:]


def assert_lanes(k, lanes):
    assert cc.lanes_text(*lanes) + "; terms in " in k, (lanes, k)


def planned_lanes(f, cls, C):
    """The width the plan of (f, cls) lands on: its ranks are the classified entries that have a slot, the phony self-loop among them."""
    kp = cc.phony_entry(f)
    return cc.lanes_for(int((cls[cc.ranked_entries(f)] >= 0).sum()) + int(cls[kp] >= 0), C)


def _set(bf, gs, clss, nc):
    assert bf.set_arc_classes(clss[0] if all(g is gs[0] for g in gs) else clss, nc) == nc


# ---- one entry on one batch: the entry's own helpers.  inst = (NI, where); terms = "lds" / "global"; lanes = the widths of the launch
def run_arcclass(mm, wl, oracle, gs, clss, nc, V, lens, env, inst, terms, lanes, what, M=None):
    def run():
        fs, bf = ta._batch(mm, wl, gs)
        _set(bf, gs, clss, nc)
        k = ta._is(bf, inst[0], inst[1], terms)
        assert_lanes(k, lanes)
        if M is not None:
            assert bf.info()["arcclass_max_M"] == M and bf.info()["arcclass_C"] == nc
        print(f"[class] {what}: arcclass: {says(k)}")
        xi, ttl = bf.arcclassposteriors(V, lens)
        assert xi.shape == (len(gs), nc, V.shape[1])
        with shared_references():
            worst = ta._check(oracle, gs, fs, clss, nc, V, lens, xi, ttl, None, f"[class] {what}: arcclass")
        print(f"[class] {what}: arcclass: worst error over its bar {worst:.3g}")
        return bf

    return _with_env(env, run)


def run_scored(mm, wl, gs, clss, nc, V, lens, env, inst, terms, lanes, what, M=None, with_u=(True, False)):
    def run():
        fs, bf = ta._batch(mm, wl, gs)
        _set(bf, gs, clss, nc)
        k = ts._is(bf, inst[0], inst[1], terms)
        assert_lanes(k, lanes)
        if M is not None:
            assert bf.info()["arcclass_max_M"] == M
        print(f"[class] {what}: scored: {says(k)}")
        for given in with_u:
            U = ts._scores(40, len(gs), V.shape[1], nc) if given else None
            gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
            assert xi.shape == (len(gs), nc, V.shape[1]) and gamma.shape == V.shape
            with shared_references():
                worst = ts._check(gs, fs, clss, nc, U, V, lens, gamma, xi, ttl, None, f"[class] {what}: scored, U {'given' if given else 'NULL'}")
            print(f"[class] {what}: scored, U {'given' if given else 'NULL'}: worst error over its bars {worst:.3g}")
        return bf

    return _with_env(env, run)


def run_classcost(mm, wl, case):
    """tc._run_case (risk, grad, ttl by classcost_reference.check with GRAD_ABS_A, gamma by check_gamma; D given and D NULL)."""
    with shared_references():
        bf, _ = tc._run_case(mm, wl, case)
    print(f"[class] {case[0]}: classcost: {says(_with_env(case[1], lambda: bf.kernels('classcost')))}")
    return bf


def run_entry(entry, mm, wl, oracle, gs, clss, nc, V, lens, env, inst, terms, lanes, what, M=None):
    if entry == "arcclass":
        return run_arcclass(mm, wl, oracle, gs, clss, nc, V, lens, env, inst, terms, lanes, what, M)
    if entry == "scored":
        return run_scored(mm, wl, gs, clss, nc, V, lens, env, inst, terms, lanes, what, M)
    assert entry == "classcost"
    return run_classcost(mm, wl, (what, env, inst[0], inst[1], gs, clss, nc, V, lens))


def base(mm, wl):
    g = cc.base_graph(wl)
    f = wl.to_fsm(mm, g)
    V, lens = cc.base_inputs(g)
    info = mm.compile(f, mm.statemap(g.state2pdf, g.P)).info()
    assert 64 * min(8, max(info["packed_items"]) + 1) == cc.NT  # (NW = min(items + 1, 8): NT is a fact, not a hope)
    return g, f, V, lens


# ---- S. class shapes
@pytest.mark.parametrize("phony", cc.PHONY_VARIANTS)
@pytest.mark.parametrize("lanes", cc.LANES)
@pytest.mark.parametrize("entry", ["arcclass", "scored"])
def test_class_shapes(mm, wl, oracle, torch, entry, lanes, phony):
    g, f, V, lens = base(mm, wl)
    cls, C, facts = cc.shape_layout(f, lanes, cc.SHAPE_SEED, phony)
    assert planned_lanes(f, cls, C) == lanes
    # (behind the utterance the phony self-loop's class alone holds 1, exactly: arcclass_reference.frame_rule, checked as structural)
    run_entry(entry, mm, wl, oracle, [g, g], [cls, cls], C, V, lens, {}, RESIDENT, "lds", [lanes], f"shapes on {lanes} lane(s), phony {phony}", facts["M"])


@pytest.mark.parametrize("lanes", cc.LANES)
@pytest.mark.parametrize("entry", ["arcclass", "scored"])
def test_class_shapes_on_two_waves(mm, wl, oracle, torch, entry, lanes):
    """NW = 2: many trips of the class loop (549 classes on one lane each: 5 trips; 69 on 8: 5; 13 on 64: 7, a wave per class)."""
    g, f, V, lens = base(mm, wl)
    cls, C, facts = cc.shape_layout(f, lanes, cc.SHAPE_SEED, "own")
    run_entry(entry, mm, wl, oracle, [g, g], [cls, cls], C, V, lens, TWO_WAVES, RESIDENT, "lds", [lanes], f"shapes on {lanes} lane(s), two waves", facts["M"])


# ---- T. thresholds and rank counts
@pytest.mark.parametrize("M,lanes", list(zip(cc.threshold_values(cc.THRESHOLD_C), (1, 8, 8, 64))), ids=["2C-1", "2C", "32C-1", "32C"])
@pytest.mark.parametrize("entry", ["arcclass", "scored"])
def test_width_thresholds(mm, wl, oracle, torch, entry, M, lanes):
    """The width flips 1 -> 8 at M = 2 C and 8 -> 64 at M = 32 C, exactly; M is read back from info()."""
    g, f, V, lens = base(mm, wl)
    C = cc.THRESHOLD_C
    cls = cc.threshold_layout(f, C, M)
    assert cc.lanes_for(M, C) == lanes
    run_entry(entry, mm, wl, oracle, [g, g], [cls, cls], C, V, lens, {}, RESIDENT, "lds", [lanes], f"M = {M}, C = {C}", M)


@pytest.mark.parametrize("q", range(6), ids=["NT-1", "NT", "NT+1", "8NT-1", "8NT", "8NT+1"])
@pytest.mark.parametrize("nt", [cc.NT, cc.NT_TWO_WAVES])
@pytest.mark.parametrize("entry", ["arcclass", "scored"])
def test_rank_count_at_the_block_size(mm, wl, oracle, torch, entry, nt, q):
    """5 classes; every M is below the term cap: terms in LDS."""
    g, f, V, lens = base(mm, wl)
    M = cc.rank_values(nt)[q]
    cls = cc.rank_layout(f, M)
    run_entry(entry, mm, wl, oracle, [g, g], [cls, cls], 5, V, lens, ENVS[nt], RESIDENT, "lds", [cc.lanes_for(M, 5)], f"M = {M} at {nt} threads", M)


# ---- C. the class count at the block size
@pytest.mark.parametrize("off", [-2, -1, 0, 1, 2], ids=["NT-2", "NT-1", "NT", "NT+1", "NT+2"])
@pytest.mark.parametrize("nt", [cc.NT, cc.NT_TWO_WAVES])
@pytest.mark.parametrize("entry", ["scored", "classcost", "arcclass"])
def test_class_count_at_the_block_size(mm, wl, oracle, torch, entry, nt, off):
    """Every entry of the graph has a class: 9 704 ranks over C classes are 8 lanes per class at 512 threads (8 trips of 8 waves) and
    64 lanes at 128 (65 trips of 2 waves)."""
    g, f, V, lens = base(mm, wl)
    C = nt + off
    cls = cc.count_layout(f, C)
    lanes = {cc.NT: 8, cc.NT_TWO_WAVES: 64}[nt]
    assert planned_lanes(f, cls, C) == lanes
    run_entry(entry, mm, wl, oracle, [g, g], [cls, cls], C, V, lens, ENVS[nt], RESIDENT, "lds", [lanes], count_name(C, nt), f.nnz)


# ---- H. beyond 16-bit indices
def high_case(mm, wl, which):
    """(graphs, class arrays, C, V, lens): the 70 000-state graph with cc.high_layout, the 40-state one with its destination pdfs in
    the same 82 classes."""
    gs, V, _, lens, _ = ti.case_random_big(wl) if which == "alone" else ti.case_mixed(wl, which == "big_first")
    made = {}
    for g in gs:
        if id(g) not in made:
            f = wl.to_fsm(mm, g)
            made[id(g)] = cc.high_layout(g, f)[0] if g.S > cc.HIGH else cc.dst_layout(g, f, cc.HIGH_C)[0]
    return gs, [made[id(g)] for g in gs], cc.HIGH_C, V, lens


@pytest.mark.parametrize("which", ["alone", "big_first", "small_first"])
@pytest.mark.parametrize("entry", ["arcclass", "scored", "classcost"])
def test_beyond_16_bit_indices(mm, wl, oracle, torch, entry, which):
    """<0,global> with no environment switch; 301 333 ranks: term rows in global memory.  In the mixed batches the small graph's
    term rows lie behind or before the big one's (ClassDev::term_off with two different M), and its 184 ranks over 82 classes are
    summed on 8 lanes while the big graph's are summed on 64: the widths kernels() names are those the two plans' M give."""
    gs, clss, C, V, lens = high_case(mm, wl, which)
    assert [g.S for g in gs] == {"alone": [70000, 70000], "big_first": [70000, 40], "small_first": [40, 70000]}[which]
    own_m = {}
    for g, cls in zip(gs, clss):  # each plan's own M, from info() of a batch of that utterance alone
        if id(g) not in own_m:
            _, one = ta._batch(mm, wl, [g])
            one.set_arc_classes(cls, C)
            own_m[id(g)] = one.info()["arcclass_max_M"]
    lanes = [cc.lanes_for(own_m[id(g)], C) for g in gs]
    assert lanes == {"alone": [64, 64], "big_first": [64, 8], "small_first": [8, 64]}[which]
    run_entry(entry, mm, wl, oracle, gs, clss, C, V, lens, {}, (0, "global"), "global", lanes, high_name(which))


# ---- W. wide rows
@pytest.mark.parametrize("streamed", [False, True], ids=["production", "streamed"])
@pytest.mark.parametrize("name", ["ergodic300", "lexicon"])
@pytest.mark.parametrize("entry", ["arcclass", "scored", "classcost"])
def test_wide_rows(mm, wl, oracle, torch, entry, name, streamed):
    """Destination-pdf classes.  ergodic300: 90 301 ranks, term rows in global memory; lexicon: 6 541, in LDS."""
    gs, clss, nc, V, lens = wide_case(mm, wl, name)
    run_entry(entry, mm, wl, oracle, gs, clss, nc, V, lens, STREAMED if streamed else {}, (0, "global") if streamed else RESIDENT,
              {"ergodic300": "global", "lexicon": "lds"}[name], [64], wide_name(name, streamed))


def wide_case(mm, wl, name):
    gs, V, _, lens, _ = ti.case_wide(wl, name)
    cls, nc = cc.dst_layout(gs[0], wl.to_fsm(mm, gs[0]))
    return gs, [cls, cls], nc, V, lens


# ---- P. the pdf count at the block size (test_gpu_itemform_entries.test_pdf_count_at_the_block_size calls this)
def boundary_entry(entry, mm, wl, oracle, case, env, NT):
    """Destination-pdf classes: C = P + 1, so the score and cost rows see C = NT, NT + 1, NT + 2 as well."""
    gs, V, _, lens, _ = case
    f = wl.to_fsm(mm, gs[0])
    cls, nc = cc.dst_layout(gs[0], f)
    assert nc == gs[0].P + 1 and planned_lanes(f, cls, nc) == 8
    return run_entry(entry, mm, wl, oracle, gs, [cls, cls], nc, V, lens, env, RESIDENT, "lds", [8], boundary_name(gs[0].P, NT))


# ---- the classcost inputs of this file by name: what tools/measure_classcost_floor.py measures the float32 floor on
def count_name(C, nt):
    return f"C = {C} at {nt} threads"


def high_name(which):
    return {"alone": "70000 states, high classes", "big_first": "70000 + 40 states, high classes", "small_first": "40 + 70000 states, high classes"}[which]


def wide_name(name, streamed):
    return f"{name}, destination classes" + (", streamed" if streamed else "")


def boundary_name(P, NT):
    return f"P = {P} at {NT} threads, destination classes"


def classcost_case_names():
    return ([count_name(C, nt) for nt in ENVS for C in cc.count_values(nt)] + [high_name(w) for w in ("alone", "big_first", "small_first")] +
            [wide_name(n, s) for n in ("ergodic300", "lexicon") for s in (False, True)] +
            [boundary_name(nt + off, nt) for nt in ENVS for off in (-1, 0, 1)])


def classcost_cases(mm, wl):
    """Every classcost input of this file and of group P as test_gpu_classcost's case tuples (name, env, NI, where, graphs, class
    arrays, C, V, lens); A and D come from test_gpu_classcost._costs(40, ...), as _run_case draws them."""
    import test_gpu_itemform_entries as tn

    out = []
    g, f, V, lens = base(mm, wl)
    for nt, env in ENVS.items():
        for C in cc.count_values(nt):
            cls = cc.count_layout(f, C)
            out.append((count_name(C, nt), env, 8, "lds", [g, g], [cls, cls], C, V, lens))
    for which in ("alone", "big_first", "small_first"):
        gs, clss, C, Vh, lh = high_case(mm, wl, which)
        out.append((high_name(which), {}, 0, "global", gs, clss, C, Vh, lh))
    for name in ("ergodic300", "lexicon"):
        gs, clss, nc, Vw, lw = wide_case(mm, wl, name)
        for streamed in (False, True):
            out.append((wide_name(name, streamed), STREAMED if streamed else {}, 0 if streamed else 8, "global" if streamed else "lds", gs, clss, nc, Vw, lw))
    for block in ("production", "two_waves"):
        for off in (-1, 0, 1):
            case, env, NT = tn._boundary_case(mm, wl, "classcost", block, off)
            gs, Vp, _, lp, _ = case
            cls, nc = cc.dst_layout(gs[0], wl.to_fsm(mm, gs[0]))
            out.append((boundary_name(gs[0].P, NT), env, 8, "lds", gs, [cls, cls], nc, Vp, lp))
    assert [c[0] for c in out] == classcost_case_names()
    return out
