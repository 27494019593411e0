"""The item-form entries at the row shapes, index widths and pdf counts no other test gives them, on the MI355X against the float64
references (vitwindow: the float32 restatement, bit for bit) the entries already have:

  W. rows of hundreds of arcs in both directions -- the cases of test_gpu_itemform.case_wide -- for leakyposteriors, pathentropy,
     filterposteriors, windowposteriors, segmentposteriors and viterbiwindow, at the production plan and (`wide`) streamed;
  H. the 70 000-state graph of test_gpu_itemform.case_random_big, alone and in one batch with a 40-state graph in either order
     (case_mixed), for the same six entries: <0,global> with no environment switch, every utterance's state_out / end_out slice at
     its state_offsets;
  P. the pdf count at the block size: P = NT - 1, NT, NT + 1 for all thirteen item-form entries and pdfposteriors on the item kernel.

Every test asserts by name, from kernels() of the batch that ran, the instance it claims to run.  No comparison here has a bar of
its own: they are the _check / check_against_reference / _check_batch helpers of the entries' own test files, check_gamma,
entropy_reference.check, arc_reference.check, cost_reference.check, the Bernstein rule of test_gpu_samplepaths._size_check, and bit
equality for viterbiwindow.

The block size of group P.  NT = 64 NW.  pick_geometry gives NW = min(16, items + 1), items = max(info()["packed_items"]);
item_plan caps it at 8 for arcs, cost, leaky, entropy, filter, window, segment and weighted; pdfposteriors, samplepaths and
viterbiwindow (the Tropical plan with 8 resident items: min(16, max(items + 1, (items + 3) / 4)) = min(16, items + 1)) keep it.
random_fsm(700, P, 3.0, seed=9) packs 21 items whatever P is (P only draws state2pdf), so NT = 512 for the capped entries and
1024 for the other three: each entry gets the P that matches ITS block.  Both are asserted from info().  The second block,
NT = 128 for every entry, comes from MM_DEBUG=1 MM_NWAVES=2 on random_fsm(200, P, 3.0, seed=9); kernels() does not name the
block size, so that one rests on the switch being honoured (mm_engine.hip, pick_geometry).

The input builders and the conditions on them are module-level and need no GPU: tests/test_itemform_inputs.py runs the references
alone on them (a lost arc of a wide row, a state index cut to 16 bits and a wrong emission of the last pdfs are each visible to
the comparisons used here)."""
import contextlib
import dataclasses
import io

import numpy as np
import pytest

import entropy_reference as er
import filter_reference as fr
import test_gpu_filterposteriors as tf
import test_gpu_itemform as ti
import test_gpu_leakyposteriors as tl
import test_gpu_pathentropy as te
import test_gpu_segmentposteriors as tsg
import test_gpu_viterbiwindow as tv
import test_gpu_weightedposteriors as tw
import test_gpu_windowposteriors as twn
import test_segmentposteriors as cs
import test_viterbiwindow as cv
import test_windowposteriors as cw
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu

STREAMED = ti.STREAMED
ITEM = ti.ITEM
TWO_WAVES = {"MM_DEBUG": "1", "MM_NWAVES": "2"}
LEAK = 0.1
NEW_ENTRIES = ["leaky", "entropy", "filter", "window", "segment", "vitwindow"]
ALL_ENTRIES = ["pdfposteriors", "arcs", "sample", "cost", "leaky", "entropy", "filter", "window", "segment", "weighted", "vitwindow",
               "arcclass", "scored", "classcost"]
CLASS_ENTRIES = ("arcclass", "scored", "classcost")  # (run by tests/test_gpu_class_entries.boundary_entry: destination-pdf classes, C = P + 1)
UNCAPPED = ("pdfposteriors", "sample", "vitwindow")  # (the entries whose plan keeps up to 16 waves)
WIDE_NAMES = ["wide", "ergodic300", "lexicon"]
# segmentposteriors' end modes per utterance: the three of them across the group's batches of two
WIDE_MODES = {"wide": (2, 1), "ergodic300": (0, 2), "lexicon": (2, 0)}
# viterbiwindow's resident items on those graphs: 22 and 52 packed items fit 8 in each of 16 waves, ergodic300's 301 do not
WIDE_VITWINDOW_NI = {"wide": 8, "ergodic300": 0, "lexicon": 8}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# ---- the inputs
def drop_cost(case):
    gs, V, _, lens, _ = case
    return gs, V, lens


def case_pdf_boundary(wl, S, P):
    """random_fsm(S, P, 3.0, seed=9) with the states at the head of the accepting chain emitting from the pdfs P-8 .. P-1, two
    utterances of 14 frames (lengths 14 and 9); the cost of the cost entry."""
    g = wl.random_fsm(S, P, 3.0, seed=9)
    s2p = np.array(g.state2pdf, copy=True)
    s2p[:8] = (P - 1 - np.arange(8)) % P
    g = dataclasses.replace(g, state2pdf=s2p)
    V = np.random.default_rng(10).standard_normal((2, 14, P)).astype(np.float32)
    cost = np.random.default_rng(11).standard_normal((2, 14, P)).astype(np.float32)
    return [g, g], V, cost, np.array([14, 9], dtype=np.int32), None


def block_threads(entry, items, env=None):
    """The threads of a workgroup of `entry` on a graph of `items` packed items (item_plan; MM_NWAVES as pick_geometry reads it)."""
    nw = min(16, items + 1)
    if env and "MM_NWAVES" in env:
        nw = int(env["MM_NWAVES"])
    return 64 * (nw if entry in UNCAPPED else min(nw, 8))


def window_args(lens):
    """One closed and one open utterance (alternating), the commit frame at half the length."""
    B = len(lens)
    return np.array([1, 0] * B, dtype=np.int32)[:B], (np.asarray(lens) // 2).astype(np.int32)


def _vector(g, L, what, holes):
    """A float32 vector [S + 1] of ln U(0, 1) with `holes` of its real entries at -inf, drawn from (S, L, what) alone: an
    utterance gets the same vector in whichever batch it stands, so that its reference is shared."""
    rng = np.random.default_rng([g.S, int(L), what])
    v = np.log(rng.random(g.S + 1)).astype(np.float32)
    if holes:
        v[rng.choice(g.S, size=holes, replace=False)] = -np.inf
    return v


def segment_args(gs, lens, modes):
    """state_in: NULL for the longest utterance(s), a random vector for the others; end_in: a random vector with -inf at one real
    state in twenty (read where the mode is 2)."""
    states = [None if L == max(lens) else _vector(g, L, 1, 0) for g, L in zip(gs, lens)]
    end = [_vector(g, L, 2, max(1, g.S // 20)) for g, L in zip(gs, lens)]
    return np.asarray(modes, dtype=np.int32), states, end


def tropical_inputs(gs, V):
    """Every weight and (2 x) every emission on the 1/16 grid, as test_viterbiwindow.case_base(rounded=True)."""
    grid = {}
    for g in gs:
        if id(g) not in grid:
            grid[id(g)] = cv.on_grid(g)
    return [grid[id(g)] for g in gs], (np.round(2.0 * V.astype(np.float64) * 16) / 16).astype(np.float32)


# ---- the references: one per utterance, computed once and shared among the tests of this module (never modified)
_REFS = {}


def _h(x):
    return None if x is None else hash(np.ascontiguousarray(x).tobytes())


def shared_reference(entry, g, Vb, L, N, extra, make):
    key = (entry, g.name, g.S, g.P, _h(g.state2pdf), _h(g.w), _h(Vb), int(L), int(N)) + tuple(extra)
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def filter_references(gs, V, lens):
    N = V.shape[1]
    return [shared_reference("filter", g, V[b], lens[b], N, (), lambda: fr.reference(g, V[b].astype(np.float64), int(lens[b]), N)) for b, g in enumerate(gs)]


def window_references(case):
    gs, V, lens, closed, commit = case
    one = lambda b: cw.references(([gs[b]], V[b : b + 1], lens[b : b + 1], closed[b : b + 1], commit[b : b + 1]))[0]  # noqa: E731
    return [shared_reference("window", g, V[b], lens[b], V.shape[1], (int(closed[b]), int(commit[b])), lambda: one(b)) for b, g in enumerate(gs)]


def segment_references(case):
    gs, V, lens, modes, states, end = case
    one = lambda b: cs.references(([gs[b]], V[b : b + 1], lens[b : b + 1], modes[b : b + 1], [states[b]], [end[b]]))[0]  # noqa: E731
    return [shared_reference("segment", g, V[b], lens[b], V.shape[1], (int(modes[b]), _h(states[b]), _h(end[b])), lambda: one(b)) for b, g in enumerate(gs)]


def vitwindow_references(gs, V, lens, closed, commit):
    one = lambda b: cv.references([gs[b]], V[b : b + 1], lens[b : b + 1], closed[b : b + 1], commit[b : b + 1], False)[0]  # noqa: E731
    return [shared_reference("vitwindow", g, V[b], lens[b], V.shape[1], (int(closed[b]), int(commit[b])), lambda: one(b)) for b, g in enumerate(gs)]


# ---- the instance names of kernels()
KERNELS = {"leaky": ("mm_leaky_fwd_kernel", "mm_leaky_bwd_kernel"), "entropy": ("mm_entropy_fwd_kernel", "mm_entropy_bwd_kernel"),
           "filter": ("mm_filter_kernel",), "window": ("mm_window_fwd_kernel", "mm_window_bwd_kernel"),
           "segment": ("mm_window_fwd_kernel", "mm_segment_bwd_kernel"), "vitwindow": ("mm_vitwindow_fwd_kernel",)}


def assert_instance(entry, k, NI, where):
    for name in KERNELS[entry]:
        assert f"{name}<{NI},{where}>" in k, (entry, NI, where, k)


def packed_items(mm, wl, gs, semiring="log"):
    return max(max(mm.compile(wl.to_fsm(mm, g, semiring), mm.statemap(g.state2pdf, g.P)).info()["packed_items"]) for g in {id(g): g for g in gs}.values())


def vitwindow_resident(mm, wl, gs):
    """item_plan's Tropical branch: 8 resident items per wave while the whole graph fits 8 items in each of 16 waves, else streamed."""
    return 8 if packed_items(mm, wl, gs, "tropical") <= 128 else 0


# ---- one entry on one batch: the entry's own helpers, the reference shared.  Returns kernels() of the batch that ran.
def run_entry(entry, mm, wl, oracle, gs, V, lens, env, what, modes=(2, 1)):
    if entry == "leaky":
        bf = _with_env(env, lambda: tl._batch(mm, wl, gs))
        gamma, ttl = bf.leakyposteriors(V, lens, leak=LEAK)
        assert np.isfinite(ttl).all()
        worst = tl._check(gamma, ttl, gs, V, lens, LEAK)
        print(f"[entries] {what}: leaky: worst log-posterior error over its bar {worst:.3g}")
        return bf.kernels("leaky")
    if entry == "entropy":
        bf_fs = _with_env(env, lambda: te._batch(mm, wl, gs))
        name = "entries: " + ", ".join(f"{g.name}/{g.P}" for g in gs) + f", V {_h(V)}"  # (the inputs, not the instance: shared)
        for b, g in enumerate(gs):  # (an utterance that stands in two batches: its reference into _check_batch's store, once)
            te._REFS[(name, b)] = shared_reference("entropy", g, V[b], lens[b], V.shape[1], (),
                                                   lambda: er.reference(*oracle, g, bf_fs[0][b], V[b].astype(np.float64), int(lens[b]), V.shape[1]))
        bf, H, grad, ttl, gamma = te._check_batch(mm, wl, oracle, (gs, V, lens, None), name, bf_fs)
        assert np.isfinite(ttl).all()
        worst = np.zeros(3)
        for b in range(len(gs)):  # (the figures entropy_reference.check printed above, gathered for one line)
            ref = te._reference(oracle, (name, b), gs[b], bf_fs[0][b], V[b], int(lens[b]), V.shape[1])
            with contextlib.redirect_stdout(io.StringIO()):
                he, _ = er.check(H[b], grad[b], ttl[b], ref, int(lens[b]))
            ge = float(np.max(np.abs(grad[b].astype(np.float64) - ref[1]) / (1e-4 * np.abs(ref[1]) + er.GRAD_ABS_A * np.abs(ref[1]).max())))
            worst = np.maximum(worst, (he, ge, check_gamma(gamma[b][None], ref[2][None], [int(lens[b])])))
        print(f"[entries] {what}: entropy: worst error over its bar: H {worst[0]:.3g}, grad {worst[1]:.3g}, gamma {worst[2]:.3g}")
        return bf.kernels("entropy")
    if entry == "filter":
        bf = _with_env(env, lambda: tf._batch(mm, wl, gs))
        out = tf._run(bf, V, lens)
        assert np.isfinite(out[2]).all()
        tf._check(bf, out, filter_references(gs, V, lens), lens, f"[entries] {what}: filter")
        return bf.kernels("filter")
    if entry == "window":
        case = (gs, V, lens) + window_args(lens)
        bf = _with_env(env, lambda: twn._batch(mm, wl, gs))
        out = twn._run(bf, case)
        assert np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
        twn._check(bf, out, window_references(case), lens, f"[entries] {what}: window")
        return bf.kernels("window")
    if entry == "segment":
        case = (gs, V, lens) + segment_args(gs, lens, modes)
        bf = _with_env(env, lambda: tsg._batch(mm, wl, gs))
        out = tsg._run(bf, case)
        assert np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
        tsg._check(bf, out, segment_references(case), lens, f"[entries] {what}: segment")
        return bf.kernels("segment")
    assert entry == "vitwindow"
    gs, V = tropical_inputs(gs, V)
    closed, commit = window_args(lens)
    bf = _with_env(env, lambda: tv._batch(mm, wl, gs))
    out = bf.viterbiwindow(V, lens, closed=closed, commit=commit, commit_converged=False, want_state=True)
    assert np.isfinite(out[1]).all()
    tv._check(bf, out, vitwindow_references(gs, V, lens, closed, commit), what)
    print(f"[entries] {what}: vitwindow: path, score, converged, ncommit, mcommit and state_out bit for bit")
    return bf.kernels("vitwindow")


# ---- W. wide rows
@pytest.mark.parametrize("name", WIDE_NAMES)
@pytest.mark.parametrize("entry", NEW_ENTRIES)
def test_wide_rows(mm, wl, oracle, torch, entry, name):
    """The production plan: <8,lds> (viterbiwindow on `ergodic300`: 301 items are more than 16 waves hold, its plan streams them)."""
    gs, V, lens = drop_cost(ti.case_wide(wl, name))
    k = run_entry(entry, mm, wl, oracle, gs, V, lens, {}, f"wide rows, {name}", WIDE_MODES[name])
    if entry == "vitwindow":
        assert vitwindow_resident(mm, wl, tropical_inputs(gs, V)[0]) == WIDE_VITWINDOW_NI[name]
    assert_instance(entry, k, WIDE_VITWINDOW_NI[name] if entry == "vitwindow" else 8, "lds")


@pytest.mark.parametrize("entry", NEW_ENTRIES)
def test_wide_rows_streamed(mm, wl, oracle, torch, entry):
    gs, V, lens = drop_cost(ti.case_wide(wl, "wide"))
    k = run_entry(entry, mm, wl, oracle, gs, V, lens, STREAMED, "wide rows, wide, streamed", WIDE_MODES["wide"])
    assert_instance(entry, k, 0, "lds" if entry == "vitwindow" else "global")  # (the tropical plan alone streams with its vectors in LDS)


# ---- H. beyond 16-bit state indices: the production route to <0,global>
@pytest.mark.parametrize("entry", NEW_ENTRIES)
def test_beyond_16_bit_indices(mm, wl, oracle, torch, entry):
    gs, V, lens = drop_cost(ti.case_random_big(wl))
    k = run_entry(entry, mm, wl, oracle, gs, V, lens, {}, "70000 states", (2, 1))
    assert_instance(entry, k, 0, "global")


@pytest.mark.parametrize("big_first", [True, False], ids=["big_first", "small_first"])
@pytest.mark.parametrize("entry", NEW_ENTRIES)
def test_mixed_batch_of_a_graph_beyond_16_bits_and_a_small_one(mm, wl, oracle, torch, entry, big_first):
    """Two state counts in one batch: the 40-state graph's slice of state_out / end_out lies behind or before the 70 002-state
    one's.  (The big graph's utterance is the one of test_beyond_16_bit_indices at the same place: its reference is shared.)"""
    gs, V, lens = drop_cost(ti.case_mixed(wl, big_first))
    assert [g.S for g in gs] == ([70000, 40] if big_first else [40, 70000])
    k = run_entry(entry, mm, wl, oracle, gs, V, lens, {}, f"70000 + 40 states, big first {big_first}", (2, 0) if big_first else (0, 1))
    assert_instance(entry, k, 0, "global")


# ---- P. the pdf count at the block size
def _boundary_case(mm, wl, entry, block, off):
    """The case whose P is `off` from the block size of `entry`, with the block size asserted from info()."""
    S, env = (700, {}) if block == "production" else (200, TWO_WAVES)
    items = packed_items(mm, wl, [wl.random_fsm(S, 8, 3.0, seed=9)], "tropical" if entry == "vitwindow" else "log")  # (P only draws state2pdf)
    NT = block_threads(entry, items, env)
    case = case_pdf_boundary(wl, S, NT + off)
    items = packed_items(mm, wl, case[0][:1], "tropical" if entry == "vitwindow" else "log")
    if block == "production":
        assert items >= (15 if entry in UNCAPPED else 7), items  # NW = min(items + 1, 16 or 8): NT is a fact, not a hope
        assert NT == (1024 if entry in UNCAPPED else 512)
    else:
        assert NT == 128
    assert block_threads(entry, items, env) == NT and case[0][0].P == NT + off
    if entry == "vitwindow":
        assert items <= 128  # (8 resident items: the plan's NW follows the items)
    return case, env, NT


@pytest.mark.parametrize("off", [-1, 0, 1], ids=["NT-1", "NT", "NT+1"])
@pytest.mark.parametrize("block", ["production", "two_waves"])
@pytest.mark.parametrize("entry", ALL_ENTRIES)
def test_pdf_count_at_the_block_size(mm, wl, oracle, torch, entry, block, off):
    case, env, NT = _boundary_case(mm, wl, entry, block, off)
    gs, V, cost, lens, _ = case
    what = f"P = {gs[0].P} at {NT} threads"
    print(f"[entries] {entry}: {what}")
    if entry == "pdfposteriors":
        k = ti._pdf_check(mm, wl, oracle, case, {**ITEM, **env})
        assert ti._item_fb_name(8, "lds") in k, k
    elif entry == "arcs":
        ti._arcs_are(_with_env(env, lambda: ti._arc_check(mm, wl, oracle, gs, V, lens, want_batch=True))[2].kernels("arcs"), 8, "lds")
    elif entry == "sample":
        ti._sample_is(_with_env(env, lambda: ti._size_check(mm, wl, oracle, gs, V, lens))[0].kernels("sample"), 8, "lds")
    elif entry == "cost":
        ti._cost_is(_with_env(env, lambda: ti._cost_check(mm, wl, oracle, case))[0].kernels("cost"), 8, "lds")
    elif entry == "weighted":
        _with_env(env, lambda: tw._run_case(mm, wl, torch, gs, V, lens, 89, "<8,lds>"))  # (asserts its instance itself)
    elif entry in CLASS_ENTRIES:
        import test_gpu_class_entries as tce

        tce.boundary_entry(entry, mm, wl, oracle, case, env, NT)  # (asserts its instance, lanes per class and term rows itself)
    else:
        assert_instance(entry, run_entry(entry, mm, wl, oracle, gs, V, lens, env, what, (2, 1)), 8, "lds")
