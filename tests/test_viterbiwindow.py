"""Windowed best paths (mm_viterbiwindow_f32) without a GPU: the bindings of the new entry, the argument checks that need no device,
and the NumPy restatement of tests/vitwindow_reference.py -- the header's definition -- against brute-force enumeration of every
state sequence of tiny graphs (path, score, surviving sets, convergence point, state_out and mcommit), against the consequences
the header states -- (b) finality, (c) re-windowing, bit for bit on the 1/16 grid in float32, (d) the level of a frame -- the
len = 0, c = 0 and no-path conventions, and the host replay of streaming.OnlineViterbi's policy against whole-audio best paths.
The cases of tests/test_gpu_viterbiwindow.py are built here, with the non-vacuity of their convergence points."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np

import vitwindow_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def on_grid(g):
    """The GraphSpec with every weight rounded to a multiple of 1/16: sums of a few hundred of them are exact in float32."""
    r = lambda x: np.round(np.asarray(x, dtype=np.float64) * 16) / 16
    return dataclasses.replace(g, w=r(g.w), final_w=r(g.final_w), init_w=r(g.init_w))


def case_base(wl, rounded=True, seed=11):
    """random_fsm(40, 6, 3.0, seed=1), B = 6, N = 40, lens = [40, 33, 1, 0, 38, 40]: emissions 2 N(0, 1) (rounded: to 1/16, as the
    FSM's weights), utterance 0 with some -inf entries in frame 8, utterance 4 dead at frame 4."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    if rounded:
        g = on_grid(g)
    B, N = 6, 40
    lens = np.array([40, 33, 1, 0, 38, 40], dtype=np.int32)
    V = 2.0 * np.random.default_rng(seed).standard_normal((B, N, g.P))
    V = (np.round(V * 16) / 16 if rounded else V).astype(np.float32)
    V[0, 7, [1, 4]] = -np.inf
    V[4, 3, :] = -np.inf
    return [g] * B, V, lens


# (closed, commit, commit_converged) of the base case: both end modes, commits 0, mid and beyond len, with and without the
# convergence point
BASE_MODES = [
    (np.array([0, 1, 0, 1, 0, 1], dtype=np.int32), np.array([0, 15, 5, 3, 20, 99], dtype=np.int32), False),
    (np.array([1, 0, 1, 0, 1, 0], dtype=np.int32), np.array([17, 0, 0, 0, 2, 0], dtype=np.int32), True),
    (None, None, False),
    (None, None, True),
]


def references(gs, V, lens, closed=None, commit=None, commit_converged=False, state_in=None, dtype=np.float32):
    """The restatement of every utterance (state_in: per utterance [S + 1] vectors or None)."""
    N = V.shape[1]
    sys = {}
    out = []
    for b, g in enumerate(gs):
        sys.setdefault(id(g), vr.system(g))
        out.append(vr.reference(g, V[b], int(lens[b]), N, None if state_in is None else state_in[b], bool(closed[b]) if closed is not None else False,
                                None if commit is None else int(commit[b]), commit_converged, dtype, sys[id(g)]))
    return out


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds its 18 parameters, the host interface and the
    Julia wrapper are there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_viterbiwindow_f32" in mm.SYMBOLS
    assert lib.mm_viterbiwindow_f32.argtypes is not None and len(lib.mm_viterbiwindow_f32.argtypes) == 18
    assert callable(mm.windowbestpath) and hasattr(mm.BatchedFSM, "viterbiwindow")
    assert hasattr(mm, "OnlineViterbi") and all(hasattr(mm.OnlineViterbi, k) for k in ("push", "finish", "reset"))
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_viterbiwindow_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_viterbiwindow_f32, LIB\)", src) and re.search(r"function viterbiwindow\(", src)


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: path or score NULL (-1), path_stride_b < N (-2); with those in
    order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(path=None, score=None, psb=8, N=8):
        return lib.mm_viterbiwindow_f32(None, p, 8, 1, None, N, None, None, None, 0, None, None, None, path, psb, score, None, None)

    assert call() == -1 and b"path/score is NULL" in lib.mm_last_error()
    assert call(path=p) == -1 and b"path/score is NULL" in lib.mm_last_error()
    assert call(path=p, score=p, psb=7) == -2 and b"path_stride_b" in lib.mm_last_error()
    assert call(path=p, score=p) == -1 and b"NULL batch" in lib.mm_last_error()


def _tiny(wl):
    """A pdf per state: with shared pdfs two orders of the same arcs weigh the same in exact arithmetic, and the roundings of the
    enumeration and of the recursion would decide such ties differently."""
    gs = [wl.l2r_hmm(3), wl.random_fsm(5, 3, mean_deg=2.0, seed=4), wl.random_fsm(4, 2, mean_deg=2.5, seed=9, n_init=3)]
    return [dataclasses.replace(g, state2pdf=np.arange(g.S, dtype=np.int32), P=g.S) for g in gs]


def test_reference_against_path_enumeration(wl):
    """Graphs of up to 5 states, up to 5 frames, both end modes, from alpha_hat and from a carried vector: path, score, every
    surviving set and the convergence point; state_out and mcommit at every commit frame."""
    rng = np.random.default_rng(61)
    seen_conv = set()
    for g in _tiny(wl):
        for L in (1, 3, 5):
            V = (2.0 * rng.standard_normal((5, g.P))).astype(np.float32)
            for state_in in (None, rng.standard_normal(g.S + 1)):
                for closed in (False, True):
                    r = vr.reference(g, V, L, 5, state_in, closed)
                    path, score, sets, conv = vr.enumerate_paths(g, V, L, state_in, closed)
                    what = (g.name, L, state_in is None, closed)
                    if not np.isfinite(score):
                        assert np.isneginf(r.score) and (r.path == -1).all() and r.converged == 0, what
                        continue
                    assert abs(r.score - score) <= 1e-10 and np.array_equal(r.path[:L], path) and (r.path[L:] == -1).all(), what
                    assert len(r.sets) == L and all(np.array_equal(a, e) for a, e in zip(r.sets, sets)), what
                    assert r.converged == conv, what
                    seen_conv.add(conv)
                for c in range(1, L + 1):
                    r = vr.reference(g, V, L, 5, state_in, False, c)
                    mc, so = vr.enumerate_commit(g, V, c, state_in)
                    assert r.ncommit == c and abs(r.mcommit - mc) <= 1e-10, (g.name, L, c)
                    m = np.isfinite(so)
                    assert (np.isneginf(r.state_out) == ~m).all() and np.abs(r.state_out[m] - so[m]).max() <= 1e-10, (g.name, L, c)
    assert len(seen_conv) >= 3, seen_conv  # the convergence point took several values, 0 among them or not


def test_conventions(wl):
    g = wl.random_fsm(5, 3, mean_deg=2.0, seed=4)
    rng = np.random.default_rng(62)
    V = rng.standard_normal((6, g.P)).astype(np.float32)
    sys = vr.system(g)
    st = rng.standard_normal(g.S + 1).astype(np.float32)
    for state_in, start in ((None, sys.pi), (st, st)):
        r = vr.reference(g, V, 0, 6, state_in, dtype=np.float32)  # len = 0
        assert (r.path == -1).all() and np.isneginf(r.score) and r.converged == 0 and r.ncommit == 0 and r.mcommit == 0
        assert np.array_equal(r.state_out, start)
        r = vr.reference(g, V, 4, 6, state_in, commit=0, dtype=np.float32)  # c = 0 with len > 0
        assert np.isfinite(r.score) and r.ncommit == 0 and r.mcommit == 0 and np.array_equal(r.state_out, start)
    # commit == NULL: len without commit_converged, the convergence point with it
    r = vr.reference(g, V, 4, 6)
    assert r.ncommit == 4
    r = vr.reference(g, V, 4, 6, commit_converged=True)
    assert r.ncommit == r.converged
    # no path: the window dies at frame 3 -- the prefix's state_out ahead of the death, -inf behind it
    Vd = V.copy()
    Vd[2] = -np.inf
    r = vr.reference(g, Vd, 4, 6, commit=2, commit_converged=True)
    assert np.isneginf(r.score) and (r.path == -1).all() and r.converged == 0 and r.ncommit == 2
    assert np.isfinite(r.mcommit) and np.isfinite(r.state_out).any()
    r = vr.reference(g, Vd, 4, 6, commit=3)
    assert np.isneginf(r.mcommit) and np.isneginf(r.state_out).all()
    assert not any(np.isnan(x).any() for x in (r.state_out, np.asarray(r.mcommit), np.asarray(r.score)))


def test_base_case_is_not_vacuous(wl):
    """Every full-length live utterance of the GPU tests' base case converges beyond half of its frames, rounded or not, in
    either end mode; the dead utterance has no path; ties are decided (the grid makes them likely)."""
    for rounded in (True, False):
        gs, V, lens = case_base(wl, rounded)
        N = V.shape[1]
        for closed in (np.zeros(6, dtype=np.int32), np.ones(6, dtype=np.int32)):
            refs = references(gs, V, lens, closed)
            conv = [r.converged for r in refs]
            print(f"base case (rounded {rounded}, closed {int(closed[0])}): converged {conv} of lens {lens.tolist()}")
            assert all(conv[b] >= N / 2 for b in (0, 5)), conv
            assert np.isneginf(refs[4].score) and refs[4].converged == 0 and np.isneginf(refs[3].score)
            assert all(np.isfinite(refs[b].score) for b in (0, 1, 2, 5))
        assert all(r.converged < lens[b] for b, r in enumerate(references(gs, V, lens)) if b in (0, 1, 5))  # ... and is not trivially len


def test_finality(wl):
    """(b): the path of an open window of 25 frames up to its convergence point is the path of every longer window from the same
    start, open or closed."""
    gs, V, lens = case_base(wl, rounded=False)
    short = references(gs, V, np.minimum(lens, 25))
    checked = 0
    for closed in (0, 1):
        long = references(gs, V, lens, np.full(6, closed, dtype=np.int32))
        for b in range(6):
            if lens[b] > 25 and np.isfinite(long[b].score):
                k = short[b].converged
                assert k >= 1 and np.array_equal(short[b].path[:k], long[b].path[:k]), (b, closed)
                assert not np.array_equal(short[b].path[:25], long[b].path[:25]) or k <= 25
                checked += 1
    assert checked == 6


def _rewindow(gs, V, lens, closed, c, dtype):
    first = references(gs, V, lens, closed, c, dtype=dtype)
    B, M, _ = V.shape
    V2 = np.zeros_like(V)
    for b in range(B):
        V2[b, : M - c[b]] = V[b, c[b] :]
    second = references(gs, V2, lens - c, closed, state_in=[r.state_out for r in first], dtype=dtype)
    return first, second


def test_rewindowing(wl):
    """(c): on the 1/16 grid the second window has the first's path behind c and score - mcommit, bit for bit in float32; on
    unrounded inputs in float64 the same path and the score to rounding."""
    closed = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    c = np.array([12, 20, 1, 0, 2, 39], dtype=np.int32)
    for rounded, dtype in ((True, np.float32), (False, np.float64)):
        gs, V, lens = case_base(wl, rounded)
        first, second = _rewindow(gs, V, lens, closed, c, dtype)
        for b in range(6):
            L, cb = int(lens[b]), int(min(c[b], lens[b]))
            assert np.array_equal(second[b].path[: L - cb], first[b].path[cb:L]), (b, rounded)
            if L == cb:  # nothing behind c: a window without a frame has no path
                assert np.isneginf(second[b].score)
            elif np.isfinite(first[b].score):
                want = first[b].score - first[b].mcommit
                assert second[b].score == want if rounded else abs(second[b].score - want) <= 1e-9, (b, rounded, second[b].score, want)
            else:
                assert np.isneginf(second[b].score)


def test_the_level_of_a_frame(wl):
    """(d): a constant on every emission of a frame moves score (and mcommit behind the frame) by it and nothing else."""
    gs, V, lens = case_base(wl, rounded=True)
    closed, commit, cc = BASE_MODES[0]
    base = references(gs, V, lens, closed, commit, cc)
    n = 5
    for shift in (100.0, -150.0):
        Vs = V.copy()
        Vs[:, n] += np.float32(shift)
        for b, (r, r0) in enumerate(zip(references(gs, Vs, lens, closed, commit, cc), base)):
            assert np.array_equal(r.path, r0.path) and r.converged == r0.converged and r.ncommit == r0.ncommit, (b, shift)
            if np.isfinite(r0.score):
                assert r.score == r0.score + np.float32(shift) * (lens[b] > n), (b, shift)
            assert r.mcommit == r0.mcommit + np.float32(shift) * (r0.ncommit > n) or np.isneginf(r0.mcommit)
            assert np.array_equal(r.state_out, r0.state_out)


def test_online_policy_replay(wl):
    """The host replay of streaming.OnlineViterbi: with room for every frame the emitted states are the best path of the whole
    audio, its score exactly (grid) and nothing is forced; with max_pending = 4 every frame is still emitted once and some are
    forced."""
    gs, V, lens = case_base(wl, rounded=True)
    whole = references(gs, V, lens, np.ones(6, dtype=np.int32))
    forced_any = 0
    for b in range(6):
        L = int(lens[b])
        chunks = [min(7, max(0, L - k)) for k in range(0, 42, 7)]
        em, score, nforced, total = vr.replay_online(gs[b], V[b], chunks, 40)
        states = np.concatenate(em)
        assert states.size == L and nforced == 0
        assert np.array_equal(states, whole[b].path[:L]) and (total == whole[b].score or (np.isneginf(total) and np.isneginf(whole[b].score))), b
        em, score, nforced, total = vr.replay_online(gs[b], V[b], chunks, 4)
        assert sum(e.size for e in em) == L
        forced_any += nforced > 0
    assert forced_any >= 1
