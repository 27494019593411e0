"""Segment posteriors (mm_segmentposteriors_f32) without a GPU: the bindings of the new entry, the argument checks that need no
device, and the float64 reference of tests/segment_reference.py -- the header's definition -- against brute-force enumeration,
against the window reference (a: end_in NULL), against the whole closed reference over chains of chunks (b), the shifts (c) and
(d), the independence of the start (f), and the len = 0, no-mass and dead-utterance conventions; the float32 mode of the reference
against the bars the kernels are held to; and a NumPy model of BatchedFSM.chunkedposteriors' bookkeeping against whole references."""
import ctypes as C
import os
import re

import numpy as np

import filter_reference as fr
import segment_reference as sr
import window_reference as wr
from test_filterposteriors import _graphs
from test_gpu_parity import check_gamma
from test_windowposteriors import case_den600, distinct_graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there.
    (The header's signature has 17 parameters: batch, V and its two strides, lens, N, state_in, end_mode, end_in, end_out, lend,
    gamma and its three strides, ttl, stream.)"""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_segmentposteriors_f32" in mm.SYMBOLS
    assert lib.mm_segmentposteriors_f32.argtypes is not None and len(lib.mm_segmentposteriors_f32.argtypes) == 17
    assert hasattr(mm.BatchedFSM, "segmentposteriors") and hasattr(mm.BatchedFSM, "chunkedposteriors") and callable(mm.chunkedposteriors)
    assert callable(mm.longform.chunked_loglik) and mm.chunked_loglik is mm.longform.chunked_loglik
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_segmentposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_segmentposteriors_f32, LIB\)", src) and re.search(r"function segmentposteriors\(", src)


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: gamma NULL (-1), g strides that cannot even hold the N frames
    (-2); with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(gamma=None, gs=(0, 0, 0), N=8):
        return lib.mm_segmentposteriors_f32(None, p, 8, 1, None, N, None, None, None, None, None, gamma, gs[0], gs[1], gs[2], None, None)

    assert call() == -1 and b"gamma is NULL" in lib.mm_last_error()
    assert call(gamma=p, gs=(64, 0, 1)) == -2 and b"g strides" in lib.mm_last_error()
    assert call(gamma=p, gs=(8, 1, 1)) == -1 and b"NULL batch" in lib.mm_last_error()


def _same(so, so_ref, tol):
    m = np.isfinite(so_ref)
    return bool((np.isneginf(so) == ~m).all() and (not m.any() or np.abs(so[m] - so_ref[m]).max() <= tol))


def _end_vector(rng, S1, holes=2):
    e = np.log(rng.random(S1))
    e[rng.choice(S1 - 1, size=holes, replace=False)] = -np.inf
    return e


def test_reference_against_path_enumeration(wl):
    """gamma, ttl, lend and end_out of all three end modes, with and without state_in, end_in with -inf entries."""
    rng = np.random.default_rng(61)
    for g, L in ((wl.l2r_hmm(3), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 4),
                 (wl.random_fsm(5, 3, mean_deg=2.0, seed=8), 1)):
        V = rng.standard_normal((6, g.P))
        for state_in in (None, np.log(rng.random(g.S + 1))):
            for mode, end_in in ((0, None), (1, None), (2, None), (2, _end_vector(rng, g.S + 1)), (1, _end_vector(rng, g.S + 1)), (0, _end_vector(rng, g.S + 1))):
                gam, ttl, lend, eo = sr.reference(g, V, L, 6, state_in, mode, end_in)
                g_e, t_e, l_e, eo_e = sr.enumerate_paths(g, V, L, state_in, mode, end_in)
                what = (g.name, L, state_in is None, mode, end_in is None)
                if not np.isfinite(t_e):  # (the end vector's holes may leave no path: the no-mass convention)
                    assert (gam == 0).all() and np.isneginf(ttl) and np.isneginf(lend) and np.isneginf(eo).all(), what
                    continue
                assert np.abs(gam[:L] - g_e).max() <= 1e-10 and (gam[L:] == 0).all(), what
                assert abs(ttl - t_e) <= 1e-10, what
                assert (np.isneginf(lend) and np.isneginf(l_e)) or abs(lend - l_e) <= 1e-10, what
                assert _same(eo, eo_e, 1e-10) and np.isneginf(eo[g.S]), what
                if np.isfinite(lend):
                    assert eo.max() == 0
                assert np.allclose(gam[:L].sum(-1), 1.0, atol=1e-12)


def test_without_an_end_vector_it_is_the_window(wl):
    """(a): end_in NULL -- gamma and ttl of the window reference with closed = end_mode, mode 2 included."""
    rng = np.random.default_rng(62)
    for g in _graphs(wl):
        N, L = 25, 21
        V = rng.standard_normal((N, g.P))
        for state_in in (None, np.log(rng.random(g.S + 1))):
            for mode in (0, 1, 2, 7):
                gam, ttl, _, _ = sr.reference(g, V, L, N, state_in, mode, None)
                g_w, t_w, _, _ = wr.reference(g, V, L, N, state_in, mode != 0)
                assert np.abs(gam - g_w).max() <= 1e-12 and abs(ttl - t_w) <= 1e-12 * max(1.0, abs(t_w)), (g.name, mode)


def test_chaining_is_exact(wl):
    """(b): chunks of 1, 4, 7, 21 (the length: it ends exactly on a boundary), 25 and 30 frames at N = 25, L = 21 against the whole
    closed reference, gamma and log Z to 1e-10; and two segments with any end: ttl_A + lend_B = the one call's ttl."""
    rng = np.random.default_rng(63)
    for g in (wl.l2r_hmm(3), wl.random_fsm(6, 3, mean_deg=2.0, seed=4), wl.random_fsm(40, 6, 3.0, seed=1)):
        N, L = 25, 21
        V = rng.standard_normal((N, g.P))
        whole = wr.reference(g, V, L, N, None, True)
        for chunk in (1, 4, 7, 21, 25, 30):
            gam, ttl, seen = sr.chained(g, V, L, N, chunk)
            assert seen <= max(chunk, 1) and (chunk >= N or seen <= chunk)
            assert np.abs(gam - whole[0]).max() <= 1e-10 and abs(ttl - whole[1]) <= 1e-10, (g.name, chunk, np.abs(gam - whole[0]).max())
        for L0 in (0, 1):
            gam, ttl, _ = sr.chained(g, V, L0, N, 4)
            w0 = wr.reference(g, V, L0, N, None, True)
            assert np.abs(gam - w0[0]).max() <= 1e-10 and ((np.isneginf(ttl) and np.isneginf(w0[1])) or abs(ttl - w0[1]) <= 1e-10), (g.name, L0)
        L1 = 9
        for mode, end_in in ((0, None), (1, None), (2, _end_vector(rng, g.S + 1, 1))):
            one = sr.reference(g, V, L, N, None, mode, end_in)
            state = fr.reference(g, V, L1, N)[3]
            gB, tB, lB, eB = sr.reference(g, V[L1:], L - L1, N - L1, state, mode, end_in)
            gA, tA, lA, eA = sr.reference(g, V, L1, L1, None, 2, eB)
            assert np.abs(gA - one[0][:L1]).max() <= 1e-10 and np.abs(gB - one[0][L1:]).max() <= 1e-10, (g.name, mode)
            assert abs(tA + lB - one[1]) <= 1e-10 and abs(lA + lB - one[2]) <= 1e-10 and _same(eA, one[3], 1e-10), (g.name, mode)


def test_shifts_and_the_start(wl):
    """(c) a constant per frame: gamma and end_out stay, ttl and lend move by the constants' sum; (d) a constant on end_in: ttl and
    lend move by it (b_0 is linear in b_len, and ttl_A + lend_B must stay the one call's ttl), nothing else; (f) end_out and lend do not depend on state_in."""
    rng = np.random.default_rng(64)
    for g in _graphs(wl):
        V = rng.standard_normal((20, g.P))
        k = rng.standard_normal(20) * 30
        e = _end_vector(rng, g.S + 1)
        for mode, end_in in ((0, None), (1, None), (2, e)):
            a, b = sr.reference(g, V, 17, 20, None, mode, end_in), sr.reference(g, V + k[:, None], 17, 20, None, mode, end_in)
            assert np.abs(a[0] - b[0]).max() <= 1e-12, g.name
            assert abs(b[1] - a[1] - k[:17].sum()) <= 1e-10 and abs(b[2] - a[2] - k[:17].sum()) <= 1e-10 and _same(b[3], a[3], 1e-11)
            c = sr.reference(g, V, 17, 20, np.log(rng.random(g.S + 1)), mode, end_in)
            assert (g.S < 10 or np.abs(c[0] - a[0]).max() > 1e-6) and abs(c[2] - a[2]) <= 1e-10 and _same(c[3], a[3], 1e-10), g.name
        a, d = sr.reference(g, V, 17, 20, None, 2, e), sr.reference(g, V, 17, 20, None, 2, e + 50.0)
        assert np.abs(a[0] - d[0]).max() <= 1e-12 and abs(d[1] - a[1] - 50.0) <= 1e-10 and abs(d[2] - a[2] - 50.0) <= 1e-10 and _same(d[3], a[3], 1e-11)


def test_empty_massless_and_dead_conventions(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    S = g.S
    rng = np.random.default_rng(65)
    V = rng.standard_normal((10, g.P))
    e = _end_vector(rng, S + 1)

    def dead(r):
        return (r[0] == 0).all() and np.isneginf(r[1]) and np.isneginf(r[2]) and np.isneginf(r[3]).all()

    # len = 0: the end vector the segment was given
    gam, ttl, lend, eo = sr.reference(g, V, 0, 10, None, 2, e)
    assert (gam == 0).all() and np.isneginf(ttl) and lend == 0 and np.array_equal(eo, e)
    gam, ttl, lend, eo = sr.reference(g, V, 0, 10, None, 0, e)
    assert np.isneginf(ttl) and lend == 0 and (eo[:S] == 0).all() and np.isneginf(eo[S])
    for mode, end_in in ((1, e), (2, None)):
        gam, ttl, lend, eo = sr.reference(g, V, 0, 10, None, mode, end_in)
        fw = np.full(S + 1, -np.inf)
        np.logaddexp.at(fw, g.final_idx, g.final_w)
        assert np.isneginf(ttl) and abs(lend - fw.max()) <= 1e-12 and _same(eo, fw - fw.max(), 1e-12) and eo.max() == 0
    import dataclasses

    nofinal = dataclasses.replace(g, final_idx=g.final_idx[:0], final_w=g.final_w[:0])
    assert dead(sr.reference(nofinal, V, 0, 10, None, 1, None))
    # no mass: the alive mass dies inside the segment; a start or an end vector without a live state; a zero total
    Vd = V.copy()
    Vd[4, :] = -np.inf
    for mode, end_in in ((0, None), (1, None), (2, e)):
        assert dead(sr.reference(g, Vd, 9, 10, None, mode, end_in))
        assert dead(sr.reference(g, V, 10, 10, np.full(S + 1, -np.inf), mode, end_in))
        assert np.isfinite(sr.reference(g, Vd, 4, 10, None, mode, end_in)[1])
    assert dead(sr.reference(g, V, 10, 10, None, 2, np.full(S + 1, -np.inf)))
    only_f = np.full(S + 1, -np.inf)
    only_f[S] = 0.0  # (the final state's entry is not read)
    assert dead(sr.reference(g, V, 10, 10, None, 2, only_f))
    h = wl.l2r_hmm(3)
    Vh = rng.standard_normal((2, h.P))
    assert dead(sr.reference(h, Vh, 2, 2, None, 1, None)) and np.isfinite(sr.reference(h, Vh, 2, 2, None, 0, None)[1])
    # a dead utterance propagates backwards through the chunks, and forwards by the filter's state: gamma = 0 everywhere
    gam, ttl, _ = sr.chained(g, Vd, 9, 10, 3)
    assert (gam == 0).all() and np.isneginf(ttl)
    for r in (sr.reference(g, Vd, 9, 10, None, 2, e), sr.chained(g, Vd, 9, 10, 3)):
        assert not any(np.isnan(np.asarray(x, dtype=np.float64)).any() for x in r)


# ---- the inputs of tests/test_gpu_segmentposteriors.py (module level: the float32 mode below runs on the very same inputs)
def case_random40(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N, B, S1 = 30, 6, g.S + 1
    lens = np.array([30, 25, 1, 0, 28, 30], dtype=np.int32)
    modes = np.array([0, 1, 2, 2, 1, 2], dtype=np.int32)
    rng = np.random.default_rng(0)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf  # a frame with -inf entries
    V[4, 14, :] = -np.inf  # utterance 4 dies mid-segment
    state = np.log(rng.random((B, S1))).astype(np.float32)
    has_state = [False, True, False, True, True, True]
    end = np.log(rng.random((B, S1))).astype(np.float32)
    end[1] = -np.inf  # (utterance 1 ends on the final weights: not read)
    end[2] = -np.inf  # an end vector without a live state: no mass
    end[3, [3, 17]] = -np.inf  # (no frame: handed back as given)
    end[5, [0, 8, 30]] = -np.inf
    return [g] * B, V, lens, modes, [state[b] if has_state[b] else None for b in range(B)], end


def case_random40_other_ends(wl):
    """... with the one-frame utterance 2 on a live end vector and the 30 frames of utterance 5 on one without a live state."""
    gs, V, lens, modes, states, end = case_random40(wl)
    end = end.copy()
    end[2] = np.log(np.random.default_rng(12).random(end.shape[1])).astype(np.float32)
    end[2, [3, 17]] = -np.inf
    end[5] = -np.inf
    return gs, V, lens, modes, states, end


def case_big(wl):
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    rng = np.random.default_rng(4)
    V = rng.standard_normal((2, 12, g.P)).astype(np.float32)
    end = np.log(rng.random((2, g.S + 1))).astype(np.float32)
    end[0, ::7] = -np.inf
    return [g, g], V, np.array([12, 7], dtype=np.int32), np.array([2, 0], dtype=np.int32), [None, np.log(rng.random(g.S + 1)).astype(np.float32)], end


def case_distinct(wl):
    gs = distinct_graphs(wl)
    rng = np.random.default_rng(5)
    V = rng.standard_normal((4, 40, 5)).astype(np.float32)
    ends = [np.log(rng.random(g.S + 1)).astype(np.float32) for g in gs]
    ends[3][5:60] = -np.inf
    states = [None, np.log(rng.random(gs[1].S + 1)).astype(np.float32), None, np.log(rng.random(gs[3].S + 1)).astype(np.float32)]
    return gs, V, np.array([40, 33, 20, 38], dtype=np.int32), np.array([2, 0, 1, 2], dtype=np.int32), states, ends


def case_many_pdfs(wl):
    g = wl.random_fsm(700, 600, 3.0, seed=9)
    rng = np.random.default_rng(10)
    V = rng.standard_normal((3, 14, g.P)).astype(np.float32)
    end = np.log(rng.random((3, g.S + 1))).astype(np.float32)
    return [g] * 3, V, np.array([14, 9, 2], dtype=np.int32), np.array([2, 1, 2], dtype=np.int32), [None, None, np.log(rng.random(g.S + 1)).astype(np.float32)], end


def case_den(wl):
    gs, V, lens, _, _ = case_den600(wl)
    rng = np.random.default_rng(11)
    g = gs[0]
    end = np.log(rng.random((4, g.S + 1))).astype(np.float32)
    end[2, 100:400] = -np.inf
    states = [None, np.log(rng.random(g.S + 1)).astype(np.float32), np.log(rng.random(g.S + 1)).astype(np.float32), None]
    return gs, V, lens, np.array([2, 1, 2, 0], dtype=np.int32), states, end


def references(case, dtype=np.float64):
    """The references of a case, one (gamma, ttl, lend, end_out) per utterance."""
    gs, V, lens, modes, states, end = case
    return [sr.reference(gs[b], V[b].astype(np.float64), int(lens[b]), V.shape[1], states[b], int(modes[b]), end[b] if end is not None else None, dtype)
            for b in range(len(gs))]


def check_against_reference(gamma, ttl, lend, eo, ref, L):
    """One utterance against its float64 reference under the project's bars -- gamma: check_gamma of tests/test_gpu_parity.py; ttl
    and lend: np.isclose(rtol=1e-5, atol=1e-4); end_out: the state_out bar of test_windowposteriors.check_against_reference, -inf
    exactly where the reference has -inf -- and a segment without mass or without a frame by its exact conventions.  Returns the
    worst error over its bar of (gamma, ttl / lend, end_out)."""
    g_ref, t_ref, l_ref, e_ref = ref
    gamma, eo = np.asarray(gamma, dtype=np.float64), np.asarray(eo, dtype=np.float64)
    assert not (np.isnan(gamma).any() or np.isnan(eo).any() or np.isnan(ttl) or np.isnan(lend))
    assert (gamma[L:] == 0).all()
    wg = wt = ws = 0.0
    if np.isfinite(t_ref):
        wg = check_gamma(gamma[None], g_ref[None], [L])
        assert np.isclose(ttl, t_ref, rtol=1e-5, atol=1e-4), (ttl, t_ref)
        wt = abs(ttl - t_ref) / (1e-4 + 1e-5 * abs(t_ref))
    else:
        assert (gamma == 0).all() and np.isneginf(ttl), ttl
    if np.isfinite(l_ref):
        assert np.isclose(lend, l_ref, rtol=1e-5, atol=1e-4), (lend, l_ref)
        wt = max(wt, abs(lend - l_ref) / (1e-4 + 1e-5 * abs(l_ref)))
    else:
        assert np.isneginf(lend), lend
    assert (np.isneginf(eo) == np.isneginf(e_ref)).all()
    m = e_ref > np.log(1e-30)
    if m.any():
        e = np.abs(eo[m] - e_ref[m]) / (1e-4 * np.maximum(np.abs(e_ref[m]), 1.0))
        assert (e <= 1.0).all(), e.max()
        ws = float(e.max())
    return wg, wt, ws


CHUNK_LENS = np.array([150, 120, 150, 33], dtype=np.int32)


def test_float32_mode_within_the_bars(wl):
    """The recursions carried in float32 against float64 on the GPU tests' inputs, the chained ones included: below half of every
    bar the kernels are held to (were it more on an input, the input would have to change, not the bar)."""
    worst = np.zeros(3)
    for case in (case_random40(wl), case_random40_other_ends(wl), case_distinct(wl), case_many_pdfs(wl), case_den(wl)):
        lens = case[2]
        for b, (r64, r32) in enumerate(zip(references(case), references(case, dtype=np.float32))):
            worst = np.maximum(worst, check_against_reference(r32[0], r32[1], r32[2], r32[3], r64, int(lens[b])))
    gs, V, _, _, _ = case_den600(wl)
    N = V.shape[1]
    for b in range(len(gs)):
        L = int(CHUNK_LENS[b])
        whole = wr.reference(gs[b], V[b].astype(np.float64), L, N, None, True)
        for chunk in (37, 40):
            gam, ttl, _ = sr.chained(gs[b], V[b], L, N, chunk, np.float32)
            worst[0] = max(worst[0], check_gamma(gam[None], whole[0][None], [L]))
            assert np.isclose(ttl, whole[1], rtol=1e-5, atol=1e-4)
            worst[1] = max(worst[1], abs(ttl - whole[1]) / (1e-4 + 1e-5 * abs(whole[1])))
    print(f"float32 recursions: worst error over its bar: gamma {worst[0]:.3g}, ttl / lend {worst[1]:.3g}, end_out {worst[2]:.3g}")
    assert (worst <= 0.5).all()


def test_driver_bookkeeping(wl):
    """The NumPy model of BatchedFSM.chunkedposteriors (segment_reference.chained) against whole closed references: varying lengths,
    one ending exactly on a chunk boundary, one wholly inside chunk 0, an empty one; no call sees more than `chunk` frames."""
    rng = np.random.default_rng(66)
    for g in (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), wl.random_fsm(40, 6, 3.0, seed=1)):
        N = 40
        V = rng.standard_normal((N, g.P))
        for chunk in (8, 13, 40, 64):
            for L in (40, 32, 24, 5, 1, 0):
                whole = wr.reference(g, V, L, N, None, True)
                gam, ttl, seen = sr.chained(g, V, L, N, chunk)
                assert seen <= chunk or chunk >= N
                assert np.abs(gam - whole[0]).max() <= 1e-10, (g.name, chunk, L)
                assert (np.isneginf(ttl) and np.isneginf(whole[1])) or abs(ttl - whole[1]) <= 1e-9, (g.name, chunk, L, ttl, whole[1])
