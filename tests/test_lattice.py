"""Beam-pruned best-path lattices (mm_lattice_f32) without a GPU: the bindings of the new entry, the argument checks that need no
device, the NumPy restatement of tests/lattice_reference.py -- the header's definition -- against brute-force enumeration of every
complete path of hand-built graphs (parallel entries, ties, a dead end, an utterance without a path), the consequences (a) .. (d)
the header states on the restatement, and decode.lattice_arcs / decode.lattice_fsm on a restated lattice.  The cases of
tests/test_gpu_lattice.py are built here, with their input conditions asserted from the restatement alone."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import classpath_reference as cr
import lattice_reference as lr
from test_classpath import case_classes
from test_viterbiwindow import on_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
ARC_COUNTS = (1, 63, 65, 255, 257, 1025)  # the wave, block and iteration edges of the compaction (64 lanes, 256 threads, 4 each)


# ---- the cases the GPU tests run
def grid(x):
    return (np.round(np.asarray(x, dtype=np.float64) * 16) / 16).astype(np.float32)


def emissions(seed, B, N, P, rounded=True, scale=2.0):
    V = scale * np.random.default_rng(seed).standard_normal((B, N, P))
    return grid(V) if rounded else V.astype(np.float32)


def fsm_with_entries(mm, n):
    """A tropical FSM over 5 real states and 3 pdfs with exactly n stored entries, weights on the 1/16 grid: the arcs of a small
    ergodic graph repeated as parallel entries (every third repeat an exact duplicate of its entry's weight: ties between
    parallels) until n - 1 entries stand, then the phony self-loop.  n = 1: the single arc 0 -> f, no self-loop (runs with len = N
    only).  Returns (FSM, GraphSpec-like with state2pdf and P)."""
    S = 5
    g = SimpleNamespace(state2pdf=np.array([0, 1, 2, 0, 1], dtype=np.int32), P=3)
    if n == 1:
        f = mm.FSM.from_fields([0], [0.0], [0, 0, 0, 0, 0, 0, 1], [0], np.array([-0.5], dtype=np.float32), list(range(S)), semiring="tropical")
        return f, g
    pairs = [(s, d) for s in range(S) for d in ((s + 1) % S, s, (s + 2) % S)] + [(4, S), (2, S)]
    ents = []
    for k in range(n - 1):
        s, d = pairs[k % len(pairs)]
        rep = k // len(pairs)
        ents.append((s, d, -0.25 - ((3 * k) % 11) / 16.0 if rep % 3 else -0.25 - ((3 * (k % len(pairs))) % 11) / 16.0))
    ents.append((S, S, 0.0))
    ents.sort(key=lambda e: e[1])  # (stable: CSC order, the parallels of a pair in their order)
    colptr = np.zeros(S + 2, dtype=np.int64)
    for _, d, _ in ents:
        colptr[d + 1] += 1
    f = mm.FSM.from_fields([0, 3], [0.0, -0.5], np.cumsum(colptr), [e[0] for e in ents], np.array([e[2] for e in ents], dtype=np.float32),
                           list(range(S)), semiring="tropical")
    return f, g


def entries_case(mm, n):
    """(f, g, V [B, N, P], lens) of fsm_with_entries(n): B = 3, N = 6 with a short utterance (n = 1: B = 2, N = 1, full lengths)."""
    f, g = fsm_with_entries(mm, n)
    if n == 1:
        return f, g, emissions(n, 2, 1, g.P), np.array([1, 1], dtype=np.int32)
    return f, g, emissions(n, 3, 6, g.P), np.array([6, 4, 6], dtype=np.int32)


def chain_graph(wl, S):
    """A chain of S states: a loop on and a step from every state, every fourth state final, initial states at both ends of the index
    range (S - 40 starts paths through states beyond 16 bits once S > 65 576), weights on the 1/16 grid, 4 pdfs."""
    s = np.arange(S)
    src = np.concatenate([s, s[:-1]])
    dst = np.concatenate([s, s[1:]])
    w = np.concatenate([-(s % 5) / 16.0 - 0.125, -((3 * s[:-1]) % 7) / 16.0 - 0.0625])
    fin = s[::4]
    return wl.GraphSpec(f"chain{S}", S, np.array([0, S - 40]), np.array([-0.25, 0.0]), src, dst, w, fin, -(fin % 3) / 16.0, (s % 4).astype(np.int32), 4)


def scan_cases():
    """(B, N, lens) with B * N = 1, 255, 256, 257 and 3 x 700 (several chunks of the scan), lens mixed among 0, 1, < N and N."""
    return [(1, 1, [1]), (5, 51, [51, 0, 1, 30, 51]), (4, 64, [64, 1, 0, 63]), (1, 257, [257]), (3, 700, [700, 1, 333])]


def distinct_case(mm, wl):
    """Four different graphs with state and arc offsets; utterance 1 has no path (its frame 2 emits nothing) between two that have."""
    gs = [on_grid(wl.random_fsm(60, 5, 3.0, seed=2, n_init=4)), on_grid(wl.l2r_hmm(5)), on_grid(wl.random_fsm(25, 5, 2.0, seed=7)),
          on_grid(wl.lfmmi_denominator(300, 5, seed=1))]
    B, N = 4, 30
    lens = np.array([30, 22, 30, 17], dtype=np.int32)
    V = emissions(21, B, N, 5)
    V[1, 2, :] = -np.inf
    return gs, [wl.to_fsm(mm, g, semiring="tropical") for g in gs], V, lens


def unrounded_cases(mm, wl):
    """The two graphs of the unrounded case with standard-normal V: (g, f, V, lens)."""
    out = []
    for g, B, N, lens in ((wl.random_fsm(30, 5, 3.0, seed=9), 3, 25, [25, 18, 25]), (wl.lexicon_fsm(80, seed=2), 2, 40, [40, 31])):
        out.append((g, wl.to_fsm(mm, g, semiring="tropical"), emissions(5, B, N, g.P, rounded=False, scale=1.0), np.array(lens, dtype=np.int32)))
    return out


def to_oracle_fsm(o, f):
    """A product FSM (tropical) as the oracle's, through its arc-list constructor."""
    i, j, w = ar.fsm_entries(f)
    S = f.colptr.size - 2
    real = j < S
    fin = (j == S) & (i < S)
    return o.make_fsm(o.SEMIRINGS["tropical"], list(zip((int(s) for s in f.alpha_idx), (float(v) for v in f.alpha_val))),
                      [((int(a), int(b)), float(v)) for a, b, v in zip(i[real], j[real], w[real])],
                      [(int(a), float(v)) for a, v in zip(i[fin], w[fin])], list(range(S)), np.float64)


def as_lattice(mm, br):
    return mm.Lattice(br.counts, br.offsets, br.arc, br.score, br.best)


def stub_batch(mm, fs, gs):
    """What decode.lattice_arcs / lattice_fsm read of a batch, without a device."""
    return SimpleNamespace(cfsms=[SimpleNamespace(fsm=f, S1=f.S1, C_hat=mm.statemap(g.state2pdf, g.P)) for f, g in zip(fs, gs)])


# ---- the tests
def test_entry_is_bound(mm):
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_lattice_f32" in mm.SYMBOLS and len(lib.mm_lattice_f32.argtypes) == 15
    assert callable(mm.lattice) and hasattr(mm.BatchedFSM, "lattice") and mm.Lattice._fields == ("counts", "offsets", "arc", "score", "best")
    assert callable(mm.decode.lattice_arcs) and callable(mm.decode.lattice_fsm) and mm.lattice_fsm is mm.decode.lattice_fsm
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_lattice_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_lattice_f32, LIB\)", src) and "function lattice(" in src


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: beam, counts or total NULL (-1), counts_stride_b < N (-2), arc
    without score or score without arc (-1), a negative cap and a cap without arc (-1); with those in order the NULL batch is what
    is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(beam=p, counts=p, csb=8, total=p, arc=None, score=None, cap=0, N=8):
        return lib.mm_lattice_f32(None, p, 8, 1, None, N, beam, counts, csb, total, None, arc, score, cap, None)

    for kw in ({"beam": None}, {"counts": None}, {"total": None}):
        assert call(**kw) == -1 and b"is NULL" in lib.mm_last_error(), kw
    assert call(csb=7) == -2 and b"counts_stride_b" in lib.mm_last_error()
    assert call(arc=p, cap=4) == -1 and b"both" in lib.mm_last_error()
    assert call(score=p) == -1 and b"both" in lib.mm_last_error()
    assert call(arc=p, score=p, cap=-1) == -1 and b"cap" in lib.mm_last_error()
    assert call(cap=3) == -1 and b"cap" in lib.mm_last_error()
    assert call() == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(arc=p, score=p, cap=4) == -1 and b"NULL batch" in lib.mm_last_error()


def test_binding_argument_helpers(mm):
    """beam as a number, a [B] array, a wrong shape; max_arcs negative."""
    import torch
    from importlib import import_module

    inf = import_module(mm.__name__ + ".inference")
    dev = torch.device("cpu")
    assert inf._beam_vector(2.5, 3, dev).tolist() == [2.5] * 3 and inf._beam_vector(np.float32(1), 2, dev).dtype == torch.float32
    assert inf._beam_vector([1, 2, INF], 3, dev).tolist() == [1.0, 2.0, INF]
    assert inf._beam_vector(torch.tensor([0.5, 1.5], dtype=torch.float64), 2, dev).tolist() == [0.5, 1.5]
    with pytest.raises(mm.DimensionMismatch):
        inf._beam_vector([1, 2], 3, dev)
    assert inf._record_cap(None) is None and inf._record_cap(7) == 7
    with pytest.raises(ValueError):
        inf._record_cap(-1)


def hand_graphs(mm):
    """(name, FSM, s2p, P, V [N, P], L, N): graphs of at most 4 real states and 5 frames.
    parallel: 0 -> 1 twice with equal weights and once worse, 1 -> 2 twice with different weights.
    ties: two state sequences of equal weight.  dead end: state 3 is entered and never left.  no path: frame 2 emits nothing.
    short: len 2 of N 4 (the phony self-loop carries best to frame N + 1), len 0."""
    z = lambda *rows: np.array(rows, dtype=np.float32)
    #        col 0   col 1                   col 2                 col 3 (f)
    rows = [0,      0, 0, 0, 1,             1, 1, 2,              2, 1, 3]
    vals = [-1.0,   -0.5, -0.5, -0.75, -1., -0.25, -0.5, -1.0,    0.0, -2.0, 0.0]
    par = mm.FSM.from_fields([0], [0.0], [0, 1, 5, 8, 11], rows, np.asarray(vals, dtype=np.float32), list("abc"), semiring="tropical")
    arcs = [((0, 1), -0.5), ((0, 2), -0.5), ((1, 3), -0.25), ((2, 3), -0.25), ((1, 1), -1.0), ((3, 3), -0.5), ((0, 0), -0.125)]
    tie = mm.FSM([(0, 0.0)], arcs, [(3, 0.0), (1, -3.0)], list("abcd"), semiring="tropical")
    dead = mm.FSM([(0, 0.0), (1, -0.5), (2, -1.0)], [((0, 1), -0.5), ((1, 2), -0.25), ((1, 3), 0.0), ((0, 0), -0.5), ((2, 2), -0.5), ((3, 3), 0.0)],
                  [(2, -0.25)], list("abcd"), semiring="tropical")
    V3 = z([0, -1, -2], [-0.5, 0.125, -1], [-2, 0.25, 0], [-1, -0.5, 0.5], [-0.25, -1, 0.25])
    V4 = z([0, 0, 0, 0], [-0.5, 0.25, 0.25, -1], [-1, 0.5, -0.5, 0.25], [0, -0.25, -0.25, 0.5], [0.25, -1, 0, 0.125])
    Vn = V4.copy()
    Vn[2] = -np.inf
    return [("parallel", par, np.arange(3), 3, V3, 5, 5), ("parallel, len 3", par, np.arange(3), 3, V3, 3, 5), ("ties", tie, np.arange(4), 4, V4, 4, 4),
            ("ties, len 5", tie, np.arange(4), 4, V4, 5, 5), ("dead end", dead, np.arange(4), 4, V4, 4, 5), ("no path", dead, np.arange(4), 4, Vn, 4, 4),
            ("len 0", tie, np.arange(4), 4, V4, 0, 4), ("len 1", dead, np.arange(4), 4, V4, 1, 3)]


@pytest.mark.parametrize("beam", [0.0, 0.5, 1.0, 3.0, INF, -1.0, float("nan")])
def test_restatement_against_brute_force(mm, beam):
    seen_parallel_tie = seen_tie = seen_empty = False
    for name, f, s2p, P, V, L, N in hand_graphs(mm):
        kept, best = lr.brute_force(f, s2p, P, V, L, N, beam)
        for dt in (np.float32, np.float64):
            r = lr.reference(f, s2p, P, V, L, N, beam, dt)
            assert float(r.best) == best, (name, r.best, best)
            got = {(int(t), int(k)): float(s) for t, k, s in zip(r.t, r.arc, r.score)}
            assert got == kept, (name, beam, dt, got, kept)
            assert r.counts.sum() == len(kept) and (r.counts[L:] == 0).all() and not np.isnan(r.score).any()
            assert all(np.array_equal(r.arc[r.t == t], np.sort(r.arc[r.t == t])) for t in range(N))
        if name == "no path" or L == 0:
            assert best == -np.inf and not kept
            seen_empty = True
        if beam == 0.0 and name == "parallel":
            # (both of the tied parallels 0 -> 1, entries 1 and 2, and not the worse one, entry 3)
            seen_parallel_tie = any((t, 1) in kept and (t, 2) in kept and (t, 3) not in kept for t in range(L))
        if beam == 0.0 and name == "ties":
            i, j, _ = ar.fsm_entries(f)
            seen_tie = any(len({(int(i[k]), int(j[k])) for (tt, k) in kept if tt == t}) >= 2 for t in range(L))  # (two state sequences)
        if not (beam >= 0):
            assert not kept
    assert seen_empty and (beam != 0.0 or (seen_parallel_tie and seen_tie))


def test_consequences_on_the_restatement(mm, wl):
    """(a) the arcs the best path of classpath_reference takes are kept at any beam >= 0 with score 0; (b) beam 0 keeps arcs of
    score 0 only, at least one per transition, and all of them lie on a path of the best weight; (c) nested in the beam; (d) the
    maximum of the kept scores into (j, frame t + 2) is mu wherever mu >= -beam -- all exact on the 1/16 grid, in float32."""
    g, f, twin, V, lens = case_classes(mm, wl, rounded=True)
    N = V.shape[1]
    sy = lr.system(f)
    for b in range(V.shape[0]):
        L = int(lens[b])
        path = cr.reference(f, g.state2pdf, g.P, None, 0, None, V[b], L, N)
        prev = None
        for beam in (0.0, 2.0, 8.0, INF):
            r = lr.reference(f, g.state2pdf, g.P, V[b], L, N, beam, np.float32, sy)
            r64 = lr.reference(f, g.state2pdf, g.P, V[b], L, N, beam, np.float64, sy)
            assert np.array_equal(r.arc, r64.arc) and np.array_equal(r.score.astype(np.float64), r64.score) and float(r.best) == float(r64.best)
            recs = set(zip(r.t.tolist(), r.arc.tolist()))
            if np.isfinite(path.score):
                assert np.float32(path.score) == r.best
                for t in range(L):  # (a)
                    assert (t, int(path.entries[t])) in recs and r.s[t, int(path.entries[t])] == 0
                assert (r.counts[:L] >= 1).all()
            else:
                assert r.counts.sum() == 0 and np.isneginf(r.best)
            if beam == 0.0:  # (b)
                assert (r.score == 0).all()
            if prev is not None:  # (c)
                assert prev <= recs
            prev = recs
            for t in range(L):  # (d)
                m = np.full(sy.S1, -np.inf, dtype=np.float32)
                sel = r.t == t
                np.maximum.at(m, sy.j[r.arc[sel]], r.score[sel])
                want = r.mu[t + 1] >= -np.float32(beam)
                assert np.array_equal(m[want], r.mu[t + 1][want]) and np.isneginf(m[~want]).all(), (b, beam, t)


def test_lattice_fsm_of_a_restated_lattice(mm, wl, oracle):
    """decode.lattice_arcs returns the records of an utterance with their ends; the oracle's viterbi on decode.lattice_fsm's graph
    and map, over the same V, gives the original best score -- at a beam of 0 and of 2; an utterance without a path has no graph."""
    oracle = oracle[0]  # (the Python oracle)
    g, f, twin, V, lens = case_classes(mm, wl, rounded=True)
    B, N = V.shape[0], V.shape[1]
    i, j, w = ar.fsm_entries(f)
    bf = stub_batch(mm, [f] * B, [g] * B)
    for beam in (0.0, 2.0):
        br = lr.batch_reference([f] * B, [g] * B, V, lens, beam)
        lat = as_lattice(mm, br)
        for b in range(B):
            t, k, src, dst, s = mm.decode.lattice_arcs(bf, lat, b)
            r = br.refs[b]
            assert np.array_equal(t, r.t) and np.array_equal(k, r.arc) and np.array_equal(src, i[r.arc]) and np.array_equal(dst, j[r.arc])
            assert np.array_equal(s, r.score)
            if not np.isfinite(r.best):
                with pytest.raises(ValueError):
                    mm.decode.lattice_fsm(bf, lat, b)
                continue
            lf, s2p = mm.decode.lattice_fsm(bf, lat, b)
            L = int(lens[b])
            assert lf.semiring == "tropical" and len(s2p) == lf.S1 - 1 and all(0 <= n < L for n, _ in lf.labels)
            _, score, _, _ = oracle.viterbi(to_oracle_fsm(oracle, lf), s2p, g.P, V[b, :L].T.astype(np.float64), L)
            assert score == float(r.best), (b, beam, score, r.best)
    cut = mm.Lattice(br.counts, br.offsets, br.arc[:5], br.score[:5], br.best)
    with pytest.raises(ValueError):
        mm.decode.lattice_arcs(bf, cut, 0)


def test_gpu_case_conditions(mm, wl):
    """What the GPU tests rely on, from the reference alone: the entry counts, full ballots at beam inf, duplicates reported at
    beam 0, arcs exactly on the threshold, float32 = float64 on the rounded inputs, paths through states beyond 16 bits, the rows of
    the chains beyond the LDS, and the unrounded case's excused arcs within 1 % of the kept ones."""
    for n in ARC_COUNTS:
        f, g, V, lens = entries_case(mm, n)
        assert f.nnz == n
        i, j, w = ar.fsm_entries(f)
        full = lr.batch_reference([f] * len(lens), [g] * len(lens), V, lens, INF)
        zero = lr.batch_reference([f] * len(lens), [g] * len(lens), V, lens, 0.0)
        assert np.isfinite(full.best).all() and (zero.counts.sum(axis=1) >= lens).all()
        if n >= 63:
            assert full.counts.max() >= n // 2  # (most of the plane survives: whole waves of kept entries)
            dup = [np.unique(np.stack([i[r.arc], j[r.arc], r.t]), axis=1).shape[1] < r.arc.size for r in zero.refs]
            assert any(dup)  # (beam 0 reports both of two tied parallel entries)
    g, f, twin, V, lens = case_classes(mm, wl, rounded=True)
    B, N = V.shape[0], V.shape[1]
    on_threshold = 0
    for beam in (0.0, 2.0, 8.0):
        r32 = lr.batch_reference([f] * B, [g] * B, V, lens, beam, np.float32)
        r64 = lr.batch_reference([f] * B, [g] * B, V, lens, beam, np.float64)
        assert np.array_equal(r32.arc, r64.arc) and np.array_equal(r32.score.astype(np.float64), r64.score)
        on_threshold += int((r32.score == -np.float32(beam)).sum()) if beam > 0 else 0
    assert on_threshold >= 100  # (49 at beam 2, 119 at beam 8: the >= of the rule is exercised)
    for S in (45000, 70000):
        gch = chain_graph(wl, S)
        fch = wl.to_fsm(mm, gch, semiring="tropical")
        assert 2 * (S + 4) * 4 > 160 * 1024
        Vc = emissions(3, 2, 3, 4)
        r = lr.batch_reference([fch] * 2, [gch] * 2, Vc, np.array([3, 2]), 1.0)
        ic, jc, _ = ar.fsm_entries(fch)
        assert np.isfinite(r.best).all() and r.counts[0].min() >= 2
        assert (ic[r.arc] > S - 50).any() and (ic[r.arc] < 10).any()
        if S == 70000:
            assert (ic[r.arc] > 65535).any() and r.arc.max() > 2 * 65536
    for g, f, V, lens in unrounded_cases(mm, wl):
        for beam in (2.0, 8.0):
            for b in range(V.shape[0]):
                r64 = lr.reference(f, g.state2pdf, g.P, V[b], int(lens[b]), V.shape[1], beam, np.float64)
                tol = lr.tau(V.shape[1], r64.alpha)
                fin = r64.s[np.isfinite(r64.s)]
                near = int((np.abs(fin + beam) <= tol).sum())
                assert r64.arc.size > 0 and near <= 0.01 * r64.arc.size, (g.name, beam, b, near, r64.arc.size)
