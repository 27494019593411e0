"""Lattice best paths (mm_latticebest_f32) without a GPU: the bindings of the new entry, the argument checks that need no device,
the float32 restatement of tests/latbest_reference.py -- the header's definition -- against brute-force enumeration of every lattice
path of hand-built graphs (exact on the 1/16 grid, ties between parallel entries included; within the rounding of the adds on
unrounded inputs), against lattice_reference for consequence (b), on doctored records; decode.lattice_rescore and
decode.lattice_onebest on host arrays.  The cases of tests/test_gpu_latticebest.py are built here."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import latbest_reference as lb
import latpost_reference as lp
import lattice_reference as lr
from test_lattice import INF, as_lattice, emissions, grid, hand_graphs, stub_batch
from test_latticeposteriors import record_scores, small_graphs
from test_viterbiwindow import on_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restated_batch(mm, fs, gs):
    """stub_batch with a latticebest that is the restatement: what decode.lattice_rescore / lattice_onebest need of a batch."""
    bf = stub_batch(mm, fs, gs)

    def latticebest(lat, V, lens=None, extra=None, want_path=True):
        ref = lb.reference(fs, gs, V, lens, lat.offsets, lat.arc, extra)
        return mm.LatticeBest(ref.best, ref.score, ref.rec if want_path else None, ref.path if want_path else None)

    bf.latticebest = latticebest
    return bf


def unique_best_seed(mm, wl, g, f, B, N, lens, seeds=range(40)):
    """The first seed whose grid emissions give a beam-0 reference lattice of ONE record per cell for every utterance with a path,
    and at least one such utterance: (seed, V)."""
    for seed in seeds:
        V = emissions(seed, B, N, g.P)
        br = lr.batch_reference([f] * B, [g] * B, V, lens, 0.0)
        L = np.full(B, N) if lens is None else np.asarray(lens)
        want = (np.arange(N)[None] < L[:, None]) & np.isfinite(br.best)[:, None]
        if np.isfinite(br.best).any() and np.array_equal(br.counts, want.astype(np.int32)):
            return seed, V
    raise AssertionError("no seed with a unique best path")


# ---- the tests
def test_entry_is_bound(mm):
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_latticebest_f32" in mm.SYMBOLS and len(lib.mm_latticebest_f32.argtypes) == 17
    assert callable(mm.latticebest) and hasattr(mm.BatchedFSM, "latticebest")
    assert mm.LatticeBest._fields == ("best", "score", "rec", "path")
    assert mm.lattice_rescore is mm.decode.lattice_rescore and mm.lattice_onebest is mm.decode.lattice_onebest
    assert callable(mm.lattices.lattice_best_score) and mm.lattice_best_score is mm.lattices.lattice_best_score
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_latticebest_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr and "21 = mm_latticebest_f32" in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_latticebest_f32, LIB\)", src) and "function latticebest(" in src


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: offsets or best NULL (-1), a negative nrec (-1), arc or score NULL
    with records to read (-1), rec or path strides below N (-2); with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))

    def call(offsets=p, arc=p, nrec=4, extra=None, best=fp, score=fp, rec=None, rsb=0, path=None, psb=0, N=8):
        return lib.mm_latticebest_f32(None, fp, 8, 1, None, N, offsets, arc, nrec, extra, best, score, rec, rsb, path, psb, None)

    for kw in ({"offsets": None}, {"best": None}, {"arc": None}, {"score": None}):
        assert call(**kw) == -1 and b"is NULL" in lib.mm_last_error(), kw
    assert call(nrec=-1) == -1 and b"nrec" in lib.mm_last_error()
    assert call(rec=p, rsb=7) == -2 and b"rec_stride_b" in lib.mm_last_error()
    assert call(path=p, psb=7, rec=p, rsb=8) == -2 and b"path_stride_b" in lib.mm_last_error()
    assert call() == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(arc=None, score=None, nrec=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (an empty lattice needs neither)
    assert call(rec=p, rsb=8, path=p, psb=9, extra=fp) == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(rsb=0, psb=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (strides of outputs not asked for are not looked at)


def _lattices_of(f, g, V, L, N, beams=(INF, 1.0)):
    for beam in beams:
        r = lr.reference(f, g.state2pdf, g.P, V, L, N, beam)
        yield beam, np.concatenate([[0], np.cumsum(r.counts, dtype=np.int64)]), r.arc


def _against_brute_force(name, f, g, Vn, L, N, offsets, arc, extra, exact):
    ref = lb.reference([f], [g], Vn[None, :N], [L], offsets, arc, extra)
    cl = lp.cells(offsets, arc.size, 0, N)
    through, best, rec = lb.brute_force(f, g.state2pdf, g.P, Vn, L, N, cl, arc, extra)
    what = (name, extra is not None)
    assert ref.best.dtype == np.float32 and ref.score.dtype == np.float32 and not np.isnan(ref.score).any(), what
    assert np.isneginf(best) == np.isneginf(ref.best[0]), what
    want = np.array([through.get(r, -np.inf) - best if best > -np.inf else -np.inf for r in range(arc.size)])
    assert np.array_equal(np.isneginf(want), np.isneginf(ref.score)), what
    fin = ~np.isneginf(want)
    if exact:
        assert np.isneginf(best) or float(ref.best[0]) == best, what
        assert np.array_equal(ref.score[fin].astype(np.float64), want[fin]), what
        assert ref.rec[0, :L].tolist() == (rec if rec else [-1] * L) and (ref.rec[0, L:] == -1).all(), (what, ref.rec[0], rec)
    else:
        tol = (L + 2) * 2.0 ** -24 * ref.amax[0]
        assert np.isneginf(best) or abs(float(ref.best[0]) - best) <= tol, (what, float(ref.best[0]), best, tol)
        # (a score is a difference of two such sums)
        assert (np.abs(ref.score[fin].astype(np.float64) - want[fin]) <= 2 * tol).all(), (what, tol)
    i = lr.system(f).i
    on = ref.rec[0] >= 0
    assert np.array_equal(ref.path[0][on], i[arc[ref.rec[0][on]]]) and (ref.path[0][~on] == -1).all(), what
    return ref, through, best, rec


def test_restatement_against_brute_force_on_the_grid(mm):
    """Every hand graph of test_lattice (parallel entries with ties, two state sequences, a dead end, no path, len 0 and 1), the
    lattices of beam inf and 1 under the lattice's V, ANOTHER V, and V with -inf entries, extra NULL and given, all on the 1/16
    grid: best, score and rec of the float32 restatement are the enumeration's EXACTLY -- the tie rule between parallel entries and
    between state sequences included."""
    seen_parallel_tie = seen_sequence_tie = seen_no_path = seen_dead = False
    for name, f, s2p, P, V, L, N in hand_graphs(mm):
        g = SimpleNamespace(state2pdf=s2p, P=P)
        sy = lr.system(f)
        for beam, offsets, arc in _lattices_of(f, g, V, L, N):
            V2 = grid(V + 0.5 * np.random.default_rng(len(name)).standard_normal(V.shape))
            V3 = V2.copy()
            if N > 2:
                V3[1, 0] = -np.inf
            V4 = V2.copy()
            V4[min(1, N - 1)] = -np.inf
            for Vn in (V, V2, V3, V4):
                for extra in (None, grid(record_scores(7, arc.size))):
                    ref, through, best, rec = _against_brute_force((name, beam), f, g, Vn, L, N, offsets, arc, extra, exact=True)
                    seen_no_path |= arc.size > 0 and np.isneginf(best)
                    seen_dead |= best > -np.inf and len(through) < arc.size
                    for t, r in enumerate(rec):
                        lo, hi = int(offsets[t]), int(offsets[t + 1])
                        tied = [x for x in range(lo, hi) if x != r and ref.score[x] == 0 and sy.j[arc[x]] == sy.j[arc[r]]]
                        seen_parallel_tie |= any(sy.i[arc[x]] == sy.i[arc[r]] for x in tied)
                        seen_sequence_tie |= any(sy.i[arc[x]] != sy.i[arc[r]] for x in tied)
                        assert all(x > r for x in tied if sy.i[arc[x]] == sy.i[arc[r]])  # (of tied parallels the lowest record)
    assert seen_parallel_tie and seen_sequence_tie and seen_no_path and seen_dead


def test_restatement_against_brute_force_on_unrounded_inputs(mm):
    """The same graphs with standard-normal perturbations of V and extra off the grid: best within (len + 2) 2^-24 max|a| of the
    float64 enumeration -- the rounding of the len + 1 float32 adds along a path, max|a| the largest forward value -- and the
    scores, differences of two such sums, within twice that."""
    for name, f, s2p, P, V, L, N in hand_graphs(mm):
        g = SimpleNamespace(state2pdf=s2p, P=P)
        for beam, offsets, arc in _lattices_of(f, g, V, L, N):
            rng = np.random.default_rng(len(name) + 1)
            Vn = (V + rng.standard_normal(V.shape)).astype(np.float32)
            for extra in (None, record_scores(9, arc.size)):
                _against_brute_force((name, beam), f, g, Vn, L, N, offsets, arc, extra, exact=False)


def test_consequence_b_against_the_lattice_reference(mm, wl):
    """(b) extra NULL, the lattice's own V, inputs on the 1/16 grid: best and score are the lattice's, bit for bit, at every beam;
    (c) the score of every record of the path is 0 and every cell's maximum is 0."""
    for g, f in small_graphs(mm, wl):
        gx = on_grid(g)
        fx = wl.to_fsm(mm, gx, semiring="tropical")
        B, N = 3, 6
        for lens in (np.array([6, 1, 0], dtype=np.int32), None):
            V = emissions(4, B, N, g.P)
            for beam in (0.0, 2.0, INF):
                br = lr.batch_reference([fx] * B, [gx] * B, V, lens, beam)
                ref = lb.reference([fx] * B, [gx] * B, V, lens, br.offsets, br.arc)
                assert bits(ref.best, br.best.astype(np.float32)) and bits(ref.score, br.score.astype(np.float32)), (g.name, beam)
                for b in range(B):
                    L = N if lens is None else int(lens[b])
                    if np.isfinite(ref.best[b]):
                        assert (ref.score[ref.rec[b, :L]] == 0).all() and (ref.rec[b, L:] == -1).all()
                        for t in range(L):
                            assert ref.score[br.offsets[b * N + t] : br.offsets[b * N + t + 1]].max() == 0
                    else:
                        assert (ref.rec[b] == -1).all() and (ref.path[b] == -1).all()


def test_doctored_records_in_the_restatement(mm):
    """Entry indices -1, nnz and the phony self-loop's are dead records; offsets that decrease or reach behind nrec are clamped; a
    smaller nrec is the truncated lattice: the restatement against the enumeration over the same doctored arrays."""
    name, f, s2p, P, V, L, N = hand_graphs(mm)[3]  # ("ties, len 5")
    g = SimpleNamespace(state2pdf=s2p, P=P)
    sy = lr.system(f)
    _, offsets, arc = next(_lattices_of(f, g, V, L, N, (INF,)))
    clean = lb.reference([f], [g], V[None, :N], [L], offsets, arc)
    arc = arc.copy()
    lo1 = int(offsets[1])
    assert int(offsets[2]) - lo1 >= 4
    arc[lo1], arc[lo1 + 1], arc[lo1 + 2] = -1, sy.i.size, int(np.flatnonzero(sy.phony)[0])
    ref, through, best, rec = _against_brute_force(name, f, g, V, L, N, offsets, arc, None, exact=True)
    assert np.isfinite(best) and np.isneginf(ref.score[lo1 : lo1 + 3]).all() and not any(lo1 <= r < lo1 + 3 for r in rec)
    assert best <= float(clean.best[0])
    # a cut lattice: the cells behind nrec are empty, the utterance loses its paths
    cut = lb.reference([f], [g], V[None, :N], [L], offsets, arc, nrec=int(offsets[3]))
    assert cut.score.size == offsets[3] and np.isneginf(cut.best[0]) and np.isneginf(cut.score).all() and (cut.rec == -1).all()
    # offsets that decrease, are negative and reach behind nrec; lens beyond N and below 0
    bad = offsets.copy()
    bad[0], bad[3] = -5, 2 ** 40
    ref = lb.reference([f], [g], V[None, :N], [L + 7], bad, arc)
    cl = lp.cells(bad, arc.size, 0, N)
    through, best, rec = lb.brute_force(f, s2p, P, V, N, N, cl, arc)
    assert (np.isneginf(best) and np.isneginf(ref.best[0])) or float(ref.best[0]) == best
    assert np.isneginf(lb.reference([f], [g], V[None, :N], [-3], offsets, arc).best[0])


def test_gpu_case_conditions(mm, wl):
    """What tests/test_gpu_latticebest.py relies on, checked on the restatement: a seed with a unique best path for every utterance
    exists for its graph and lengths; at beam 3 the lattice of that seed holds a way round the third record of utterance 0's best
    path; the doctored offsets of its last case leave four records uncovered and every utterance its path."""
    g = on_grid(small_graphs(mm, wl)[1][0])
    f = wl.to_fsm(mm, g, semiring="tropical")
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    fs, gs = [f] * B, [g] * B
    seed, V = unique_best_seed(mm, wl, g, f, B, N, lens)
    br = lr.batch_reference(fs, gs, V, lens, 3.0)
    ref = lb.reference(fs, gs, V, lens, br.offsets, br.arc)
    assert np.isfinite(ref.best).all()
    extra = np.zeros(br.arc.size, dtype=np.float32)
    extra[ref.rec[0, 2]] = -np.inf
    again = lb.reference(fs, gs, V, lens, br.offsets, br.arc, extra)
    assert np.isfinite(again.best[0]) and again.best[0] < ref.best[0] and not (again.rec == ref.rec[0, 2]).any()
    g2, f2 = small_graphs(mm, wl)[1]
    V2 = emissions(31, B, N, g2.P, rounded=False, scale=1.0)
    full = lr.batch_reference([f2] * B, [g2] * B, V2, None, INF)
    gap = full.offsets.copy()
    gap[0], gap[-1] = 2, gap[-1] - 2
    ref = lb.reference([f2] * B, [g2] * B, V2, None, gap, full.arc)
    assert np.isnan(ref.score).sum() == 4 and np.isfinite(ref.best).all()


def test_rescore_and_onebest_on_host_arrays(mm, wl):
    """decode.lattice_rescore on the lattice's own V at a beam no wider than the lattice's is the reference lattice at that beam,
    member by member, bit for bit (grid inputs); with beam None it keeps every record with a finite score; under another V and an
    extra it keeps exactly the records within the beam of the NEW best, and the result goes back in with the same scores;
    decode.lattice_onebest returns one record per transition, connected, ending in the final state, whose weights add up to best."""
    g, f = small_graphs(mm, wl)[1]
    g = on_grid(g)
    f = wl.to_fsm(mm, g, semiring="tropical")
    B, N = 3, 6
    lens = np.array([6, 4, 0], dtype=np.int32)
    fs, gs = [f] * B, [g] * B
    V = emissions(9, B, N, g.P)
    br = lr.batch_reference(fs, gs, V, lens, 6.0)
    lat = as_lattice(mm, br)
    bf = restated_batch(mm, fs, gs)
    for beam2 in (0.0, 2.0, 6.0):
        rs = mm.decode.lattice_rescore(bf, lat, V, lens=lens, beam=beam2)
        want = lr.batch_reference(fs, gs, V, lens, beam2)
        assert isinstance(rs, mm.Lattice) and rs.counts.dtype == np.int32 and rs.offsets.dtype == np.int64
        assert bits(rs.counts, want.counts) and bits(rs.offsets, want.offsets) and bits(rs.arc, want.arc), beam2
        assert bits(rs.score, want.score.astype(np.float32)) and bits(rs.best, want.best.astype(np.float32)), beam2
    full = mm.decode.lattice_rescore(bf, lat, V, lens=lens)
    assert bits(full.arc, br.arc) and bits(full.counts, br.counts)
    V2 = emissions(10, B, N, g.P)
    extra = grid(record_scores(3, br.arc.size))
    ref = lb.reference(fs, gs, V2, lens, br.offsets, br.arc, extra)
    rs = mm.decode.lattice_rescore(bf, lat, V2, extra, lens, beam=1.0)
    keep = ref.score >= -1.0
    assert 0 < keep.sum() < keep.size and bits(rs.arc, br.arc[keep]) and bits(rs.score, ref.score[keep]) and bits(rs.best, ref.best)
    again = lb.reference(fs, gs, V2, lens, rs.offsets, rs.arc, extra[keep])
    assert bits(again.best, ref.best) and bits(again.score, ref.score[keep])  # (every path within the beam keeps all its records)
    with pytest.raises(ValueError):
        mm.decode.lattice_rescore(bf, lat, V, lens=lens, beam=-1.0)
    i, j, w = ar.fsm_entries(f)
    res = bf.latticebest(lat, V2, lens, extra)
    for b in range(B):
        t, k, src, dst = mm.decode.lattice_onebest(bf, lat, res, b)
        L = int(lens[b]) if np.isfinite(ref.best[b]) else 0
        assert t.tolist() == list(range(L)) and k.size == L
        if L:
            assert np.array_equal(src[1:], dst[:-1]) and dst[-1] == f.S1 - 1 and np.array_equal(src, ref.path[b, :L])
            r = ref.rec[b, :L]
            total = float(lr.system(f).pi[src[0]]) + V2[b, 0, g.state2pdf[src[0]]] + w[k].sum() + extra[r].sum() + sum(V2[b, n + 1, g.state2pdf[dst[n]]] for n in range(L - 1))
            assert total == float(ref.best[b])
    with pytest.raises(ValueError):
        mm.decode.lattice_onebest(bf, lat, bf.latticebest(lat, V2, lens, extra, want_path=False), 0)
