"""Lattice posteriors (mm_latticeposteriors_f32) without a GPU: the bindings of the new entry, the argument checks that need no
device, the float64 restatement of tests/latpost_reference.py -- the header's definition -- against brute-force enumeration of every
lattice path of hand-built graphs (parallel entries, extra given and NULL, V with -inf entries, doctored records), against the
oracle's float64 pdfposteriors on the beam = inf lattice (every arc with a finite score kept: logz and gamma are the full graph's),
and against finite differences of its own logz (gamma = d logz / d V, exp(post) = d logz / d extra); decode.lattice_prune on host
arrays.  The cases of tests/test_gpu_latticeposteriors.py are built here."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import latpost_reference as lp
import lattice_reference as lr
from test_lattice import INF, as_lattice, emissions, grid, hand_graphs, stub_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cell sizes around the workgroup of the forward-backward (1024 threads: one record per thread in registers, the others gathered
# again: a second and a third turn) and its waves (64), and around the 256 threads of the per-pdf sums
CELL_COUNTS = (1, 63, 65, 255, 257, 1023, 1024, 1025, 2049)


# ---- the cases the GPU tests run
def small_graphs(mm, wl):
    """(g, f) of the 3-state left-to-right graph and a 40-state random graph, tropical."""
    return [(g, wl.to_fsm(mm, g, semiring="tropical")) for g in (wl.l2r_hmm(3), wl.random_fsm(40, 5, 3.0, seed=11, n_init=3))]


def record_scores(seed, n, scale=1.0):
    """An `extra` for n records: standard-normal scores (a rescoring), float32."""
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def log_twin(o, f):
    """The oracle's log-semiring FSM with the weights of the tropical product FSM f, through its arc-list constructor."""
    i, j, w = ar.fsm_entries(f)
    S = f.colptr.size - 2
    real = j < S
    fin = (j == S) & (i < S)
    return o.make_fsm(o.SEMIRINGS["log"], list(zip((int(s) for s in f.alpha_idx), (float(np.float32(v)) for v in f.alpha_val))),
                      [((int(a), int(b)), float(np.float32(v))) for a, b, v in zip(i[real], j[real], w[real])],
                      [(int(a), float(np.float32(v))) for a, v in zip(i[fin], w[fin])], list(range(S)), np.float64)


# ---- the tests
def test_entry_is_bound(mm):
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_latticeposteriors_f32" in mm.SYMBOLS and len(lib.mm_latticeposteriors_f32.argtypes) == 16
    assert callable(mm.latticeposteriors) and hasattr(mm.BatchedFSM, "latticeposteriors")
    assert mm.LatticePosteriors._fields == ("post", "logz", "gamma")
    assert callable(mm.decode.lattice_prune) and mm.lattice_prune is mm.decode.lattice_prune
    assert callable(mm.lattices.lattice_loglik) and mm.lattice_loglik is mm.lattices.lattice_loglik
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_latticeposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr and "19 = mm_latticeposteriors_f32" in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_latticeposteriors_f32, LIB\)", src) and "function latticeposteriors(" in src


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: offsets or logz NULL (-1), a negative nrec (-1), arc or post NULL
    with records to read (-1), gamma strides that overlap rows (-2); with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))

    def call(offsets=p, arc=p, nrec=4, extra=None, post=fp, logz=fp, gamma=None, gsb=0, gsn=0, N=8):
        return lib.mm_latticeposteriors_f32(None, fp, 8, 1, None, N, offsets, arc, nrec, extra, post, logz, gamma, gsb, gsn, None)

    for kw in ({"offsets": None}, {"logz": None}, {"arc": None}, {"post": None}):
        assert call(**kw) == -1 and b"is NULL" in lib.mm_last_error(), kw
    assert call(nrec=-1) == -1 and b"nrec" in lib.mm_last_error()
    assert call(gamma=fp, gsb=8 * 4 - 1, gsn=4) == -2 and b"gamma_stride" in lib.mm_last_error()
    assert call(gamma=fp, gsb=0, gsn=0) == -2 and b"gamma_stride" in lib.mm_last_error()
    assert call() == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(arc=None, post=None, nrec=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (an empty lattice needs neither)
    assert call(gamma=fp, gsb=32, gsn=4, extra=fp) == -1 and b"NULL batch" in lib.mm_last_error()


def _lattices_of(f, g, V, L, N, beams=(INF, 1.0)):
    for beam in beams:
        r = lr.reference(f, g.state2pdf, g.P, V, L, N, beam)
        yield beam, np.concatenate([[0], np.cumsum(r.counts, dtype=np.int64)]), r.arc


def test_restatement_against_brute_force(mm):
    """Every hand graph of test_lattice (parallel entries with ties, two state sequences, a dead end, no path, len 0 and 1), the
    lattices of beam inf and 1 under ANOTHER V, with extra NULL and given, and with -inf in V that removes records: post, logz and
    gamma of the restatement are the enumeration's; the posteriors of every cell of an utterance with a path sum to 1."""
    seen_dead_record = seen_no_path = seen_parallel = False
    for name, f, s2p, P, V, L, N in hand_graphs(mm):
        g = SimpleNamespace(state2pdf=s2p, P=P)
        i, j, _ = ar.fsm_entries(f)
        for beam, offsets, arc in _lattices_of(f, g, V, L, N):
            V2 = grid(V + 0.5 * np.random.default_rng(len(name)).standard_normal(V.shape))
            V3 = V2.copy()
            if N > 2:
                V3[1, 0] = -np.inf  # (frame 1 no longer emits pdf 0: the records into its states die)
            V4 = V2.copy()
            V4[min(1, N - 1)] = -np.inf  # (a frame that emits nothing: the records stay, every path dies)
            for Vn in (V, V2, V3, V4):
                for extra in (None, record_scores(7, arc.size)):
                    ref = lp.reference([f], [g], Vn[None, :N], [L], offsets, arc, extra)
                    cl = lp.cells(offsets, arc.size, 0, N)
                    through, logz = lp.brute_force(f, s2p, P, Vn, L, N, cl, arc, extra)
                    what = (name, beam, extra is not None)
                    assert np.isneginf(logz) == np.isneginf(ref.logz[0]) and (np.isneginf(logz) or abs(logz - ref.logz[0]) <= 1e-12 * max(1, abs(logz))), what
                    want = np.array([through.get(r, -np.inf) - logz if logz > -np.inf else -np.inf for r in range(arc.size)])
                    assert np.array_equal(np.isneginf(want), np.isneginf(ref.post)), what
                    fin = ~np.isneginf(want)
                    assert np.allclose(ref.post[fin], want[fin], rtol=0, atol=1e-12), what
                    gam = np.zeros((N, P))
                    for t, (lo, hi) in enumerate(cl[:L]):
                        for r in range(lo, hi):
                            if fin[r]:
                                gam[t, s2p[i[arc[r]]]] += np.exp(want[r])
                        if logz > -np.inf:
                            assert abs(np.exp(ref.post[lo:hi]).sum() - 1) <= 1e-12, what
                    assert np.allclose(ref.gamma[0], gam, rtol=0, atol=1e-12) and (ref.gamma[0, L:] == 0).all(), what
                    seen_no_path |= arc.size > 0 and np.isneginf(logz)
                    seen_dead_record |= logz > -np.inf and bool(np.isneginf(want).any())
                    for lo, hi in cl[:L]:
                        pairs = list(zip(i[arc[lo:hi]].tolist(), j[arc[lo:hi]].tolist()))
                        seen_parallel |= logz > -np.inf and len(set(pairs)) < len(pairs)
    assert seen_dead_record and seen_no_path and seen_parallel, (seen_dead_record, seen_no_path, seen_parallel)


def test_doctored_records_in_the_restatement(mm):
    """Entry indices -1, nnz and the phony self-loop's are dead records; offsets that decrease or reach behind nrec are clamped; a
    smaller nrec is the truncated lattice: the restatement against the enumeration over the same doctored arrays."""
    name, f, s2p, P, V, L, N = hand_graphs(mm)[3]  # ("ties, len 5")
    g = SimpleNamespace(state2pdf=s2p, P=P)
    sy = lr.system(f)
    _, offsets, arc = next(_lattices_of(f, g, V, L, N, (INF,)))
    arc = arc.copy()
    phony = int(np.flatnonzero(sy.phony)[0])
    lo1, hi1 = int(offsets[1]), int(offsets[2])
    assert hi1 - lo1 >= 4
    arc[lo1], arc[lo1 + 1], arc[lo1 + 2] = -1, sy.i.size, phony
    ref = lp.reference([f], [g], V[None, :N], [L], offsets, arc)
    through, logz = lp.brute_force(f, s2p, P, V, L, N, lp.cells(offsets, arc.size, 0, N), arc)
    assert np.isfinite(logz) and abs(ref.logz[0] - logz) <= 1e-12 and np.isneginf(ref.post[lo1 : lo1 + 3]).all()
    assert all(abs(ref.post[r] - (v - logz)) <= 1e-12 for r, v in through.items()) and not any(lo1 <= r < lo1 + 3 for r in through)
    # a cut lattice: the cells behind nrec are empty, the utterance loses its paths
    cut = lp.reference([f], [g], V[None, :N], [L], offsets, arc, nrec=int(offsets[3]))
    assert cut.post.size == offsets[3] and np.isneginf(cut.logz[0]) and np.isneginf(cut.post).all() and (cut.gamma == 0).all()
    assert lp.cells(np.array([0, 5, 3, 9, 2 ** 40, -4]), 7, 0, 5) == [(0, 5), (5, 5), (3, 7), (7, 7), (7, 7)]


def test_restatement_against_the_oracle_on_full_lattices(mm, wl, oracle):
    """beam = inf keeps every arc with a finite through-score: logz and gamma of the lattice under the SAME V are the oracle's
    float64 pdfposteriors of the same weights as a log-semiring FSM, lens included."""
    o = oracle[0]
    for g, f in small_graphs(mm, wl):  # (the graphs the GPU parity test runs)
        B, N = 3, 6
        lens = np.array([6, 1, 0], dtype=np.int32)
        V = emissions(3, B, N, g.P, rounded=False, scale=1.0)
        br = lr.batch_reference([f] * B, [g] * B, V, lens, INF)
        ref = lp.reference([f] * B, [g] * B, V, lens, br.offsets, br.arc)
        live = [b for b in range(B) if lens[b] > 0]
        gam, ttl = o.pdfposteriors_batch(log_twin(o, f), list(g.state2pdf), g.P, [V[b].T.astype(np.float64) for b in live], [int(lens[b]) for b in live])
        for q, b in enumerate(live):
            L = int(lens[b])
            if np.isneginf(ttl[q]):  # (neither graph has a path of one frame)
                assert L == 1 and np.isneginf(ref.logz[b]) and (ref.gamma[b] == 0).all()
                continue
            assert np.isfinite(ttl[q]) and abs(ref.logz[b] - ttl[q]) <= 1e-9 * abs(ttl[q]), (g.name, b, ref.logz[b], ttl[q])
            assert np.allclose(ref.gamma[b, :L], gam[q].T[:L], rtol=0, atol=1e-9), (g.name, b)
        assert np.isneginf(ref.logz[2]) and (ref.gamma[2] == 0).all()


def test_gradients_of_the_restatement_by_finite_differences(mm, wl):
    """gamma = d logz / d V and exp(post) = d logz / d extra: central differences of the restatement's own logz with a step of
    2^-8 on inputs of the 1/16 grid (every perturbed input is a float32: the restatement reads V and the weights as float32).  The
    truncation error of a central difference is h^2 / 6 times a third derivative of a log-partition function, which is a third
    cumulant of an indicator and at most 1 in size: 2.6e-6; the bar is 2e-5."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 1, 5
    V = emissions(5, B, N, g.P)
    br = lr.batch_reference([f], [g], V, None, 3.0)
    extra = grid(record_scores(3, br.arc.size))
    ref = lp.reference([f], [g], V, None, br.offsets, br.arc, extra)
    assert np.isfinite(ref.logz[0]) and br.arc.size > 20
    h = 2.0 ** -8
    logz = lambda Vn, en: lp.reference([f], [g], Vn, None, br.offsets, br.arc, en).logz[0]
    for n in range(N):
        for p in range(g.P):
            Vp, Vm = V.copy(), V.copy()
            Vp[0, n, p] += h
            Vm[0, n, p] -= h
            assert abs((logz(Vp, extra) - logz(Vm, extra)) / (2 * h) - ref.gamma[0, n, p]) <= 2e-5, (n, p)
    for r in range(0, br.arc.size, 3):
        ep, em = extra.copy(), extra.copy()
        ep[r] += h
        em[r] -= h
        assert abs((logz(V, ep) - logz(V, em)) / (2 * h) - np.exp(ref.post[r])) <= 2e-5, r


def test_lattice_prune_on_host_arrays(mm, wl):
    """The records with post >= log(threshold), in their order, with counts and offsets recomputed -- NumPy members and CPU tensors
    alike; threshold 0 drops only the records without a path; the result goes back into the restatement (whose posteriors of the
    kept records can only grow), into lattice_arcs and lattice_fsm."""
    import torch

    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    lens = np.array([6, 4, 0], dtype=np.int32)
    V = emissions(9, B, N, g.P)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, 6.0)
    lat = as_lattice(mm, br)
    V2 = emissions(10, B, N, g.P)
    ref = lp.reference([f] * B, [g] * B, V2, lens, br.offsets, br.arc)
    post = ref.post.astype(np.float32)
    for thr in (0.0, 0.05, 0.5):
        keep = post >= (np.log(thr) if thr > 0 else -np.inf)
        keep &= ~np.isneginf(post)
        assert 0 < keep.sum() and (thr == 0 or keep.sum() < keep.size)
        pr = mm.decode.lattice_prune(lat, post, thr)
        assert isinstance(pr, mm.Lattice) and isinstance(pr.arc, np.ndarray) and pr.counts.dtype == np.int32 and pr.offsets.dtype == np.int64
        assert np.array_equal(pr.arc, br.arc[keep]) and np.array_equal(pr.score, br.score[keep]) and pr.best is lat.best
        cell = np.searchsorted(br.offsets[1:], np.flatnonzero(keep), side="right")
        assert np.array_equal(pr.counts.reshape(-1), np.bincount(cell, minlength=B * N)) and pr.counts.shape == (B, N)
        assert np.array_equal(pr.offsets, np.concatenate([[0], np.cumsum(pr.counts.reshape(-1))])) and pr.offsets[-1] == keep.sum()
        tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)) for x in lat))
        pt = mm.decode.lattice_prune(tl, torch.from_numpy(post), thr)
        assert all(isinstance(x, torch.Tensor) for x in pt[:4])
        assert all(np.array_equal(a.numpy(), b) and a.numpy().dtype == b.dtype for a, b in zip(pt[:4], pr[:4]))
        again = lp.reference([f] * B, [g] * B, V2, lens, pr.offsets, pr.arc)
        if thr == 0:
            assert np.allclose(again.post, ref.post[keep], rtol=0, atol=1e-12) and np.allclose(again.logz[:2], ref.logz[:2], rtol=0, atol=1e-12)
        assert (again.logz[:2] <= ref.logz[:2] + 1e-12).all()
        bf = stub_batch(mm, [f] * B, [g] * B)
        t, k, src, dst, s = mm.decode.lattice_arcs(bf, pr, 0)
        lo, hi = int(pr.offsets[0]), int(pr.offsets[N])
        assert np.array_equal(k, pr.arc[lo:hi]) and np.array_equal(t, np.repeat(np.arange(N), pr.counts[0]))
        lf, s2p = mm.decode.lattice_fsm(bf, pr, 0)
        assert lf.semiring == "tropical" and len(s2p) == lf.S1 - 1
    with pytest.raises(ValueError):
        mm.decode.lattice_prune(lat, post[:-1], 0.5)
    with pytest.raises(ValueError):
        mm.decode.lattice_prune(lat, post, -0.1)
    with pytest.raises(ValueError):
        mm.decode.lattice_prune(mm.Lattice(br.counts, br.offsets, br.arc[:5], br.score, br.best), post[:5], 0.5)
