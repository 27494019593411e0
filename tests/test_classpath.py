"""Best paths with arc classes (mm_classpath_f32) without a GPU: the bindings of the new entries, the argument checks that need no
device, the NumPy restatement of tests/classpath_reference.py -- the header's definition -- against brute-force enumeration of every
state sequence of tiny graphs and of a hand-built FSM with parallel entries, the consequences (a) .. (e) the header states on the
restatement, and decode.events / decode.segments on hand-written tracks.  The cases of tests/test_gpu_classpath.py are built here,
with their non-vacuity asserted from the restatement alone."""
import ctypes as C
import os
import re

import numpy as np

import arc_reference as ar
import classpath_reference as cr
import vitwindow_reference as vr
from test_viterbiwindow import _tiny, case_base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases the GPU tests run
def with_parallels(mm, f, every=5):
    """FSM f with a parallel twin behind every `every`-th stored entry (the phony self-loop never): the twin's weight is the
    entry's own (an exact tie between parallels), or for every other twin 3/16 more or less.  Returns (FSM, twin [nnz'] bool,
    orig [nnz']: the entry of f behind each entry)."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    rows, vals, twin, orig, colptr = [], [], [], [], [0]
    t = 0
    for col in range(S1):
        for k in range(int(f.colptr[col]), int(f.colptr[col + 1])):
            rows.append(i[k]); vals.append(w[k]); twin.append(False); orig.append(k)
            if k % every == 0 and not (i[k] == S1 - 1 and col == S1 - 1):
                rows.append(i[k]); vals.append(w[k] + (0.0, 0.1875, 0.0, -0.1875)[t % 4]); twin.append(True); orig.append(k)
                t += 1
        colptr.append(len(rows))
    f2 = mm.FSM.from_fields(f.alpha_idx, f.alpha_val, colptr, rows, np.asarray(vals, dtype=np.float32), f.labels, semiring="tropical")
    return f2, np.array(twin), np.array(orig)


LAYOUTS = ("dst", "dst_nophony", "marks", "marks_phony")


def layout(g, f, twin, name):
    """(cls [nnz], C).  dst: the destination's pdf (the phony pdf = P: the final arcs and the phony loop), a twin P + 1 higher;
    dst_nophony: the same with the phony loop unclassified; marks: boundary marks on a few arcs in three classes, the rest -1;
    marks_phony: the same with the phony loop in a class of its own."""
    i, j, _ = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    phony = (i == S1 - 1) & (j == S1 - 1)
    if name.startswith("dst"):
        cls = (ar._s2p_full(g)[j] + (g.P + 1) * twin).astype(np.int32)
        if name == "dst_nophony":
            cls[phony] = -1
        return cls, 2 * (g.P + 1)
    cls = np.full(i.size, -1, dtype=np.int32)
    k = np.arange(i.size)
    pick = (k % 4 == 1) & ~phony
    cls[pick] = (k[pick] // 4) % 3
    if name == "marks_phony":
        cls[phony] = 3
    return cls, 4


def scores(seed, B, N, nc, ninf=12):
    """U [B, N, nc] = 2 N(0, 1), on the 1/16 grid, with ninf entries of -inf per utterance."""
    rng = np.random.default_rng(seed)
    U = 2.0 * rng.standard_normal((B, N, nc))
    U = (np.round(U * 16) / 16).astype(np.float32)
    for b in range(B):
        for _ in range(ninf):
            U[b, rng.integers(N), rng.integers(nc)] = -np.inf
    return U


def case_classes(mm, wl, rounded=True):
    """case_base of test_viterbiwindow.py (40 states, B = 6, N = 40, lens with 1, 0 and a dead utterance) with parallel twins:
    (g, f, twin, V, lens)."""
    gs, V, lens = case_base(wl, rounded)
    f, twin, _ = with_parallels(mm, wl.to_fsm(mm, gs[0], semiring="tropical"))
    return gs[0], f, twin, V, lens


def references(f, g, cls, nc, U, V, lens, dtype=np.float32):
    return [cr.reference(f, g.state2pdf, g.P, cls, nc, None if U is None else U[b], V[b], int(lens[b]), V.shape[1], dtype) for b in range(V.shape[0])]


def hand_built(mm):
    """Three states in a row with parallel entries: 0 -> 1 twice (classes 0 and 1, the same weight: the class rule decides), 1 -> 2
    three times (class 2, class 1 half a unit worse, and an unclassified one of class 2's weight: -1 loses the tie).  A pdf per
    state.  Returns (FSM, s2p, P, cls, C)."""
    #        col 0      col 1                    col 2                               col 3 (final)
    rows = [0,         0, 0, 1,                 1, 1, 1, 2,                         2, 3]
    vals = [-1.0,      -0.5, -0.5, -1.0,        -0.25, -0.75, -0.25, -1.0,          0.0, 0.0]
    cls = [-1,         1, 0, -1,                2, 1, -1, 4,                        3, -1]
    f = mm.FSM.from_fields([0], [0.0], [0, 1, 4, 8, 10], rows, np.asarray(vals, dtype=np.float32), list("abc"), semiring="tropical")
    return f, np.arange(3, dtype=np.int32), 3, np.asarray(cls, dtype=np.int32), 5


# ---- the tests
def test_entry_is_bound(mm):
    """The library exports the three entries (it loads without a GPU), the Python mirror binds them, the host interface, decode.py
    and the Julia wrappers are there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert all(s in mm.SYMBOLS for s in ("mm_classpath_f32", "mm_batch_set_path_classes", "mm_batch_path_class_info"))
    assert lib.mm_classpath_f32.argtypes is not None and len(lib.mm_classpath_f32.argtypes) == 16
    assert len(lib.mm_batch_set_path_classes.argtypes) == 4 and len(lib.mm_batch_path_class_info.argtypes) == 3
    assert callable(mm.classbestpath) and all(hasattr(mm.BatchedFSM, k) for k in ("classpath", "set_path_classes", "path_class_info"))
    assert all(callable(getattr(mm.decode, k)) for k in ("events", "segments", "forced_alignment"))
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_classpath_f32(" in hdr and "int mm_batch_set_path_classes(" in hdr and "int mm_batch_path_class_info(" in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    for sym, fn in (("mm_classpath_f32", "classpath"), ("mm_batch_set_path_classes", "set_path_classes!"), ("mm_batch_path_class_info", "path_class_info")):
        assert re.search(rf"ccall\(\(:{sym}, LIB\)", src) and f"function {fn}(" in src, sym


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: path or score NULL (-1), path_stride_b or classes_stride_b < N
    (-2); with those in order the NULL batch is what is refused (-1).  The setter and the info entry refuse a NULL batch."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(path=None, score=None, psb=8, classes=None, csb=8, N=8):
        return lib.mm_classpath_f32(None, p, 8, 1, None, N, None, 0, 0, 0, path, psb, classes, csb, score, None)

    assert call() == -1 and b"path/score is NULL" in lib.mm_last_error()
    assert call(path=p) == -1 and b"path/score is NULL" in lib.mm_last_error()
    assert call(path=p, score=p, psb=7) == -2 and b"path_stride_b" in lib.mm_last_error()
    assert call(path=p, score=p, classes=p, csb=7) == -2 and b"classes_stride_b" in lib.mm_last_error()
    assert call(path=p, score=p, csb=7) == -1 and b"NULL batch" in lib.mm_last_error()  # (classes NULL: its stride is not looked at)
    assert call(path=p, score=p, classes=p) == -1 and b"NULL batch" in lib.mm_last_error()
    ids = (C.c_int32 * 4)()
    assert lib.mm_batch_set_path_classes(None, C.cast(ids, C.c_void_p), None, 2) == -1
    assert lib.mm_batch_path_class_info(None, None, None) == -1


def _check_enumeration(f, s2p, P, cls, nc, U, V, L, what):
    r = cr.reference(f, s2p, P, cls, nc, U, V, L, V.shape[0], dtype=np.float64)
    path, classes, score = cr.enumerate_paths(f, s2p, P, cls, nc, U, V, L)
    if path is None:
        assert np.isneginf(r.score) and (r.path == -1).all() and (r.classes == -1).all(), what
        return False
    assert abs(r.score - score) <= 1e-10, (what, r.score, score)
    assert np.array_equal(r.path[:L], path) and (r.path[L:] == -1).all(), (what, r.path, path)
    assert np.array_equal(r.classes[:L], classes) and (r.classes[L:] == -1).all(), (what, r.classes, classes)
    return True


def test_reference_against_path_enumeration(mm, wl):
    """Graphs of up to 5 states, up to 5 frames, a pdf per state; classes per entry, by destination and sparse; without scores and
    with random scores with -inf entries."""
    rng = np.random.default_rng(71)
    found = 0
    for g in _tiny(wl):
        f = wl.to_fsm(mm, g, semiring="tropical")
        i, j, _ = ar.fsm_entries(f)
        sparse = np.full(f.nnz, -1)
        sparse[::2] = 0
        sparse[1::4] = 2
        for name, cls, nc in (("entry", np.arange(f.nnz), f.nnz), ("dst", ar._s2p_full(g)[j], g.P + 1), ("sparse", sparse, 3)):
            for L in (1, 3, 5):
                V = (2.0 * rng.standard_normal((5, g.P))).astype(np.float32)
                U = (2.0 * rng.standard_normal((5, nc))).astype(np.float32)
                U[rng.integers(5), rng.integers(nc)] = -np.inf
                for u in (None, U):
                    found += _check_enumeration(f, g.state2pdf, g.P, cls, nc, u, V, L, (g.name, name, L, u is None))
    assert found >= 40, found
    # L = 0 and a transition whose every class is blocked: no path
    g = _tiny(wl)[0]
    f = wl.to_fsm(mm, g, semiring="tropical")
    V = rng.standard_normal((4, g.P)).astype(np.float32)
    r = cr.reference(f, g.state2pdf, g.P, np.arange(f.nnz), f.nnz, None, V, 0, 4)
    assert np.isneginf(r.score) and (r.path == -1).all() and (r.classes == -1).all()
    U = np.zeros((4, f.nnz), dtype=np.float32)
    U[1] = -np.inf
    r = cr.reference(f, g.state2pdf, g.P, np.arange(f.nnz), f.nnz, U, V, 4, 4)
    assert np.isneginf(r.score) and (r.path == -1).all() and (r.classes == -1).all() and not np.isnan(r.score)


def test_parallel_entries_the_class_rule_and_a_score(mm):
    """The hand-built FSM: the only state sequence of 3 frames is 0 1 2.  Without scores the tie 0 -> 1 goes to class 0 (the lower
    id, stored second) and the tie 1 -> 2 to class 2 (the unclassified twin is behind every class); a score of one unit on class
    1 at transition 1 decides 1 -> 2 for the entry half a unit worse; -inf on class 0 at transition 0 hands 0 -> 1 to class 1."""
    f, s2p, P, cls, nc = hand_built(mm)
    V = np.zeros((3, P), dtype=np.float32)
    for dt in (np.float32, np.float64):
        r = cr.reference(f, s2p, P, cls, nc, None, V, 3, 3, dt)
        assert r.path.tolist() == [0, 1, 2] and r.classes.tolist() == [0, 2, 3] and r.score == -0.75 and r.par_ties >= 2
        U = np.zeros((3, nc), dtype=np.float32)
        U[1, 1] = 1.0
        U[0, 0] = -np.inf
        r = cr.reference(f, s2p, P, cls, nc, U, V, 3, 3, dt)
        assert r.path.tolist() == [0, 1, 2] and r.classes.tolist() == [1, 1, 3] and r.score == -0.25, (r.classes, r.score)
        assert r.entries.tolist() == [1, 5, 8]
    for U in (None, np.zeros((3, nc), dtype=np.float32), U):
        assert _check_enumeration(f, s2p, P, cls, nc, U, V, 3, "hand-built")
    # four frames: a loop somewhere; the enumeration agrees on path and classes (distinct emissions: no tie between sequences)
    V4 = np.array([[0, -9, -9], [-0.5, 0.125, -9], [-9, 0.25, 0], [-9, -9, 0.5]], dtype=np.float32)
    U4 = np.zeros((4, nc), dtype=np.float32)
    U4[2, 1] = 1.0
    assert _check_enumeration(f, s2p, P, cls, nc, U4, V4, 4, "hand-built, 4 frames")


def test_consequences_on_the_restatement(mm, wl):
    """(a) .. (e) of the header, in float32 on the 1/16 grid, on the GPU tests' base case."""
    g, f, twin, V, lens = case_classes(mm, wl, rounded=True)
    B, N, _ = V.shape
    cls, nc = layout(g, f, twin, "dst")
    U = scores(5, B, N, nc)
    plain = references(f, g, None, 0, None, V, lens)
    scored = references(f, g, cls, nc, U, V, lens)
    # (a) U None: path and score of the recursion without a plan, whatever the plan -- and on the graph without twins those of the
    # windowed entry's restatement, closed from the FSM's own start (mm_viterbi_f32's)
    for name in LAYOUTS:
        c, n = layout(g, f, twin, name)
        for r, r0 in zip(references(f, g, c, n, None, V, lens), plain):
            assert np.array_equal(r.path, r0.path) and r.score == r0.score, name
    f0 = wl.to_fsm(mm, g, semiring="tropical")
    for b, r in enumerate(references(f0, g, None, 0, None, V, lens)):
        r0 = vr.reference(g, V[b], int(lens[b]), N, None, True, dtype=np.float32)
        assert np.array_equal(r.path, r0.path) and (r.score == r0.score or (np.isneginf(r.score) and np.isneginf(r0.score)))
    # (b) U constant in t: mm_viterbi_f32 on the FSM with the weights w_k + u_cls[k]
    u = U[0, 3].copy()
    u[np.isneginf(u)] = -2.5
    Uc = np.broadcast_to(u, (B, N, nc)).copy()
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    w2 = w.astype(np.float32).copy()
    m = (cls >= 0) & ~((i == S1 - 1) & (j == S1 - 1))
    w2[m] += u[cls[m]]
    f2 = mm.FSM.from_fields(f.alpha_idx, f.alpha_val, f.colptr, f.rowval, w2, f.labels, semiring="tropical")
    for r, r2 in zip(references(f, g, cls, nc, Uc, V, lens), references(f2, g, None, 0, None, V, lens)):
        assert np.array_equal(r.path, r2.path) and (r.score == r2.score or (np.isneginf(r.score) and np.isneginf(r2.score)))
    # (c) -inf removes the class from the transition
    for b, r in enumerate(scored):
        t, c = np.nonzero(np.isneginf(U[b, : lens[b]]))
        assert (r.classes[t] != c).all()
    # (d) the score is the sum along the returned path in the recursion's order
    for b, r in enumerate(scored):
        if np.isfinite(r.score):
            L = int(lens[b])
            assert cr.path_score(f, g.state2pdf, g.P, cls, U[b], V[b], r.path[:L], r.entries[:L]) == r.score
    # (e) an order-preserving relabelling changes `classes` by that map and nothing else
    up = lambda c: np.where(c < 0, -1, 2 * c + 1)
    U2 = np.zeros((B, N, 2 * nc + 1), dtype=np.float32)
    U2[:, :, 1::2] = U
    for r, r2 in zip(scored, references(f, g, up(cls), 2 * nc + 1, U2, V, lens)):
        assert np.array_equal(r2.path, r.path) and np.array_equal(r2.classes, up(r.classes)) and (r2.score == r.score or np.isneginf(r.score))


def test_base_case_is_not_vacuous(mm, wl):
    """From the restatement alone: with the base scores the path differs from the unscored one on at least a quarter of the live
    frames of each full-length utterance; at least one exact tie between sources and one between parallels is decided; the -inf
    entries bind (the unscored path takes a forbidden class somewhere); the dead and the empty utterance have no path."""
    for rounded in (True, False):
        g, f, twin, V, lens = case_classes(mm, wl, rounded)
        B, N, _ = V.shape
        for name in ("dst", "marks"):
            cls, nc = layout(g, f, twin, name)
            U = scores(5, B, N, nc)
            plain = references(f, g, cls, nc, None, V, lens)
            scored = references(f, g, cls, nc, U, V, lens)
            diff = [int((p.path[: lens[b]] != s.path[: lens[b]]).sum()) for b, (p, s) in enumerate(zip(plain, scored))]
            bound = sum(int((p.classes[t] == c).sum()) for b, p in enumerate(plain) for t, c in [np.nonzero(np.isneginf(U[b, : lens[b]]))])
            ties = (sum(r.src_ties for r in scored), sum(r.par_ties for r in scored))
            print(f"rounded {rounded}, {name}: frames that differ {diff} of {lens.tolist()}, forbidden classes on the unscored path {bound}, ties {ties}")
            assert np.isneginf(scored[3].score) and np.isneginf(scored[4].score) and np.isfinite(scored[2].score)
            if name == "dst":
                assert all(np.isfinite(scored[b].score) and diff[b] >= lens[b] / 4 for b in (0, 5)), diff
                assert bound >= 1
            if rounded:
                assert ties[0] >= 1 and ties[1] >= 1, ties
            assert any((r.classes[: lens[b]] == -1).any() for b, r in enumerate(scored) if np.isfinite(r.score)) == (name == "marks")


def test_decode_events_and_segments(mm):
    classes = np.array([[-1, 2, -1, -1, 0, 3, -1, -1], [1, 1, -1, 5, -1, -1, -1, -1], [-1] * 8, [-1] * 8])
    lens = np.array([6, 4, 3, 0])
    assert mm.decode.events(classes, lens) == [[(2, 1), (0, 4), (3, 5)], [(1, 0), (1, 1), (5, 3)], [], []]
    assert mm.decode.events(classes, lens, ignore=(-1, 1, 3)) == [[(2, 1), (0, 4)], [(5, 3)], [], []]
    assert mm.decode.segments(classes, lens, boundary=2) == [[(0, 2), (2, 6)], [(0, 4)], [(0, 3)], []]
    assert mm.decode.segments(classes, lens, boundary=1) == [[(0, 6)], [(0, 1), (1, 2), (2, 4)], [(0, 3)], []]
    assert mm.decode.segments(classes, lens, boundary=3) == [[(0, 6)], [(0, 4)], [(0, 3)], []]  # (a boundary on the final arc ends the last run as it is)
