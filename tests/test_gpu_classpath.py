"""Best paths with arc classes (mm_classpath_f32) on the MI355X against the float32 mode of tests/classpath_reference.py, and the
consequences the header states: (a) U NULL = viterbi, (b) constant scores = viterbi on the re-weighted FSM, (c) -inf removes a
class, repeats bit for bit; classes NULL, U NULL, hipGraph capture with U overwritten in place, the kernel instances, global
vectors by the plan, more pdfs than threads, class counts around the block size and the class cap, state indices beyond 16 bits,
distinct graphs with offsets, parallel entries, error codes, and decode.forced_alignment end to end.

The bar throughout is bit equality -- path, classes and score of every utterance of every case against the restatement that
performs the kernel's float32 operations in their order -- so there is no tolerance to measure."""
import copy
import ctypes as C

import numpy as np
import pytest

import arc_reference as ar
import class_cases as cc
import classpath_reference as cr
from test_classpath import LAYOUTS, case_classes, hand_built, layout, references, scores
from test_gpu_parity import _with_env

pytestmark = pytest.mark.gpu
STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
BIGV = {"MM_DEBUG": "1", "MM_BIGV": "1"}
BOTH = {"MM_DEBUG": "1", "MM_NITEMS": "0", "MM_BIGV": "1"}
TWO_WAVES = {"MM_DEBUG": "1", "MM_NWAVES": "2"}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib").lib


def _batch(mm, fs, gs):
    """One compiled FSM per distinct FSM object."""
    cache = {}
    for f, g in zip(fs, gs):
        if id(f) not in cache:
            cache[id(f)] = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    return mm.batch(*[cache[id(f)] for f in fs])


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and not np.isnan(a).any()


def _check(out, refs, what="", want_classes=True):
    """Every utterance, every output, bit for bit."""
    path, classes, score = out
    for b, r in enumerate(refs):
        w = (what, b)
        assert np.array_equal(path[b], r.path), (w, path[b], r.path)
        assert _same_bits(score[b], r.score), (w, score[b], r.score)
        if want_classes:
            assert np.array_equal(classes[b], r.classes), (w, classes[b], r.classes)


@pytest.fixture(scope="module")
def base(mm, wl):
    return case_classes(mm, wl, rounded=True)


@pytest.fixture(scope="module")
def unrounded(mm, wl):
    return case_classes(mm, wl, rounded=False)


def _run_layouts(mm, bf, case, what, names=LAYOUTS):
    g, f, twin, V, lens = case
    B, N, _ = V.shape
    for name in names:
        cls, nc = layout(g, f, twin, name)
        assert bf.set_path_classes(cls, nc) == nc and bf.path_class_info()["path_C"] == nc
        U = scores(5, B, N, nc)
        _check(bf.classpath(V, U, lens), references(f, g, cls, nc, U, V, lens), f"{what}, {name}, scored")
        _check(bf.classpath(V, None, lens), references(f, g, cls, nc, None, V, lens), f"{what}, {name}, U NULL")


@pytest.mark.parametrize("rounded", [True, False])
def test_base_case(mm, wl, torch, base, unrounded, rounded):
    case = base if rounded else unrounded
    g, f, twin, V, lens = case
    bf = _batch(mm, [f] * 6, [g] * 6)
    k = bf.kernels("classpath")
    assert "mm_classpath_fwd_kernel<8,lds>" in k and "mm_classpath_trace_kernel" in k and "no classes set" in k, k
    _run_layouts(mm, bf, case, f"base case, rounded {rounded}")
    assert "no classes set" not in bf.kernels("classpath")
    # the dead and the empty utterance, and the tails
    path, classes, score = bf.classpath(V, None, lens)
    assert np.isneginf(score[3]) and np.isneginf(score[4]) and (path[3] == -1).all() and (classes[4] == -1).all()
    assert (path[1, lens[1]:] == -1).all() and (classes[1, lens[1]:] == -1).all() and (path[1, : lens[1]] >= 0).all()


@pytest.mark.parametrize("env,inst", [(STREAMED, "<0,lds>"), (BIGV, "<8,global>"), (BOTH, "<0,global>")])
def test_instances(mm, wl, torch, base, env, inst):
    g, f, twin, V, lens = base
    bf = _with_env(env, lambda: _batch(mm, [f] * 6, [g] * 6))
    assert "mm_classpath_fwd_kernel" + inst in bf.kernels("classpath"), bf.kernels("classpath")
    _run_layouts(mm, bf, base, inst, names=("dst", "marks"))


def _dst_case(mm, wl, g, B, N, lens, seed):
    f = wl.to_fsm(mm, g, semiring="tropical")
    cls, nc = cc.dst_layout(g, f)
    V = np.random.default_rng(seed).standard_normal((B, N, g.P)).astype(np.float32)
    return f, cls, nc, V, np.asarray(lens, dtype=np.int32), scores(seed + 1, B, N, nc, ninf=3)


def test_vectors_global_by_the_plan(mm, wl, torch):
    """12 500 states: the vectors, the back-pointer and the class rows exceed the 160 KB of a compute unit; the plan itself puts
    them in global memory."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    f, cls, nc, V, lens, U = _dst_case(mm, wl, g, 2, 12, (12, 7), 4)
    bf = _batch(mm, [f, f], [g, g])
    bf.set_path_classes(cls, nc)
    assert ",global>" in bf.kernels("classpath"), bf.kernels("classpath")
    for u in (U, None):
        out = bf.classpath(V, u, lens)
        assert np.isfinite(out[2]).all()
        _check(out, references(f, g, cls, nc, u, V, lens), "12500 states")


def test_more_pdfs_than_threads(mm, wl, torch):
    """1100 pdfs against at most 1024 threads: a frame's emissions are staged in two parts -- and 1101 classes, the score row too."""
    g = wl.random_fsm(1200, 1100, 3.0, seed=9)
    f, cls, nc, V, lens, U = _dst_case(mm, wl, g, 3, 14, (14, 9, 2), 10)
    bf = _batch(mm, [f] * 3, [g] * 3)
    bf.set_path_classes(cls, nc)
    _check(bf.classpath(V, U, lens), references(f, g, cls, nc, U, V, lens), "1200 states, 1100 pdfs")


def test_class_counts_around_the_block_size_and_the_cap(mm, wl, torch, base):
    """C = NT - 2 .. NT + 2 on a two-wave block (both sides of `tid < C` and of `C > NT`, every padding of C + 1); C at the cap runs,
    C one above it is refused with the cap in the message."""
    g, f, twin, V, lens = base
    B, N, _ = V.shape
    bf = _with_env(TWO_WAVES, lambda: _batch(mm, [f] * B, [g] * B))
    for nc in cc.count_values(cc.NT_TWO_WAVES):
        cls = cc.count_layout(f, nc)
        bf.set_path_classes(cls, nc)
        U = scores(nc, B, N, nc)
        out = bf.classpath(V, U, lens)
        _check(out, references(f, g, cls, nc, U, V, lens), f"C = {nc}")
    one = _batch(mm, [f], [g])
    cap = one.path_class_info()["path_class_cap"]
    assert 1000 < cap <= 65534, cap
    cls = cc.count_layout(f, 50).astype(np.int32)
    cls[cls == 49] = cap - 1  # (the last class of the plan is used)
    one.set_path_classes(cls, cap)
    U = scores(3, 1, 3, cap, ninf=40)
    V3, l3 = np.ascontiguousarray(V[:1, :3]), np.array([3], dtype=np.int32)
    _check(one.classpath(V3, U, l3), references(f, g, cls, cap, U, V3, l3), "C at the cap")
    cls[cls == cap - 1] = cap
    one.set_path_classes(cls, cap + 1)
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        one.classpath(V3, np.zeros((1, 3, cap + 1), dtype=np.float32), l3)
    assert ei.value.code == -4 and str(cap) in str(ei.value), str(ei.value)
    assert "exceed the cap" in one.kernels("classpath")
    # ... without scores the plan is within reach: the ids still fit 16 bits
    _check(one.classpath(V3, None, l3), references(f, g, cls, cap + 1, None, V3, l3), "C above the cap, U NULL")


def test_beyond_16_bit_indices(mm, wl, torch):
    """The 70 000-state graph (<0,global> with no switch), classes of their own for the arcs with a state beyond 16 bits at either
    end: the best paths take some."""
    g = wl.random_fsm(70000, 40, 3.0, seed=3)
    f = wl.to_fsm(mm, g, semiring="tropical")
    cls, nc = cc.high_layout(g, f)
    B, N = 2, 6
    lens = np.array([6, 4], dtype=np.int32)
    V = np.random.default_rng(4).standard_normal((B, N, g.P)).astype(np.float32)
    U = scores(8, B, N, nc, ninf=3)
    U[:, :, g.P + 1 :] += 8.0  # (a bonus on the high classes draws a best path through states beyond 16 bits)
    bf = _batch(mm, [f, f], [g, g])
    bf.set_path_classes(cls, nc)
    assert "mm_classpath_fwd_kernel<0,global>" in bf.kernels("classpath"), bf.kernels("classpath")
    refs = references(f, g, cls, nc, U, V, lens)
    assert all(np.isfinite(r.score) for r in refs) and any((r.classes >= g.P + 1).any() for r in refs) and any((r.path >= cc.HIGH).any() for r in refs)
    _check(bf.classpath(V, U, lens), refs, "70000 states")


def test_distinct_graphs_with_offsets(mm, wl, torch):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    B, N = 4, 30
    lens = np.array([30, 22, 30, 17], dtype=np.int32)
    V = (2.0 * np.random.default_rng(21).standard_normal((B, N, 5))).astype(np.float32)
    fs = [wl.to_fsm(mm, g, semiring="tropical") for g in gs]
    clss = [cc.dst_layout(g, f, 6)[0] for g, f in zip(gs, fs)]
    clss[2] = np.where(np.arange(fs[2].nnz) % 3 == 0, -1, clss[2]).astype(np.int32)
    U = scores(22, B, N, 6, ninf=4)
    bf = _batch(mm, fs, gs)
    assert bf.set_path_classes(clss, 6) == 6
    for u in (U, None):
        out = bf.classpath(V, u, lens)
        refs = [cr.reference(f, g.state2pdf, g.P, c, 6, None if u is None else u[b], V[b], int(lens[b]), N) for b, (f, g, c) in enumerate(zip(fs, gs, clss))]
        assert sum(np.isfinite(r.score) for r in refs) >= 3
        _check(out, refs, "distinct graphs")


def test_parallel_entries(mm, wl, torch):
    """The hand-built FSM of test_classpath.py: the class rule decides a tie, a score decides between parallels."""
    f, s2p, P, cls, nc = hand_built(mm)
    g = wl.l2r_hmm(3)
    bf = _batch(mm, [f, f], [g, g])
    bf.set_path_classes(cls, nc)
    V = np.zeros((2, 4, P), dtype=np.float32)
    V[1] = np.array([[0, -9, -9], [-0.5, 0.125, -9], [-9, 0.25, 0], [-9, -9, 0.5]], dtype=np.float32)
    lens = np.array([3, 4], dtype=np.int32)
    U = np.zeros((2, 4, nc), dtype=np.float32)
    U[0, 1, 1], U[0, 0, 0], U[1, 2, 1] = 1.0, -np.inf, 1.0
    for u in (None, U):
        refs = [cr.reference(f, s2p, P, cls, nc, None if u is None else u[b], V[b], int(lens[b]), 4) for b in range(2)]
        _check(bf.classpath(V, u, lens), refs, "hand-built")
    assert refs[0].classes.tolist() == [1, 1, 3, -1]
    path, classes, _ = bf.classpath(V, None, lens)
    assert classes[0].tolist() == [0, 2, 3, -1] and path[0].tolist() == [0, 1, 2, -1]


def test_consequences(mm, wl, torch, base, unrounded):
    """(a) against bf.viterbi itself on the same batch, (b) against viterbi on a re-weighted FSM on the grid, (c) -inf removes the
    class."""
    for case in (base, unrounded):
        g, f, twin, V, lens = case
        B, N, _ = V.shape
        bf = _batch(mm, [f] * B, [g] * B)
        path0, score0 = bf.viterbi(V, lens)
        path, classes, score = bf.classpath(V, None, lens, want_classes=False)  # no plan at all
        assert classes is None and np.array_equal(path, path0) and _same_bits(score, score0)
        for name in LAYOUTS:
            cls, nc = layout(g, f, twin, name)
            bf.set_path_classes(cls, nc)
            for want in (True, False):
                path, _, score = bf.classpath(V, None, lens, want_classes=want)
                assert np.array_equal(path, path0) and _same_bits(score, score0), (name, want)
        # (c)
        cls, nc = layout(g, f, twin, "dst")
        bf.set_path_classes(cls, nc)
        U = scores(5, B, N, nc, ninf=40)
        path, classes, score = bf.classpath(V, U, lens)
        for b in range(B):
            t, c = np.nonzero(np.isneginf(U[b, : lens[b]]))
            assert (classes[b, t] != c).all()
    # (b) on the grid
    g, f, twin, V, lens = base
    B, N, _ = V.shape
    cls, nc = layout(g, f, twin, "dst")
    u = scores(6, 1, 1, nc, ninf=0)[0, 0]
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    w2 = w.astype(np.float32).copy()
    m = (cls >= 0) & ~((i == S1 - 1) & (j == S1 - 1))
    w2[m] += u[cls[m]]
    f2 = mm.FSM.from_fields(f.alpha_idx, f.alpha_val, f.colptr, f.rowval, w2, f.labels, semiring="tropical")
    path2, score2 = _batch(mm, [f2] * B, [g] * B).viterbi(V, lens)
    bf = _batch(mm, [f] * B, [g] * B)
    bf.set_path_classes(cls, nc)
    path, _, score = bf.classpath(V, np.broadcast_to(u, (B, N, nc)).copy(), lens)
    assert np.array_equal(path, path2) and _same_bits(score, score2)


def test_bit_identical_repeats_null_classes_and_graph_capture(mm, wl, torch, unrounded):
    """A repeated call returns the same bits; path and score do not depend on `classes` being asked for; one capture after a first
    call replays the bits, and a replay after U was overwritten in place follows the new scores."""
    lib = _lib(mm)
    g, f, twin, V, lens = unrounded
    B, N, P = V.shape
    cls, nc = layout(g, f, twin, "dst")
    bf = _batch(mm, [f] * B, [g] * B)
    bf.set_path_classes(cls, nc)
    U0, U1 = scores(5, B, N, nc), scores(6, B, N, nc)
    Vt, lt, Ut = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(U0).cuda()
    run = lambda: bf.classpath(Vt, Ut, lt)
    out0, out1 = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    path = torch.full((B, N), 7, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 7.0, device="cuda")
    rc = lib.mm_classpath_f32(bf._h, Vt.data_ptr(), N * P, P, lt.data_ptr(), N, Ut.data_ptr(), *Ut.stride(), path.data_ptr(), N, None, 0,
                              score.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(path, out0[0]) and torch.equal(score, out0[2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = run()
    for Un in (U0, U1, U0):
        Ut.copy_(torch.from_numpy(Un).cuda())
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _check([t.cpu().numpy() for t in out2], references(f, g, cls, nc, Un, V, lens), "replay")
    assert not torch.equal(out2[0], bf.classpath(Vt, torch.from_numpy(U1).cuda(), lt)[0])  # (the two score sets give different paths)


def test_capture_before_a_first_call_is_refused(mm, wl, torch, base):
    """Neither the item forms, the planes nor the workspace are made during a capture."""
    g, f, twin, V, lens = base
    fresh = _batch(mm, [f] * 3, [g] * 3)
    cls, nc = layout(g, f, twin, "marks")
    fresh.set_path_classes(cls, nc)
    Vt = torch.from_numpy(V[:3]).cuda()
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.classpath(Vt, None, None)
    assert ei.value.code == -1, str(ei.value)
    # ... and the batch works afterwards
    _check(fresh.classpath(V[:3], None, None), references(f, g, cls, nc, None, V[:3], np.full(3, V.shape[1])), "after the refused capture")


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    path = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    classes = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    score = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ft = wl.to_fsm(mm, g, semiring="tropical")
    nc = 3
    U = torch.zeros((B, N, nc), device="cuda")
    ids = (np.arange(ft.nnz) % nc).astype(np.int32)

    def call(h, path_ptr=path.data_ptr(), psb=N, cls_ptr=classes.data_ptr(), csb=N, u_ptr=U.data_ptr(), us=(N * nc, nc, 1)):
        return lib.mm_classpath_f32(h, V.data_ptr(), N * P, P, None, N, u_ptr, *us, path_ptr, psb, cls_ptr, csb, score.data_ptr(), st)

    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h) == -4 and b"tropical" in lib.mm_last_error()
    assert lib.mm_batch_set_path_classes(lb._h, ids.ctypes.data, None, nc) == -4
    assert lib.mm_batch_path_class_info(lb._h, None, None) == -4
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h) == -4
    tb = _batch(mm, [ft] * B, [g] * B)
    # the arc-class setter still refuses the tropical batch
    assert lib.mm_batch_set_arc_classes(tb._h, ids.ctypes.data, None, nc) == -4
    # no plan: U or classes asked for are refused, neither runs
    assert call(tb._h) == -1 and b"no classes set" in lib.mm_last_error()
    assert call(tb._h, u_ptr=None) == -1 and call(tb._h, cls_ptr=None) == -1
    assert call(tb._h, u_ptr=None, cls_ptr=None) == 0
    # the setter's own refusals
    assert lib.mm_batch_set_path_classes(tb._h, None, None, nc) == -1
    assert lib.mm_batch_set_path_classes(tb._h, ids.ctypes.data, None, 0) == -1
    assert lib.mm_batch_set_path_classes(tb._h, ids.ctypes.data, None, 2) == -1  # (an id outside [-1, C))
    assert lib.mm_batch_set_path_classes(tb._h, ids.ctypes.data, None, 65535) == -4
    offs = np.array([0, ft.nnz, 2 * ft.nnz - 1], dtype=np.int64)
    assert lib.mm_batch_set_path_classes(tb._h, np.concatenate([ids, ids]).ctypes.data, offs.ctypes.data, nc) == -2
    assert tb.path_class_info()["path_C"] == 0
    assert lib.mm_batch_set_path_classes(tb._h, ids.ctypes.data, None, nc) == 0 and tb.path_class_info()["path_C"] == nc
    assert call(tb._h, path_ptr=None) == -1
    assert call(tb._h, psb=N - 1) == -2 and call(tb._h, csb=N - 1) == -2
    assert call(tb._h, us=(N * nc - 1, nc, 1)) == -2 and call(tb._h, us=(N * nc, nc - 1, 1)) == -2
    assert call(tb._h) == 0
    torch.cuda.synchronize()
    with pytest.raises(mm.DimensionMismatch):
        tb.classpath(V, torch.zeros((B, N, nc + 1), device="cuda"), None)
    for b in (lb, pb):
        with pytest.raises(mm.MarkovModelsAMDError):
            b.kernels("classpath")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.classpath(V, None, None)


def test_forced_alignment_end_to_end(mm, wl, torch):
    """A left-to-right HMM of 5 states over 12 frames; classes: the forward arc into state s = s, the final arc = 5, the loop of
    state s = 6 + s.  Two marks pin the arcs into states 2 and 4; the path meets them, and is the restatement's under the marks'
    0 / -inf scores."""
    g = wl.l2r_hmm(5)
    f = wl.to_fsm(mm, g, semiring="tropical")
    i, j, _ = ar.fsm_entries(f)
    cls = np.where(i == j, 6 + i, j).astype(np.int32)
    cls[(i == 5) & (j == 5)] = -1
    nc, N = 11, 12
    V = (2.0 * np.random.default_rng(3).standard_normal((2, N, g.P))).astype(np.float32)
    lens = np.array([12, 10], dtype=np.int32)
    bf = _batch(mm, [f, f], [g, g])
    bf.set_path_classes(cls, nc)
    marks = [[(3, 2), (8, 4)], [(6, 3)]]
    path, classes, score = mm.decode.forced_alignment(bf, V, marks, lens)
    U = np.zeros((2, N, nc), dtype=np.float32)
    U[0, 3], U[0, 8], U[1, 6] = -np.inf, -np.inf, -np.inf
    U[0, 3, 2], U[0, 8, 4], U[1, 6, 3] = 0, 0, 0
    refs = references(f, g, cls, nc, U, V, lens)
    _check((path, classes, score), refs, "forced alignment")
    assert path[0, 3] == 1 and path[0, 4] == 2 and path[0, 8] == 3 and path[0, 9] == 4 and classes[0, 3] == 2 and classes[0, 8] == 4
    assert path[1, 6] == 2 and path[1, 7] == 3 and classes[1, 6] == 3 and np.isfinite(score).all()
    free = references(f, g, cls, nc, None, V, lens)
    assert not np.array_equal(free[0].path, refs[0].path) and all(fr.score >= r.score for fr, r in zip(free, refs))
    ev = mm.decode.events(classes, lens, ignore=(-1, 6, 7, 8, 9, 10))
    assert [c for c, _ in ev[0]] == [1, 2, 3, 4, 5] and (2, 3) in ev[0] and (4, 8) in ev[0] and ev[0][-1] == (5, 11)
    # ... and the module-level call shape
    paths, clss, sc = mm.classbestpath(bf, [mm.expand(V[b].T, int(lens[b]), "tropical") for b in range(2)], cls, U, C=nc)
    assert all(np.array_equal(paths[b], refs[b].path[: lens[b]]) and np.array_equal(clss[b], refs[b].classes[: lens[b]]) for b in range(2))
    assert _same_bits(sc, score)
