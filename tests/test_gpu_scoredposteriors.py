"""Posteriors with per-frame arc-class scores (mm_scoredposteriors_f32) on the MI355X against the float64 reference of
tests/scored_reference.py: xi and ttl by the bar of arcclass_reference.check, gamma by check_gamma of test_gpu_parity.  Every
instance, both placements of the term rows, the class cap, the identities with the arc-class, pdf and weighted posteriors of the
same batch, constraints, and the properties of the entry: bit-identical repeats, optional outputs, strides, hipGraph capture,
relabelling, error codes; transition_loglik's gradients.  Every test asserts by name, from kernels("scored"), the instance and the
term-row placement it claims to run, and prints its worst error over the bar.  U is N(0, 1) with a few -inf entries unless a
case says otherwise."""
import ctypes as C
import re

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr
import scored_reference as sr
from test_gpu_arcclassposteriors import STREAMED, _batch, _dst_pdf, _lib, _sparse, _src_pdf
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _is(bf, NI, where, terms):
    k = bf.kernels("scored")
    assert f"mm_scored_fwd_kernel<{NI},{where}>" in k and f"mm_scored_bwd_kernel<{NI},{where}>" in k, k
    assert k.endswith("terms in LDS" if terms == "lds" else "terms in global memory"), k
    return k


def _term_cap(bf):
    return int(re.search(r"term cap (\d+)", bf.kernels("scored")).group(1))


def _scores(seed, B, N, nc, ninf=4):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((B, N, nc)).astype(np.float32)
    for _ in range(ninf):
        U[rng.integers(B), rng.integers(N), rng.integers(nc)] = -np.inf
    return U


def _check(gs, fs, clss, nc, U, V, lens, gamma, xi, ttl, idx=None, what=""):
    """Every utterance (or those of idx) against the float64 reference: returns the worst error over the bars."""
    N = V.shape[1]
    idx = list(range(len(gs)) if idx is None else idx)
    worst = 0.0
    gref = np.zeros((len(idx), N, V.shape[2]))
    alive = []
    for q, b in enumerate(idx):
        g_ref, x_ref, z, exact = sr.reference(gs[b], fs[b], clss[b], nc, None if U is None else U[b].astype(np.float64), V[b].astype(np.float64),
                                              int(lens[b]), N)
        gref[q] = g_ref
        w = acr.check(xi[b], ttl[b], x_ref, z, exact)
        print(f"{what} utterance {b}: len {int(lens[b])}, log Z {z:.6g}, worst xi error / bar {w:.3g}")
        worst = max(worst, w)
        if np.isfinite(z):
            alive.append(q)
        else:
            assert (gamma[b] == 0).all()
    if alive:
        sel = [idx[q] for q in alive]
        w = check_gamma(gamma[sel], gref[alive], [int(lens[b]) for b in sel])
        print(f"{what}: worst gamma error / bar {w:.3g}")
        worst = max(worst, w)
    assert not np.isnan(gamma).any() and not np.isnan(xi).any() and not np.isnan(ttl).any()
    return worst


def _run_shared(mm, wl, g, B, V, lens, layouts, NI, where, terms, seed=40, idx=None, block=None):
    fs, bf = _batch(mm, wl, [g] * B)
    out = {}
    for name, (cls, nc) in layouts.items():
        assert bf.set_arc_classes(cls, nc) == nc
        _is(bf, NI, where, terms)
        U = _scores(seed, B, V.shape[1], nc)
        if block is not None:
            U[block[0], block[1], :] = -np.inf
        gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
        assert xi.shape == (B, nc, V.shape[1]) and gamma.shape == V.shape
        _check([g] * B, fs, [cls] * B, nc, U, V, lens, gamma, xi, ttl, idx, name)
        out[name] = (gamma, xi, ttl)
    return fs[0], bf, out


def test_random_graph_lengths_no_path_and_a_blocked_frame(mm, wl, torch):
    """<8,lds>, terms in LDS.  The inputs of the arc-class test (a frame of V with -inf entries, an utterance of one frame, one of
    none, one without a path) and a sixth utterance whose scores block every class at transition 7; one class per entry, the
    destination's pdf, a sparse layout with an empty class."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    f = wl.to_fsm(mm, g)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2, N], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((6, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf
    V[4, 4, :] = -np.inf
    layouts = {"entry": (np.arange(f.nnz, dtype=np.int32), f.nnz), "dst": _dst_pdf(g, f), "sparse": _sparse(f)}
    _, bf, out = _run_shared(mm, wl, g, 6, V, lens, layouts, 8, "lds", "lds", block=(5, 7))
    for name, (gamma, xi, ttl) in out.items():
        assert np.isneginf(ttl[3]) and np.isneginf(ttl[4]) and (xi[3] == 0).all() and (xi[4] == 0).all()
        assert (gamma[3] == 0).all() and (gamma[4] == 0).all()
        if name != "sparse":  # every entry has a class: no path survives the blocked transition
            assert np.isneginf(ttl[5]) and (xi[5] == 0).all() and (gamma[5] == 0).all()
        else:
            assert np.isfinite(ttl[5])
    xi = out["dst"][1]
    assert np.isfinite(out["dst"][2][2]), "the scores of the one-frame utterance must leave it a path"
    assert (xi[2, g.P, 1:] == 1).all() and (xi[2, : g.P, 1:] == 0).all()  # behind one frame: the phony loop alone
    assert (out["sparse"][1][:, 1] == 0).all()  # the empty class


def _case_instances(wl, which):
    if which == "streamed":
        return wl.lfmmi_denominator(600, 40, seed=5), 30, np.array([30, 19], dtype=np.int32), STREAMED, (0, "global", "lds")
    if which == "bigv":  # (53 608 entries, all with a class: beyond every term cap)
        return wl.random_fsm(12500, 40, 3.0, seed=3), 40, np.array([40, 29], dtype=np.int32), {}, (8, "global", "global")
    from test_gpu_itemform import case_wide

    gs, V, _, lens, _ = case_wide(wl, "wide")
    return gs[0], V.shape[1], lens, STREAMED, (0, "global", "lds")


@pytest.mark.parametrize("which", ["streamed", "bigv", "wide"])
def test_instances(mm, wl, torch, which):
    """<0,global> on the denominator graph and on rows of hundreds of arcs (long streamed rows), <8,global> on a graph whose
    vectors do not fit the LDS."""
    g, N, lens, env, (NI, where, terms) = _case_instances(wl, which)
    f = wl.to_fsm(mm, g)
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    layouts = {"dst": _dst_pdf(g, f)} if which != "streamed" else {"dst": _dst_pdf(g, f), "sparse": _sparse(f)}
    _with_env(env, lambda: _run_shared(mm, wl, g, 2, V, lens, layouts, NI, where, terms))


def test_wide_rows_resident(mm, wl, torch):
    """case_wide(wl, "wide") on the default instance: <8,lds> with its long rows streamed beside the class plane."""
    from test_gpu_itemform import case_wide

    gs, V, _, lens, _ = case_wide(wl, "wide")
    f = wl.to_fsm(mm, gs[0])
    _run_shared(mm, wl, gs[0], 2, V, lens, {"dst": _dst_pdf(gs[0], f)}, 8, "lds", "lds")


@pytest.mark.parametrize("over", [0, 1])
def test_term_row_placement(mm, wl, torch, over):
    """Exactly cap and cap + 1 classified entries (the term cap of the plan's 5 classes, from kernels("scored")), spread over the
    classes by entry index: terms in LDS, terms in global memory.  The construction of the arc-class test on the same graph."""
    g = wl.lfmmi_denominator(1200, 40)
    fs, bf = _batch(mm, wl, [g, g])
    f = fs[0]
    bf.set_arc_classes(np.zeros(f.nnz, dtype=np.int32), 5)  # (the term cap depends on the number of classes alone)
    cap = _term_cap(bf)
    assert 0 < cap + 1 <= f.nnz, (cap, f.nnz)
    M = cap + over
    cls = np.full(f.nnz, -1, dtype=np.int32)
    pick = np.round(np.linspace(0, f.nnz - 1, M)).astype(np.int64)  # M distinct entries over the whole graph
    assert np.unique(pick).size == M
    cls[pick] = pick % 5
    N = 20
    V = np.random.default_rng(8).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([20, 13], dtype=np.int32)
    bf.set_arc_classes(cls, 5)
    assert bf.info()["arcclass_max_M"] == M and _term_cap(bf) == cap
    _is(bf, 8, "lds", "global" if over else "lds")
    U = _scores(9, 2, N, 5)
    gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
    _check([g, g], fs, [cls, cls], 5, U, V, lens, gamma, xi, ttl, None, "cap + 1" if over else "cap")


def test_class_cap(mm, wl, torch):
    """C = cap classes (most of them empty) run and are checked; C = cap + 1 is refused with the cap in the message."""
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    fs, bf = _batch(mm, wl, [g, g])
    f = fs[0]
    cap = bf.info(scored=True)["score_class_cap"]
    assert f.nnz < cap <= 65534, cap
    cls = ((np.arange(f.nnz) * 7919) % cap).astype(np.int32)
    cls[::9] = -1
    cls[3] = cap - 1
    N = 10
    V = np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([10, 6], dtype=np.int32)
    assert bf.set_arc_classes(cls, cap) == cap
    _is(bf, 8, "lds", "global")  # (the score rows of cap classes leave the term rows no LDS)
    U = _scores(3, 2, N, cap, ninf=50)
    gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
    _check([g, g], fs, [cls, cls], cap, U, V, lens, gamma, xi, ttl, None, "C = cap")
    bf.set_arc_classes(cls, cap + 1)
    assert "exceed the cap" in bf.kernels("scored")
    with pytest.raises(mm.MarkovModelsAMDError) as e:
        bf.scoredposteriors(V, None, lens)
    assert e.value.code == -4 and str(cap) in str(e.value)
    x2, _ = bf.arcclassposteriors(V, lens)  # (the arc-class entry has no such cap)
    assert x2.shape == (2, cap + 1, N)


def test_distinct_graphs_with_their_own_classes(mm, wl, torch):
    """The four graphs of the arc-class test, a layout of 6 classes each."""
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    fs, bf = _batch(mm, wl, gs)
    sp = _sparse(fs[2])[0]
    sp[3::5] = 5
    d3 = _dst_pdf(gs[3], fs[3])[0].copy()
    d3[::3] = -1
    clss = [_dst_pdf(gs[0], fs[0])[0], _src_pdf(gs[1], fs[1])[0], sp, d3]
    assert bf.set_arc_classes(clss, 6) == 6
    _is(bf, 8, "lds", "lds")
    U = _scores(6, 4, N, 6, ninf=3)
    gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
    _check(gs, fs, clss, 6, U, V, lens, gamma, xi, ttl)


def test_csr_layout_with_scrambled_entries(mm, wl, torch):
    """An FSM handed over as CSR(T_hat) with the entries of every row in a scrambled order: the classes follow the caller's entry
    order into both class planes.  Through the C ABI, xi laid out [B, C, N] by its strides."""
    lib = _lib(mm)
    g = wl.random_fsm(50, 4, 3.0, seed=9)
    f = wl.to_fsm(mm, g)
    i, j, w = ar.fsm_entries(f)
    order = np.lexsort((np.random.default_rng(1).random(i.size), i))
    S1 = f.colptr.size - 1
    ptr = np.zeros(S1 + 1, dtype=np.int64)
    np.add.at(ptr, i + 1, 1)
    ptr = np.cumsum(ptr)
    idx = np.ascontiguousarray(j[order], dtype=np.int64)
    val = np.ascontiguousarray(w[order], dtype=np.float32)
    aidx = np.ascontiguousarray(f.alpha_idx, dtype=np.int64)
    aval = np.ascontiguousarray(f.alpha_val, dtype=np.float32)
    s2p = np.ascontiguousarray(list(g.state2pdf) + [g.P], dtype=np.int32)
    h, bh = C.c_void_p(), C.c_void_p()
    assert lib.mm_fsm_create(0, S1, i.size, 1, 8, 0, 4, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, aidx.size,
                             aidx.ctypes.data, aval.ctypes.data, s2p.ctypes.data, g.P + 1, C.byref(h)) == 0
    assert lib.mm_batch_create((C.c_void_p * 2)(h, h), 2, C.byref(bh)) == 0
    try:
        nc = 7
        cls_csc = (np.arange(i.size) % (nc + 1) - 1).astype(np.int32)  # in f's CSC order; -1 for every 8th entry
        cls_caller = np.ascontiguousarray(cls_csc[order])
        assert lib.mm_batch_set_arc_classes(bh, cls_caller.ctypes.data, None, nc) == 0, lib.mm_last_error()
        N = 25
        Vn = np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)
        Un = _scores(3, 2, N, nc)
        V, U = torch.from_numpy(Vn).cuda(), torch.from_numpy(Un).cuda()
        lens = torch.tensor([25, 19], dtype=torch.int32, device="cuda")
        xi = torch.full((2, nc, N), -7.0, device="cuda")
        gamma = torch.full((2, N, g.P), -7.0, device="cuda")
        ttl = torch.empty(2, device="cuda")
        rc = lib.mm_scoredposteriors_f32(bh, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, U.data_ptr(), *U.stride(),
                                         gamma.data_ptr(), *gamma.stride(), xi.data_ptr(), xi.stride(0), xi.stride(2), xi.stride(1),
                                         ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.mm_last_error()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1024)
        assert lib.mm_batch_kernels(bh, 15, buf, 1024) == 0
        k = buf.value.decode()
        assert "mm_scored_fwd_kernel<8,lds>" in k and "mm_scored_bwd_kernel<8,lds>" in k and k.endswith("terms in LDS"), k
        _check([g, g], [f, f], [cls_csc, cls_csc], nc, Un, Vn, np.array([25, 19]), gamma.cpu().numpy(), xi.cpu().numpy(), ttl.cpu().numpy(),
               None, "scrambled CSR")
    finally:
        lib.mm_batch_destroy(bh)
        lib.mm_fsm_destroy(h)


def test_identities_with_the_other_entries(mm, wl, torch):
    """lfmmi_denominator(600, 40, seed=5), B = 6, N = 120, destination-pdf classes (every entry has one).  Two results of this
    library that each meet a bar against the exact value differ by at most twice that bar: xi by 2 (1e-4 xi + 1e-6)
    (arcclass_reference.check), gamma by 2 * 2e-5 (check_gamma), the counts by 2 (1e-4 c + 1e-6 len) (arc_reference.check); ttl
    as those checks compare it."""
    g = wl.lfmmi_denominator(600, 40, seed=5)
    B, N, P = 6, 120, g.P
    fs, bf = _batch(mm, wl, [g] * B)
    f = fs[0]
    V = np.random.default_rng(6).standard_normal((B, N, P)).astype(np.float32)
    lens = np.array([120, 100, 90, 120, 7, 64], dtype=np.int32)
    cls, nc = _dst_pdf(g, f)
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds", "lds")
    xa, ta = bf.arcclassposteriors(V, lens)
    ga, tg = bf.pdfposteriors(V, lens)
    g0, x0, t0 = bf.scoredposteriors(V, None, lens)
    g1, x1, t1 = bf.scoredposteriors(V, np.zeros((B, N, nc), dtype=np.float32), lens)
    assert (g0 == g1).all() and (x0 == x1).all() and (t0 == t1).all()  # no scores and zero scores: the same arithmetic
    ex, eg = np.abs(x0.astype(np.float64) - xa), np.abs(g0.astype(np.float64) - ga)
    print(f"U NULL: xi against arcclassposteriors worst / bar {(ex / (2 * (1e-4 * xa + 1e-6))).max():.3g}, gamma against pdfposteriors {eg.max() / 4e-5:.3g}")
    assert (ex <= 2 * (1e-4 * xa + 1e-6)).all() and eg.max() <= 4e-5
    assert np.allclose(t0, ta, rtol=1e-5, atol=1e-4) and np.allclose(t0, tg, rtol=1e-5, atol=1e-4)
    for b in range(B):
        assert (x0[b, nc - 1, lens[b] :] == 1).all() and (x0[b, : nc - 1, lens[b] :] == 0).all() and (g0[b, lens[b] :] == 0).all()
    # every entry has a class: the classes of a frame add up to 1
    fsum = np.abs(x0.astype(np.float64).sum(axis=1) - 1.0)
    print(f"sum over the classes - 1: worst {fsum.max():.3g} (bar 1e-4)")
    assert (fsum <= 1e-4).all()
    # scores constant in t: the weighted posteriors with W = w + u[cls]
    u = np.random.default_rng(7).standard_normal(nc).astype(np.float32)
    W = (np.asarray(f.nzval, dtype=np.float32) + u[cls]).astype(np.float32)
    gw, cw, tw = bf.weightedposteriors(V, torch.from_numpy(W).cuda(), None, lens)
    gu, xu, tu = bf.scoredposteriors(V, np.broadcast_to(u, (B, N, nc)).copy(), lens)
    assert np.allclose(tu, tw, rtol=1e-5, atol=1e-4)
    eg = np.abs(gu.astype(np.float64) - gw)
    worst = eg.max() / 4e-5
    assert eg.max() <= 4e-5
    for b in range(B):
        by_class = np.zeros(nc)
        np.add.at(by_class, cls, cw[b, : f.nnz].astype(np.float64))
        err, bar = np.abs(xu[b].astype(np.float64).sum(axis=1) - by_class), 2 * (1e-4 * by_class + 1e-6 * int(lens[b]))
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (b, err.max())
    print(f"U constant in t against weightedposteriors: worst / bar {worst:.3g}")


def test_constraint_forces_one_alignment(mm, wl, torch):
    """l2r_hmm(5) with loop_exit_classes: every exit is forbidden except at one chosen transition per state.  One path is left:
    gamma is its one-hot alignment and ttl its score."""
    g = wl.l2r_hmm(5)
    fs, bf = _batch(mm, wl, [g, g])
    f = fs[0]
    cls, nc = mm.loop_exit_classes(f, g.state2pdf, g.P)
    assert nc == 10
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds", "lds")
    N = 14
    lens = np.array([14, 12], dtype=np.int32)
    exits = [np.array([2, 4, 7, 8, 13]), np.array([0, 1, 6, 10, 11])]  # the transition at which state s is left (the last: into the final state)
    allowed = np.ones((2, N, nc), dtype=bool)
    allowed[:, :, 1::2] = False
    for b in range(2):
        allowed[b, exits[b], 2 * np.arange(5) + 1] = True
    U = mm.constraint_scores(allowed)
    V = np.random.default_rng(11).standard_normal((2, N, g.P)).astype(np.float32)
    gamma, xi, ttl = bf.scoredposteriors(V, U, lens)
    i, j, w = ar.fsm_entries(f)
    wt = {(int(a), int(c)): float(x) for a, c, x in zip(i, j, w)}
    a0 = dict(zip(np.asarray(f.alpha_idx).tolist(), np.asarray(f.alpha_val, dtype=np.float64).tolist()))
    for b in range(2):
        L = int(lens[b])
        state = np.searchsorted(exits[b], np.arange(L))  # frame n is in the first state whose exit is at n or later
        onehot = np.zeros((N, g.P))
        onehot[np.arange(L), state] = 1.0
        score = a0[0] + float(V[b, np.arange(L), state].astype(np.float64).sum())
        score += sum(wt[(int(state[n]), int(state[n + 1]))] for n in range(L - 1)) + wt[(4, 5)]
        w_ = check_gamma(gamma[b : b + 1], onehot[None], [L])
        print(f"utterance {b}: forced alignment, gamma worst / bar {w_:.3g}, ttl {ttl[b]:.6g} against {score:.6g}")
        assert np.isclose(ttl[b], score, rtol=1e-5, atol=1e-5 * max(1.0, abs(score)) + 1e-4)
        for s in range(5):  # each exit fires at its transition, with probability 1
            assert abs(xi[b, 2 * s + 1, exits[b][s]] - 1.0) <= 1e-4 and (np.delete(xi[b, 2 * s + 1], exits[b][s]) == 0).all()
    _check([g, g], fs, [cls, cls], nc, U, V, lens, gamma, xi, ttl, None, "constraint")


def test_bit_identical_optional_outputs_strides_capture_and_relabelling(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    fs, bf = _batch(mm, wl, [g] * 6)
    f = fs[0]
    N, B = 120, 6
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((B, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    cls, nc = _dst_pdf(g, f)
    cls = cls.copy()
    cls[::5] = -1
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds", "lds")
    U = torch.from_numpy(_scores(8, B, N, nc)).cuda()
    g0, x0, t0 = bf.scoredposteriors(V, U, lens)
    g1, x1, t1 = bf.scoredposteriors(V, U, lens)
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and torch.equal(x0, x1) and torch.equal(t0, t1)
    assert float(x0.sum()) > 0 and float(g0.sum()) > 0
    # optional outputs: what is left out changes no bit of the rest
    g2, xn, t2 = bf.scoredposteriors(V, U, lens, want_xi=False)
    gn, x2, t3 = bf.scoredposteriors(V, U, lens, want_gamma=False)
    assert xn is None and gn is None and torch.equal(g2, g0) and torch.equal(x2, x0) and torch.equal(t2, t0) and torch.equal(t3, t0)
    lib = _lib(mm)
    t4 = torch.zeros(B, device="cuda")
    rc = lib.mm_scoredposteriors_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, U.data_ptr(), *U.stride(), None, 0, 0, 0,
                                     None, 0, 0, 0, t4.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(t4, t0)
    # gamma with the frames contiguous per pdf (column-major in [N, P])
    out = torch.full((B, g.P, N), -7.0, device="cuda").permute(0, 2, 1)
    g3, _, _ = bf.scoredposteriors(V, U, lens, out=out)
    assert g3.data_ptr() == out.data_ptr() and g3.stride() == (g.P * N, 1, N) and torch.equal(g3, g0)
    # hipGraph capture; a replay follows scores overwritten in place
    Uc = U.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gc, xc, tc = bf.scoredposteriors(V, Uc, lens)
    for _ in range(2):
        gc.zero_()
        xc.zero_()
        tc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gc, g0) and torch.equal(xc, x0) and torch.equal(tc, t0)
    U2 = torch.from_numpy(_scores(9, B, N, nc)).cuda()
    g5, x5, t5 = bf.scoredposteriors(V, U2, lens)
    Uc.copy_(U2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gc, g5) and torch.equal(xc, x5) and torch.equal(tc, t5) and not torch.equal(tc, t0)
    # relabelling: class c becomes perm[c], the columns of U move with the labels; the rows of xi move bit for bit, gamma stays
    perm = np.random.default_rng(1).permutation(nc).astype(np.int32)
    pt = torch.from_numpy(perm.astype(np.int64)).cuda()
    bf.set_arc_classes(np.where(cls >= 0, perm[np.maximum(cls, 0)], -1).astype(np.int32), nc)
    Up = torch.empty_like(U)
    Up[:, :, pt] = U
    g6, x6, t6 = bf.scoredposteriors(V, Up, lens)
    torch.cuda.synchronize()
    assert torch.equal(x6[:, pt, :], x0) and torch.equal(g6, g0) and torch.equal(t6, t0)
    # replacing the plan replaces the planes: two classes, the even and the odd entries
    bf.set_arc_classes((np.arange(f.nnz) % 2).astype(np.int32), 2)
    U7 = torch.from_numpy(_scores(10, B, N, 2, ninf=0)).cuda()
    g7, x7, t7 = bf.scoredposteriors(V, U7, lens)
    torch.cuda.synchronize()
    assert x7.shape == (B, 2, N) and not torch.equal(t7, t0)
    assert torch.allclose(x7.sum(dim=1), torch.ones_like(x7[:, 0]), atol=1e-4)  # every entry has a class: the frames add up to 1
    fs2, bf2 = _batch(mm, wl, [g] * 6)  # a batch that never saw the first plan
    bf2.set_arc_classes((np.arange(f.nnz) % 2).astype(np.int32), 2)
    g8, x8, t8 = bf2.scoredposteriors(V, U7, lens)
    assert torch.equal(g8, g7) and torch.equal(x8, x7) and torch.equal(t8, t7)


def test_transition_loglik_gradients_and_a_step_uphill(mm, wl, torch):
    """grad_V = g gamma, grad_U = g xi with the rows t >= len zeroed, zeros for an utterance without a path and no NaN; one
    gradient step on U raises ttl."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    fs, bf = _batch(mm, wl, [g] * 4)
    f = fs[0]
    cls, nc = mm.loop_exit_classes(f, g.state2pdf, g.P)
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds", "lds")
    N = 24
    Vn = np.random.default_rng(12).standard_normal((4, N, g.P)).astype(np.float32)
    Vn[3, 5, :] = -np.inf  # no path
    lens = torch.tensor([24, 17, 9, 24], dtype=torch.int32, device="cuda")
    V = torch.from_numpy(Vn).cuda().requires_grad_(True)
    U = torch.from_numpy(_scores(13, 4, N, nc, ninf=0)).cuda().requires_grad_(True)
    gout = torch.tensor([1.0, -2.0, 0.5, 3.0], device="cuda")
    ttl = mm.transition_loglik(V, U, bf, lens)
    assert torch.isneginf(ttl[3]) and torch.isfinite(ttl[:3]).all()
    (ttl * gout).sum().backward()  # (utterance 3: a finite factor on ttl = -inf comes down)
    gamma, xi, t0 = bf.scoredposteriors(V.detach(), U.detach(), lens)
    assert torch.equal(t0, ttl.detach())
    live = (torch.arange(N, device="cuda")[None, :] < lens[:, None]).float()
    gz = gout.clone()
    gz[3] = 0.0
    assert torch.equal(V.grad, gamma * gz[:, None, None])
    assert torch.equal(U.grad, xi.permute(0, 2, 1) * gz[:, None, None] * live[:, :, None])
    assert not torch.isnan(V.grad).any() and not torch.isnan(U.grad).any() and (V.grad[3] == 0).all() and (U.grad[3] == 0).all()
    assert (U.grad[1, 17:] == 0).all() and float(U.grad[1, :17].abs().sum()) > 0
    # only what is needed: U alone asks for no gamma
    U2 = U.detach().clone().requires_grad_(True)
    t2 = mm.transition_loglik(V.detach(), U2, bf, lens)
    t2.sum().backward()
    assert torch.equal(U2.grad, xi.permute(0, 2, 1) * torch.tensor([1.0, 1.0, 1.0, 0.0], device="cuda")[:, None, None] * live[:, :, None])
    with torch.no_grad():
        U3 = U2 + 0.5 * U2.grad
    t3 = mm.transition_loglik(V.detach(), U3, bf, lens)
    print("ttl before / after one step on U:", t2[:3].tolist(), t3[:3].tolist())
    assert (t3[:3] > t2[:3]).all()


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N, B, P = 10, 2, g.P
    V = torch.zeros((B, N, P), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = wl.to_fsm(mm, g)
    sm = mm.statemap(g.state2pdf, g.P)
    lb = mm.batch(*([mm.compile(f, sm)] * 2))
    nc = 3
    x = torch.zeros((B, N, nc), device="cuda")
    gm = torch.zeros((B, N, P), device="cuda")
    U = torch.zeros((B, N, nc), device="cuda")
    t = torch.zeros(B, device="cuda")

    def call(bf, us=(N * nc, nc, 1), gp=gm.data_ptr(), gs=(N * P, P, 1), xp=x.data_ptr(), xs=(N * nc, nc, 1), tp=t.data_ptr(), stream=st):
        return lib.mm_scoredposteriors_f32(bf._h, V.data_ptr(), N * P, P, None, N, U.data_ptr(), *us, gp, *gs, xp, *xs, tp, stream)

    assert call(lb) == -1 and b"no classes set" in lib.mm_last_error()
    assert lb.kernels("scored").endswith("no classes set")
    cls = (np.arange(f.nnz) % nc).astype(np.int32)
    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), sm)] * 2))
    assert call(tb) == -4 and b"log" in lib.mm_last_error()
    cap = C.c_int64()
    assert lib.mm_batch_score_class_cap(tb._h, C.byref(cap)) == -4 and lib.mm_batch_score_class_cap(lb._h, None) == -1
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("scored")
    assert lib.mm_batch_set_arc_classes(lb._h, cls.ctypes.data, None, nc) == 0
    assert call(lb, gp=None, xp=None, tp=None) == -1 and b"all NULL" in lib.mm_last_error()
    assert call(lb, us=(N * nc, nc - 1, 1)) == -2 and b"u strides" in lib.mm_last_error()  # frames overlap
    assert call(lb, xs=(N * nc - 1, nc, 1)) == -2 and b"x strides" in lib.mm_last_error()
    assert call(lb, gs=(N * P, P - 1, 1)) == -2 and b"g strides" in lib.mm_last_error()
    with pytest.raises(mm.DimensionMismatch):
        lb.scoredposteriors(V, torch.zeros((B, N, nc + 1), device="cuda"))
    with pytest.raises(TypeError):
        lb.scoredposteriors(V, torch.zeros((B, N, nc), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        lb.scoredposteriors(V, U, want_gamma=False, out=gm)
    # a first call under capture is refused: the planes are not on the device yet
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(lb, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1, rc
    assert call(lb) == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert np.isclose(float(x.sum()), B * N, rtol=1e-4) and np.isclose(float(gm.sum()), B * N, rtol=1e-4)  # every entry has a class
