"""Posteriors with per-frame arc-class scores without a GPU: the float64 reference helper against path enumeration, against the
arc-class and the weighted references where the definition says they coincide, central differences of log Z in U and V against
xi and gamma, the two host helpers, and the bindings of the new entry."""
import os
import re

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr
import scored_reference as sr
import weighted_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(wl, which):
    return wl.l2r_hmm(3) if which == "l2r3" else wl.random_fsm(4, 3, mean_deg=2.0, seed=9)


def _layouts(g, f):
    """(name, cls, C): one class per entry, the source state's pdf, the destination's pdf, a sparse layout with an empty class."""
    i, j, _ = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    sparse = np.full(f.nnz, -1)
    sparse[::2] = 0
    sparse[1::4] = 2
    return [("entry", np.arange(f.nnz), f.nnz), ("src", s2p[i], g.P + 1), ("dst", s2p[j], g.P + 1), ("sparse", sparse, 3)]


def _scores(rng, N, C, ninf=3):
    U = rng.standard_normal((N, C))
    for _ in range(ninf):
        U[rng.integers(N), rng.integers(C)] = -np.inf
    return U


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
@pytest.mark.parametrize("L", [4, 3, 0])
def test_reference_against_path_enumeration(mm, wl, which, L):
    """4 states, N = 4, random U with -inf entries."""
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N = 4
    rng = np.random.default_rng(20 + L)
    V = rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        U = _scores(rng, N, C)
        gamma, xi, z, exact = sr.reference(g, f, cls, C, U, V, L, N)
        ge, xe, ze = sr.enumerate_paths(g, f, cls, C, U, V, L, N)
        assert not np.isnan(gamma).any() and not np.isnan(xi).any()
        if not np.isfinite(ze):
            assert np.isneginf(z) and (xi == 0).all() and (gamma == 0).all() and exact.all()
            continue
        assert np.isclose(z, ze, rtol=1e-10, atol=1e-10), name
        assert np.allclose(xi, xe, rtol=1e-9, atol=1e-12), name
        assert np.allclose(gamma, ge, rtol=1e-9, atol=1e-12), name
        assert np.allclose(xi[exact], xe[exact], atol=1e-15)
        assert (gamma[L:] == 0).all()
        assert acr.check(xi, z, xe, ze) <= 1e-3  # (the bar's own plumbing on a perfect answer; the enumeration's 1.0 is a rounded sum)
    if L == 0:
        return
    # a frame whose every class is blocked leaves no path
    cls, C = np.arange(f.nnz), f.nnz
    U = np.zeros((N, C))
    U[1] = -np.inf
    gamma, xi, z, exact = sr.reference(g, f, cls, C, U, V, L, N)
    assert np.isneginf(z) and (xi == 0).all() and (gamma == 0).all() and exact.all()
    assert np.isneginf(sr.enumerate_paths(g, f, cls, C, U, V, L, N)[2])


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_reference_at_zero_scores_is_the_arcclass_reference(mm, wl, oracle, which):
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N = 7
    V = np.random.default_rng(3).standard_normal((N, g.P))
    for L in (7, 5, 3):
        for name, cls, C in _layouts(g, f):
            xr, zr, er, gr = acr.reference(o, oc, g, f, cls, C, V, L, N, want_gamma=True)
            for U in (None, np.zeros((N, C))):
                gamma, xi, z, exact = sr.reference(g, f, cls, C, U, V, L, N)
                assert np.isclose(z, zr, rtol=1e-12, atol=1e-12) and (exact == er).all()
                assert np.allclose(xi, xr, rtol=1e-9, atol=1e-13), (name, L)
                assert np.allclose(gamma[:L], gr[: g.P, :L].T, rtol=1e-9, atol=1e-13), (name, L)


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_reference_at_constant_scores_is_the_weighted_reference(mm, wl, which):
    """U[t, c] = u_c: the result of the weighted reference with W[k] = w_k + u_{cls[k]} (the phony self-loop stays one(K))."""
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    i, j, w = ar.fsm_entries(f)
    N, L = 6, 5
    rng = np.random.default_rng(4)
    V = rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        cls = np.asarray(cls)
        u = rng.standard_normal(C)
        W = w + np.where(cls >= 0, u[np.maximum(cls, 0)], 0.0)
        gw, cw, _, zw = wr.reference(f, g.state2pdf, g.P, V, L, N, W=W)
        gamma, xi, z, _ = sr.reference(g, f, cls, C, np.tile(u, (N, 1)), V, L, N)
        assert np.isclose(z, zw, rtol=1e-12, atol=1e-12), name
        assert np.allclose(gamma, gw, rtol=1e-9, atol=1e-13), name
        by_class = np.zeros(C)
        fs = f.colptr.size - 2
        real = (cls >= 0) & ~((i == fs) & (j == fs))  # (the loop's count holds the N - L frames behind the utterance)
        np.add.at(by_class, cls[real], cw[real])
        assert np.allclose(xi[:, :L].sum(axis=1), by_class, rtol=1e-9, atol=1e-12), name


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_central_differences_of_log_z(mm, wl, which):
    """d log Z / d U[t, c] = xi[c, t] for t < L, d log Z / d V[n, p] = gamma[n, p]."""
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L, h = 6, 5, 1e-5
    rng = np.random.default_rng(5)
    V = rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        U = rng.standard_normal((N, C))
        gamma, xi, z, _ = sr.reference(g, f, cls, C, U, V, L, N)
        assert np.isfinite(z)
        for t in range(N):
            for c in range(C):
                Up, Um = U.copy(), U.copy()
                Up[t, c] += h
                Um[t, c] -= h
                d = (sr.log_z(g, f, cls, Up, V, L, N) - sr.log_z(g, f, cls, Um, V, L, N)) / (2 * h)
                want = xi[c, t] if t < L else 0.0  # (rows t >= L are not part of Z)
                assert abs(d - want) <= 1e-8, (name, t, c, d, want)
        for n in range(N):
            for p in range(g.P):
                Vp, Vm = V.copy(), V.copy()
                Vp[n, p] += h
                Vm[n, p] -= h
                d = (sr.log_z(g, f, cls, U, Vp, L, N) - sr.log_z(g, f, cls, U, Vm, L, N)) / (2 * h)
                assert abs(d - gamma[n, p]) <= 1e-8, (name, n, p, d, gamma[n, p])


def _hand_made(mm):
    """Four states with pdfs 0, 1, 1, 2: self-loops on 0, 1 and 3, a chain 0 -> 1 -> 2 -> 3, a skip 0 -> 2; 2 and 3 are final."""
    arcs = [((0, 0), -0.5), ((0, 1), -1.0), ((1, 1), -0.3), ((1, 2), -0.7), ((2, 3), -0.9), ((3, 3), -0.2), ((0, 2), -1.1)]
    return mm.FSM([(0, 0.0)], arcs, [(2, -0.4), (3, -0.6)], list("abcd")), np.array([0, 1, 1, 2])


def test_loop_exit_classes_on_a_hand_made_graph(mm):
    f, s2p = _hand_made(mm)
    i, j, _ = ar.fsm_entries(f)
    cls, C = mm.loop_exit_classes(f, s2p, 3)
    assert C == 6 and cls.dtype == np.int32 and cls.shape == (f.nnz,)
    S = 4
    for k in range(f.nnz):
        if i[k] == S:
            assert j[k] == S and cls[k] == -1  # the phony self-loop
        elif i[k] == j[k]:
            assert cls[k] == 2 * s2p[i[k]]
        else:
            assert cls[k] == 2 * s2p[i[k]] + 1  # every other entry that leaves a real state, the final arcs included
    assert (cls[(j == S) & (i < S)] % 2 == 1).all() and ((j == S) & (i < S)).sum() == 2
    assert sorted(cls[cls >= 0].tolist()) == sorted([0, 1, 2, 3, 3, 4, 1, 3, 5])
    assert (mm.loop_exit_classes(f, np.concatenate([s2p, [3]]), 3)[0] == cls).all()  # a pdf for the phony state changes nothing
    with pytest.raises(ValueError):
        mm.loop_exit_classes(f, s2p[:2], 3)
    with pytest.raises(ValueError):
        mm.loop_exit_classes(f, s2p, 2)  # pdf 2 is outside [0, 2)


def test_constraint_scores(mm):
    from importlib import import_module

    allowed = np.zeros((2, 3, 4), dtype=bool)
    allowed[0, 1, 2] = allowed[1, 0, 0] = True
    s = mm.constraint_scores(allowed)
    assert s.dtype == np.float32 and s.shape == allowed.shape
    assert (s[allowed] == 0).all() and np.isneginf(s[~allowed]).all()
    torch = import_module("torch")
    st = mm.constraint_scores(torch.from_numpy(allowed))
    assert st.dtype == torch.float32 and (st.numpy() == s).all()
    with pytest.raises(TypeError):
        mm.constraint_scores(allowed.astype(np.int32))
    with pytest.raises(TypeError):
        mm.constraint_scores(torch.zeros(2, 3, 4))


def test_entry_is_bound(mm):
    assert callable(mm.scoredposteriors) and hasattr(mm.BatchedFSM, "scoredposteriors") and callable(mm.transition_loglik)
    assert callable(mm.loop_exit_classes) and callable(mm.constraint_scores) and mm.transitions.transition_loglik is mm.transition_loglik
    for s in ("mm_scoredposteriors_f32", "mm_batch_score_class_cap"):
        assert s in mm.SYMBOLS
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert len(lib.mm_scoredposteriors_f32.argtypes) == 20 and len(lib.mm_batch_score_class_cap.argtypes) == 2
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_scoredposteriors_f32(" in hdr and "int mm_batch_score_class_cap(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_scoredposteriors_f32, LIB\)", src) and re.search(r"ccall\(\(:mm_batch_score_class_cap, LIB\)", src)
    assert re.search(r"function scoredposteriors\(", src)
