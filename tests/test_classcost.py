"""Expected arc-class cost and its gradient (mm_classcost_f32) without a GPU: the float64 reference helper against path
enumeration and against central differences, the identities the definition implies (with the expected-cost and the arc-class
references), and the bindings of the new entry."""
import os
import re

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr
import classcost_reference as ccr
import cost_reference as cr
from test_scoredposteriors import _layouts, _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
@pytest.mark.parametrize("L", [4, 3, 0])
def test_reference_against_path_enumeration(mm, wl, which, L):
    """4 states, N = 4, random A, with D and without; parallel entries and the phony loop as the definition has them."""
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N = 4
    rng = np.random.default_rng(30 + L)
    V = rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        A = 2.0 * rng.standard_normal((N, C))
        for D in (None, rng.standard_normal((N, g.P))):
            risk, grad, gamma, z, mass = ccr.reference(g, f, cls, V, A, D, L, N)
            re_, ge, gme, ze = ccr.enumerate_paths(g, f, cls, V, A, D, L, N)
            assert not np.isnan(grad).any() and not np.isnan(gamma).any()
            if not np.isfinite(ze):
                assert np.isneginf(z) and risk == 0 and (grad == 0).all() and (gamma == 0).all()
                continue
            scale = max(1.0, np.abs(A[:L]).sum() + (0.0 if D is None else np.abs(D[:L]).sum()))
            assert np.isclose(z, ze, rtol=1e-10, atol=1e-10), name
            assert abs(risk - re_) <= 1e-10 * scale, (name, risk, re_)
            assert np.abs(grad - ge).max() <= 1e-10 * scale, (name, np.abs(grad - ge).max())
            assert np.abs(gamma - gme).max() <= 1e-10, name
            assert (grad[L:] == 0).all() and (gamma[L:] == 0).all()
            assert mass >= abs(risk) - 1e-9 * scale
            # the bar's own plumbing on a perfect answer (a single path has grad = 0: G_b is the reference's rounding, no bar to speak of)
            if np.abs(grad).max() > 1e-9:
                assert max(ccr.check(re_, ge, ze, (risk, grad, gamma, z, mass), A, D, L, a=1e-9)) <= 1e-3
    if L == 0:
        return
    Vd = V.copy()
    Vd[1, :] = -np.inf  # no accepting path
    cls, C = np.arange(f.nnz), f.nnz
    risk, grad, gamma, z, _ = ccr.reference(g, f, cls, Vd, np.ones((N, C)), None, L, N)
    assert np.isneginf(z) and risk == 0 and (grad == 0).all() and (gamma == 0).all()
    assert np.isneginf(ccr.enumerate_paths(g, f, cls, Vd, np.ones((N, C)), None, L, N)[3])


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_central_differences_of_the_risk(mm, wl, oracle, which):
    """d risk / d V[n, p] = grad[n, p] (and d risk / d D = gamma, d risk / d A[t, c] = xi[c, t] for t < L) in float64."""
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L, h = 6, 5, 1e-6
    rng = np.random.default_rng(6)
    V = rng.standard_normal((N, g.P))
    D = rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        A = rng.standard_normal((N, C))
        risk, grad, gamma, z, _ = ccr.reference(g, f, cls, V, A, D, L, N)
        assert np.isfinite(z)
        for n in range(N):
            for p in range(g.P):
                Vp, Vm = V.copy(), V.copy()
                Vp[n, p] += h
                Vm[n, p] -= h
                d = (ccr.risk_only(g, f, cls, Vp, A, D, L, N) - ccr.risk_only(g, f, cls, Vm, A, D, L, N)) / (2 * h)
                assert abs(d - grad[n, p]) <= 1e-7, (name, n, p, d, grad[n, p])
                Dp, Dm = D.copy(), D.copy()
                Dp[n, p] += h
                Dm[n, p] -= h
                d = (ccr.risk_only(g, f, cls, V, A, Dp, L, N) - ccr.risk_only(g, f, cls, V, A, Dm, L, N)) / (2 * h)
                assert abs(d - gamma[n, p]) <= 1e-7, (name, n, p)
        # the risk is linear in A: one unit on A[t, c] moves it by the arc-class posterior xi[c, t], and by nothing beyond the length
        xi, _, _ = acr.reference(o, oc, g, f, cls, C, V, L, N)
        for t in range(N):
            for c in range(C):
                Ap = A.copy()
                Ap[t, c] += 1.0
                d = ccr.risk_only(g, f, cls, V, Ap, D, L, N) - risk
                if t >= L:
                    assert d == 0, (name, t, c)
                else:
                    assert abs(d - xi[c, t]) <= 1e-10, (name, t, c, d, xi[c, t])


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_zero_class_costs_give_the_expected_cost_reference(mm, wl, oracle, which):
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N = 7
    rng = np.random.default_rng(7)
    V, D = rng.standard_normal((N, g.P)), rng.standard_normal((N, g.P))
    for L in (7, 5, 1):
        want = cr.reference(o, oc, g, f, V, D, L, N)
        for name, cls, C in _layouts(g, f):
            got = ccr.reference(g, f, cls, V, np.zeros((N, C)), D, L, N)
            assert np.isclose(got[3], want[3], rtol=1e-12, atol=1e-12)
            assert abs(got[0] - want[0]) <= 1e-10 and np.abs(got[1] - want[1]).max() <= 1e-10 and np.abs(got[2] - want[2]).max() <= 1e-10, (name, L)


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_source_pdf_classes_give_the_expected_cost_reference(mm, wl, oracle, which):
    """cls[k] = the pdf of the source state, A[t, p] = D'[t, p], D None: the arc leaving frame t + 1 pays what the frame's pdf would."""
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    i, _, _ = ar.fsm_entries(f)
    cls = ar._s2p_full(g)[i]
    N = 7
    rng = np.random.default_rng(8)
    V, Dp = rng.standard_normal((N, g.P)), rng.standard_normal((N, g.P))
    for L in (7, 5, 1):
        A = np.concatenate([Dp, np.full((N, 1), 123.0)], axis=1)  # (class P: the phony state's entries -- the self-loop alone, which costs 0)
        want = cr.reference(o, oc, g, f, V, Dp, L, N)
        got = ccr.reference(g, f, cls, V, A, None, L, N)
        assert np.isclose(got[3], want[3], rtol=1e-12, atol=1e-12)
        assert abs(got[0] - want[0]) <= 1e-10 and np.abs(got[1] - want[1]).max() <= 1e-10 and np.abs(got[2] - want[2]).max() <= 1e-10, L


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_risk_is_the_posteriors_times_the_costs(mm, wl, oracle, which):
    """risk = sum gamma D + sum_{t<L} xi A with xi of the arc-class reference; a constant class cost per transition is paid by
    every path; sum_p grad = 0."""
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L = 7, 5
    rng = np.random.default_rng(9)
    V, D = rng.standard_normal((N, g.P)), rng.standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        A = rng.standard_normal((N, C))
        risk, grad, gamma, z, _ = ccr.reference(g, f, cls, V, A, D, L, N)
        xi, zr, _ = acr.reference(o, oc, g, f, cls, C, V, L, N)
        assert np.isclose(z, zr, rtol=1e-12, atol=1e-12)
        want = np.sum(gamma[:L] * D[:L]) + np.sum(xi[:, :L].T * A[:L])
        assert abs(risk - want) <= 1e-10, (name, risk, want)
        assert np.abs(grad.sum(axis=1)).max() <= 1e-10
        if (np.asarray(cls) >= 0).all():
            a_t = rng.standard_normal(N)
            risk, grad, _, _, _ = ccr.reference(g, f, cls, V, np.repeat(a_t[:, None], C, axis=1), None, L, N)
            assert abs(risk - a_t[:L].sum()) <= 1e-10 and np.abs(grad).max() <= 1e-10, name


def test_reference_float32_mode_agrees(mm, wl):
    for which in ("l2r3", "rand4"):
        g = _tiny(wl, which)
        f = wl.to_fsm(mm, g, dtype=np.float64)
        N, L = 7, 6
        rng = np.random.default_rng(10)
        V, D = rng.standard_normal((N, g.P)), rng.standard_normal((N, g.P))
        for name, cls, C in _layouts(g, f):
            A = rng.standard_normal((N, C))
            ref = ccr.reference(g, f, cls, V, A, D, L, N)
            r32 = ccr.reference(g, f, cls, V, A, D, L, N, dtype=np.float32)
            G = np.abs(ref[1]).max()
            assert abs(r32[0] - ref[0]) <= 1e-5 * max(1.0, ref[4]) and np.abs(r32[1] - ref[1]).max() <= 1e-5 * max(G, 1.0), name


def test_the_gradient_bar_is_the_measured_floor():
    """The constant of the gradient's bar against the committed table of tools/measure_classcost_floor.py: no smaller a floor than
    the worst row, no more than its rounding above it, and a = min(10 x, 1e-4)."""
    import json

    table = json.load(open(os.path.join(ROOT, "profiles", "classcost_floor.json")))
    worst = max(r["grad_err_over_G"] for r in table["rows"])
    assert worst == table["worst_grad_err_over_G"] and len(table["rows"]) >= 40
    assert worst <= ccr.GRAD_F32_FLOOR <= 1.01 * worst, (ccr.GRAD_F32_FLOOR, worst)
    assert ccr.GRAD_ABS_A == min(10 * ccr.GRAD_F32_FLOOR, 1e-4) and abs(table["a"] - ccr.GRAD_ABS_A) <= 0.01 * ccr.GRAD_ABS_A


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there."""
    from importlib import import_module

    for s in ("mm_classcost_f32", "mm_batch_cost_class_cap"):
        assert s in mm.SYMBOLS
    lib = import_module(mm.__name__ + "._lib").lib
    assert len(lib.mm_classcost_f32.argtypes) == 21 and len(lib.mm_batch_cost_class_cap.argtypes) == 2
    assert callable(mm.classcost) and hasattr(mm.BatchedFSM, "classcost")
    assert callable(mm.expected_class_cost) and callable(mm.mpe_loss)
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_classcost_f32(" in hdr and "int mm_batch_cost_class_cap(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_classcost_f32, LIB\)", src) and re.search(r"ccall\(\(:mm_batch_cost_class_cap, LIB\)", src)
    assert re.search(r"function classcost\(", src) and re.search(r"function cost_class_cap\(", src)
