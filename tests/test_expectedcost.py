"""Expected path cost and its gradient (mm_expectedcost_f32) without a GPU: the bindings of the new entry, the float64 reference
helper against path enumeration and against central differences, and the identities the definition implies."""
import os
import re

import numpy as np
import pytest

import cost_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_expectedcost_f32" in mm.SYMBOLS
    assert lib.mm_expectedcost_f32.argtypes is not None and len(lib.mm_expectedcost_f32.argtypes) == 17
    assert callable(mm.expectedcost) and callable(mm.expected_cost) and callable(mm.smbr_loss)
    assert hasattr(mm.BatchedFSM, "expectedcost")
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_expectedcost_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_expectedcost_f32, LIB\)", src) and re.search(r"function expectedcost\(", src)


def _shared_pdf(wl):
    """Four states on two pdfs: states that share a pdf."""
    g = wl.random_fsm(4, 2, mean_deg=2.5, seed=11)
    assert len(set(g.state2pdf)) < g.S
    return g


def _tiny_cases(wl):
    rng = np.random.default_rng(21)
    out = []
    g = wl.l2r_hmm(3)
    out.append(("l2r3 full length", g, rng.standard_normal((5, g.P)), rng.standard_normal((5, g.P)), 5, 5))
    out.append(("l2r3 short", g, rng.standard_normal((6, g.P)), rng.standard_normal((6, g.P)), 4, 6))
    g = wl.random_fsm(6, 3, mean_deg=2.0, seed=4)
    V = rng.standard_normal((4, g.P))
    V[1, 0] = -np.inf  # a frame with a -inf entry
    out.append(("rand6 -inf entry, signed costs", g, V, 3.0 * rng.standard_normal((4, g.P)), 4, 4))
    out.append(("rand6 short", g, rng.standard_normal((4, g.P)), rng.random((4, g.P)), 3, 4))
    g = _shared_pdf(wl)
    out.append(("two states per pdf", g, rng.standard_normal((5, g.P)), rng.standard_normal((5, g.P)), 5, 5))
    V = rng.standard_normal((4, g.P))
    V[2, :] = -np.inf  # no accepting path
    out.append(("no path", g, V, rng.standard_normal((4, g.P)), 4, 4))
    return out


def test_reference_against_path_enumeration(mm, wl, oracle):
    o, oc = oracle
    seen_no_path = False
    for name, g, V, cost, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        risk, grad, gamma, z = cr.reference(o, oc, g, f, V, cost, L, N)
        risk_e, grad_e, gamma_e, z_e = cr.enumerate_paths(g, f, V, cost, L, N)
        if not np.isfinite(z_e):
            seen_no_path = True
            assert np.isneginf(z) and risk == 0 and (grad == 0).all() and (gamma == 0).all(), name
            continue
        scale = max(1.0, np.abs(cost[:L]).sum())
        assert np.isclose(z, z_e, rtol=1e-10, atol=1e-10), name
        assert abs(risk - risk_e) <= 1e-10 * scale, (name, risk, risk_e)
        assert np.abs(grad - grad_e).max() <= 1e-10 * scale, (name, np.abs(grad - grad_e).max())
        assert np.abs(gamma - gamma_e).max() <= 1e-10, name
        assert (grad[L:] == 0).all() and (gamma[L:] == 0).all(), name
    assert seen_no_path


def test_reference_float32_mode_agrees(mm, wl, oracle):
    """The float32 mode of the reference is the same recursion: on tiny graphs it misses float64 by float32 rounding only."""
    o, oc = oracle
    for name, g, V, cost, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        ref = cr.reference(o, oc, g, f, V, cost, L, N)
        r32 = cr.reference(o, oc, g, f, V, cost, L, N, dtype=np.float32)
        if not np.isfinite(ref[3]):
            continue
        G = np.abs(ref[1]).max()
        assert abs(r32[0] - ref[0]) <= 1e-5 * max(1.0, np.abs(cost[:L]).sum()), name
        assert np.abs(r32[1] - ref[1]).max() <= 1e-5 * max(G, 1.0), name


def test_reference_gradients_against_central_differences(mm, wl, oracle):
    """grad = d risk / d V and gamma = d risk / d cost (eps = 1e-6; the rounding of a risk of a few units over eps is 1e-9)."""
    o, oc = oracle
    eps = 1e-6
    for name, g, V, cost, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        risk, grad, gamma, z = cr.reference(o, oc, g, f, V, cost, L, N)
        if not np.isfinite(z):
            continue
        for n in range(L):
            for p in range(g.P):
                if not np.isfinite(V[n, p]):
                    assert grad[n, p] == 0
                    continue
                d = []
                for sgn in (1.0, -1.0):
                    V2 = V.copy()
                    V2[n, p] += sgn * eps
                    d.append(cr.reference(o, oc, g, f, V2, cost, L, N)[0])
                assert abs((d[0] - d[1]) / (2 * eps) - grad[n, p]) <= 1e-7, (name, n, p)
                d = []
                for sgn in (1.0, -1.0):
                    c2 = cost.copy()
                    c2[n, p] += sgn * eps
                    d.append(cr.reference(o, oc, g, f, V, c2, L, N)[0])
                assert abs((d[0] - d[1]) / (2 * eps) - gamma[n, p]) <= 1e-7, (name, n, p)


def test_identities_on_a_300_state_graph(mm, wl, oracle):
    o, oc = oracle
    g = wl.lfmmi_denominator(300, 40, seed=2)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L = 200, 187
    rng = np.random.default_rng(5)
    V = rng.standard_normal((N, g.P))
    cost = rng.standard_normal((N, g.P))
    risk, grad, gamma, z = cr.reference(o, oc, g, f, V, cost, L, N)
    assert np.isfinite(z)
    assert abs(risk - np.sum(gamma[:L] * cost[:L])) <= 1e-9 * np.abs(cost[:L]).sum()
    assert np.abs(grad.sum(axis=1)).max() <= 1e-10
    assert np.abs(gamma[:L].sum(axis=1) - 1.0).max() <= 1e-10
    # a cost that does not depend on the pdf: every path pays the same
    c = rng.standard_normal(N)
    risk, grad, gamma, z = cr.reference(o, oc, g, f, V, np.repeat(c[:, None], g.P, axis=1), L, N)
    assert abs(risk - c[:L].sum()) <= 1e-9 * np.abs(c[:L]).sum()
    assert np.abs(grad).max() <= 1e-10
