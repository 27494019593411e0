"""Leaky-HMM pdf posteriors (mm_leakyposteriors_f32) without a GPU: the bindings of the new entry, and the float64 reference of
tests/leaky_reference.py -- the rank-one recursion of the header -- against the existing oracle on the explicitly densified
T_eps, against central differences, and against the properties the definition implies."""
import os
import re

import numpy as np

import arc_reference as ar
import graphs
import leaky_reference as lr
from test_gpu_parity import check_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = (0.0, 1e-5, 0.1)


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_leakyposteriors_f32" in mm.SYMBOLS
    assert lib.mm_leakyposteriors_f32.argtypes is not None and len(lib.mm_leakyposteriors_f32.argtypes) == 13
    assert callable(mm.leakyposteriors) and hasattr(mm.BatchedFSM, "leakyposteriors")
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_leakyposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_leakyposteriors_f32, LIB\)", src) and re.search(r"function leakyposteriors\(", src)


def _shared_pdf(wl):
    """Four states on two pdfs: states that share a pdf."""
    g = wl.random_fsm(4, 2, mean_deg=2.5, seed=11)
    assert len(set(g.state2pdf)) < g.S
    return g


def _tiny_cases(wl):
    """(name, graph, V, length, frames)"""
    rng = np.random.default_rng(31)
    out = []
    g = wl.l2r_hmm(3)
    out.append(("l2r3 full length", g, rng.standard_normal((5, g.P)), 5, 5))
    out.append(("l2r3 short", g, rng.standard_normal((6, g.P)), 4, 6))
    g = wl.random_fsm(6, 3, mean_deg=2.0, seed=4)
    V = rng.standard_normal((4, g.P))
    V[1, 0] = -np.inf  # a frame with a -inf entry
    out.append(("rand6 -inf entry", g, V, 4, 4))
    out.append(("rand6 short", g, rng.standard_normal((5, g.P)), 3, 5))
    g = _shared_pdf(wl)
    out.append(("two states per pdf", g, rng.standard_normal((5, g.P)), 5, 5))
    V = rng.standard_normal((4, g.P))
    V[2, :] = -np.inf  # no path, leak or not
    out.append(("no path", g, V, 4, 4))
    return out


def _oracle_posteriors(o, oc, g, V, L, N):
    """gamma [N, P], log Z of a plain FSM from the C oracle in float64."""
    gam, ttl = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, ar.expand_log(V, L, N), dtype=np.float64)
    gam = np.nan_to_num(gam.T.copy(), nan=0.0)
    gam[L:] = 0
    return gam, (float(ttl) if np.isfinite(ttl) else -np.inf)


def test_reference_against_the_oracle_on_the_densified_graph(wl, oracle):
    o, oc = oracle
    seen_no_path = False
    for name, g, V, L, N in _tiny_cases(wl):
        for eps in EPS:
            gam, z = lr.reference(g, V, L, N, eps)
            gam_d, z_d = _oracle_posteriors(o, oc, lr.densify(g, eps), V, L, N)
            if not np.isfinite(z_d):
                assert np.isneginf(z) and (gam == 0).all(), (name, eps)
                seen_no_path = True
                continue
            assert abs(z - z_d) <= 1e-10, (name, eps, z, z_d)
            assert np.abs(gam - gam_d).max() <= 1e-10, (name, eps, np.abs(gam - gam_d).max())
            assert np.allclose(gam[:L].sum(-1), 1.0, atol=1e-12) and (gam[L:] == 0).all()
    assert seen_no_path


def test_densified_graph_against_the_dense_cross_check(wl, oracle):
    """... and the densified matrix through the oracle's independent dense forward-backward (no phony state)."""
    o, _ = oracle
    g = wl.random_fsm(6, 3, mean_deg=2.0, seed=4)
    N = 5
    V = np.random.default_rng(2).standard_normal((N, g.P))
    for eps in EPS:
        d = lr.densify(g, eps)
        f = graphs.to_oracle(o, d)
        Th = np.full((g.S + 1, g.S + 1), -np.inf)
        Th[d.src, d.dst] = d.w
        Th[d.final_idx, g.S] = d.final_w
        post, z_d = o.dense_forward_backward(Th, np.asarray(f.alpha_hat, dtype=np.float64), V.T[np.asarray(g.state2pdf)])
        gam, z = lr.reference(g, V, N, N, eps)
        ref = np.zeros((N, g.P))
        for s in range(g.S):
            ref[:, g.state2pdf[s]] += post[s]
        assert abs(z - z_d) <= 1e-10 and np.abs(gam - ref).max() <= 1e-10, (eps, z, z_d)


def test_zero_leak_is_pdfposteriors(wl, oracle):
    o, oc = oracle
    for name, g, V, L, N in _tiny_cases(wl):
        gam, z = lr.reference(g, V, L, N, 0.0)
        gam_p, z_p = _oracle_posteriors(o, oc, g, V, L, N)
        if not np.isfinite(z_p):
            assert np.isneginf(z) and (gam == 0).all(), name
            continue
        assert abs(z - z_p) <= 1e-12 and np.abs(gam - gam_p).max() <= 1e-12, (name, z, z_p)


def restart_case(wl):
    """l2r_hmm(3) with one-hot emissions that force the pdf sequence 0, 1, 0, 1, 2: no path of the graph goes back from state 1 to
    state 0, so the plain log Z is -inf; with a leak the path restarts in the initial state."""
    g = wl.l2r_hmm(3)
    V = np.full((5, g.P), -np.inf)
    V[np.arange(5), [0, 1, 0, 1, 2]] = 0.0
    return g, V


def test_restart_case(wl, oracle):
    o, oc = oracle
    g, V = restart_case(wl)
    _, z_plain = _oracle_posteriors(o, oc, g, V, 5, 5)
    assert np.isneginf(z_plain)
    gam0, z0 = lr.reference(g, V, 5, 5, 0.0)
    assert np.isneginf(z0) and (gam0 == 0).all()
    gam, z = lr.reference(g, V, 5, 5, 1e-5)
    gam_d, z_d = _oracle_posteriors(o, oc, lr.densify(g, 1e-5), V, 5, 5)
    assert np.isfinite(z) and abs(z - z_d) <= 1e-10 and abs(z - (-14.97864)) <= 1e-5, (z, z_d)
    assert np.allclose(gam.sum(-1), 1.0, atol=1e-12) and np.abs(gam - gam_d).max() <= 1e-10


def test_gradient_of_log_z_is_gamma(wl):
    """d log Z_eps / d V(n, p) = gamma_eps(n, p), by central differences on the reference."""
    rng = np.random.default_rng(5)
    h = 1e-6
    for g, L, N in ((wl.l2r_hmm(3), 5, 5), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 4, 5), (_shared_pdf(wl), 5, 5)):
        V = rng.standard_normal((N, g.P))
        for eps in (1e-5, 0.1):
            gam, _ = lr.reference(g, V, L, N, eps)
            num = np.zeros_like(gam)
            for n in range(L):
                for p in range(g.P):
                    Vp, Vm = V.copy(), V.copy()
                    Vp[n, p] += h
                    Vm[n, p] -= h
                    num[n, p] = (lr.reference(g, Vp, L, N, eps)[1] - lr.reference(g, Vm, L, N, eps)[1]) / (2 * h)
            assert np.abs(num - gam).max() <= 1e-7, (g.name, eps, np.abs(num - gam).max())


def test_log_z_is_non_decreasing_in_the_leak(wl):
    rng = np.random.default_rng(6)
    for g, L, N in ((wl.l2r_hmm(3), 6, 6), (wl.random_fsm(40, 6, 3.0, seed=1), 17, 20), (wl.lfmmi_denominator(300, 40), 30, 30)):
        V = rng.standard_normal((N, g.P))
        z = [lr.reference(g, V, L, N, eps)[1] for eps in (0.0, 1e-5, 1e-3, 0.1, 1.0)]
        assert all(np.isfinite(z)) and all(b >= a for a, b in zip(z, z[1:])), (g.name, z)
        assert z[-1] > z[0]


def test_float32_mode_within_the_gamma_bar(wl):
    """The recursion carried in float32 against float64 on lfmmi_denominator(300, 40), N = 200: within check_gamma's bars."""
    g = wl.lfmmi_denominator(300, 40)
    N = 200
    rng = np.random.default_rng(7)
    worst = 0.0
    for eps, L in ((1e-5, N), (0.1, N - 23)):
        V = rng.standard_normal((N, g.P)).astype(np.float32).astype(np.float64)
        g64, z64 = lr.reference(g, V, L, N, eps)
        g32, z32 = lr.reference(g, V, L, N, eps, dtype=np.float32)
        assert np.isclose(z32, z64, rtol=1e-5, atol=1e-4), (z32, z64)
        worst = max(worst, check_gamma(g32[None], g64[None], [L]))
    print(f"float32 recursion: worst log-posterior error over its bar {worst:.3g}")
    assert worst <= 1.0
