"""Arc posteriors (expected transition counts) without a GPU: the float64 reference helper against path enumeration, the
identities the definition implies, and the bindings of the new entry."""
import os
import re

import numpy as np
import pytest

import arc_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(wl, which):
    return wl.l2r_hmm(3) if which == "l2r3" else wl.random_fsm(6, 3, mean_deg=2.0, seed=4)


@pytest.mark.parametrize("which,N,L", [("l2r3", 5, 5), ("l2r3", 6, 4), ("rand6", 4, 4), ("rand6", 4, 3)])
def test_reference_against_path_enumeration(mm, wl, oracle, which, N, L):
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    V = np.random.default_rng(N + L).standard_normal((N, g.P))
    c, init, z = ar.reference(o, oc, g, f, V, L, N, chunk=2)
    ce, inite, ze = ar.enumerate_paths(g, f, V, L, N)
    assert np.isfinite(z) and np.isclose(z, ze, rtol=1e-10, atol=1e-10)
    assert np.allclose(c, ce, rtol=1e-9, atol=1e-12)
    assert np.allclose(init, inite, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("which", ["l2r3", "rand6"])
def test_sum_identities(mm, wl, oracle, which):
    """Real arcs sum to len - 1, the final arcs to 1, the phony self-loop gets N - len; the initial counts sum to 1."""
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    N = 7
    V = np.random.default_rng(3).standard_normal((N, g.P))
    for L in (7, 5, 3):
        c, init, z = ar.reference(o, oc, g, f, V, L, N)
        assert np.isfinite(z)
        real, fin, phony = j != fs, (j == fs) & (i != fs), (i == fs) & (j == fs)
        assert np.isclose(c[real].sum(), L - 1, atol=1e-9)
        assert np.isclose(c[fin].sum(), 1.0, atol=1e-9)
        assert np.isclose(c[phony].sum(), N - L, atol=1e-9)
        assert np.isclose(c.sum(), N, atol=1e-9) and np.isclose(init.sum(), 1.0, atol=1e-12)
    c, init, z = ar.reference(o, oc, g, f, V, 0, N)  # no frame: no accepting path
    assert np.isneginf(z) and (c == 0).all() and (init == 0).all()


def test_entry_is_bound(mm):
    assert callable(mm.arcposteriors) and hasattr(mm.BatchedFSM, "arcposteriors")
    assert "mm_arcposteriors_f32" in mm.SYMBOLS
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert lib.mm_arcposteriors_f32.argtypes is not None and len(lib.mm_arcposteriors_f32.argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_arcposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr


def test_julia_shim_has_the_literal_ccall():
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_arcposteriors_f32, LIB\)", src)
    assert re.search(r"function arcposteriors\(", src)
