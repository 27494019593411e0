"""Posterior path sampling without a GPU: the float64 helpers of tests/sample_reference.py against each other, the Bernstein
rule on a correct sampler and on two wrong ones, and the bindings of the new entry."""
import os
import re

import numpy as np
import pytest

import arc_reference as ar
import sample_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 65536


@pytest.mark.parametrize("case", range(len(sr.TINY_CASES)))
def test_enumeration_matches_the_arc_reference(mm, wl, case):
    """log Z of the state-sequence enumeration = log Z of arc_reference's enumeration over all S1^(N+1) sequences; the
    probabilities sum to one; the support has the size recorded with the cases."""
    S, seed, N, L = sr.TINY_CASES[case]
    g, f, V = sr.tiny_case(mm, wl, S, seed, N)
    gr = sr.Graph(g, f)
    paths, logp, logZ = sr.enumerate_posterior(gr, V, L)
    assert paths.shape[0] == sr.TINY_SUPPORT[case]
    assert np.isclose(np.exp(logp).sum(), 1.0, atol=1e-12)
    if S == 5:  # (6^7 sequences; the S = 6 cases would be 7^7)
        _, _, ze = ar.enumerate_paths(g, f, V, L, N)
        assert np.isclose(logZ, ze, rtol=1e-12, atol=1e-12)
    assert np.allclose(sr.path_logprob(gr, V, paths) - logZ, logp)


@pytest.mark.parametrize("case", range(len(sr.TINY_CASES)))
def test_bernstein_rule_accepts_the_numpy_sampler(mm, wl, case):
    S, seed, N, L = sr.TINY_CASES[case]
    g, f, V = sr.tiny_case(mm, wl, S, seed, N)
    gr = sr.Graph(g, f)
    paths, logp, _ = sr.enumerate_posterior(gr, V, L)
    smp = sr.ffbs(gr, V, L, K, np.random.default_rng(7 + case))
    freq, outside = sr.frequencies(gr, paths, smp)
    ratio = sr.bernstein_ratio(freq, np.exp(logp), K)
    print(f"case {case}: support {paths.shape[0]}, min p {np.exp(logp).min():.2e}, worst cell at {ratio:.3f} of the bound")
    assert outside == 0
    assert ratio <= 1.0


@pytest.mark.parametrize("wrong", ["no_emissions", "shifted_emissions"])
@pytest.mark.parametrize("case", range(len(sr.TINY_CASES)))
def test_bernstein_rule_rejects_wrong_samplers(mm, wl, case, wrong):
    """A sampler that ignores the emissions, and one that reads them one frame late, break the rule: it can tell a wrong
    kernel from a right one."""
    S, seed, N, L = sr.TINY_CASES[case]
    g, f, V = sr.tiny_case(mm, wl, S, seed, N)
    gr = sr.Graph(g, f)
    paths, logp, _ = sr.enumerate_posterior(gr, V, L)
    Vw = np.zeros_like(V) if wrong == "no_emissions" else np.roll(V, 1, axis=0)
    smp = sr.ffbs(gr, Vw, L, K, np.random.default_rng(7 + case))
    freq, _ = sr.frequencies(gr, paths, smp)
    ratio = sr.bernstein_ratio(freq, np.exp(logp), K)
    print(f"case {case} {wrong}: worst cell at {ratio:.1f} times the bound")
    assert ratio > 1.0


def test_transition_lookup(mm, wl):
    g = wl.l2r_hmm(3)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    gr = sr.Graph(g, f)
    i, j, w = ar.fsm_entries(f)
    assert np.allclose(gr.weight(i, j), w) and np.isneginf(gr.weight([2], [0])[0])


def test_entry_is_bound(mm):
    assert callable(mm.samplepaths) and hasattr(mm.BatchedFSM, "samplepaths")
    assert "mm_samplepaths_f32" in mm.SYMBOLS
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert lib.mm_samplepaths_f32.argtypes is not None and len(lib.mm_samplepaths_f32.argtypes) == 15
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_samplepaths_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr and "Philox" in hdr


def test_julia_shim_has_the_literal_ccall():
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_samplepaths_f32, LIB\)", src)
    assert re.search(r"function samplepaths\(", src)
