"""GPU tests of the pair kernels' phase B without a q vector (mm_kernel_pairs.hip, PairLay NQ / pair_pdf_sums_lin): the pdf sums
of step t - 1 multiply, during step t, the step's own vector in LDS with the partner row through the form's pdf-major table and
divide by the staged factor of the pdf.  The float32 kernels against the float64 oracle with the accuracy bar of
test_gpu_parity.py, on the smallest shapes at which that path can go wrong:

  * 2 and 4 passes over the pdfs (mm_fbp_kernel<2>, <4>), a graph of 60 states per pdf (more than four per lane of a group: the
    loop over the table runs), a state map with a pdf without a state and a pdf of one state, a graph of up to 127 states (the
    instance whose service wave copies one row of 64 float4);
  * B = 1, 2, 3 (the single utterance, the odd batch's copy pair) and N = 2 .. 9: each agent has 1 to 5 phase-B steps, the ring
    of four partner rows wraps once, and the pdf sums of the first and the last step run;
  * an emission of -inf (a factor of exactly 0: the posterior is exactly 0, never 0 * inf), and a pdf whose factor is below what
    the linear finishes accept in every frame.

Lengths and seeds.  `last_redo_count() == 0` is asserted after every call of the plain and the -inf cases, so that what is
compared is the float32 pair kernels' own result.  mm_pair_finish_kernel marks an utterance -- for the exact kernels, whatever
phase B computed -- when in some frame the forward and the backward mass overlap below 2^MM_LT_FLOOR of the frame's scale.  On
these 600-state graphs that happens to short utterances of plain randn emissions: of 3 frames most of all, and with 200 pdfs
(three states per pdf) to nearly every utterance of 3 to 5 frames.  It is a property of graph, emissions and length; the test
picks inputs that do not have it: a seed offset per graph and, where the default lengths of a shape are marked for that seed,
other lengths or another seed for that shape (the last field of GRAPHS).  Every B and N stays, and in every plain case the longest
utterance has N frames.  What differs from the defaults: nj2 (3, 6) and nj4 (3, 6) run (6, 4, 1) instead of (6, 3, 1); nj4 (2, 5)
runs (5, 2) instead of (5, 5), so no pair of two 5-frame utterances runs on the NJ = 4 instance; nj4 (2, 3) keeps (3, 1) under a
seed of its own (3 of 40 seeds leave a 3-frame utterance unmarked there).  The -60 cases do not assert the count.
"""
import dataclasses

import numpy as np
import pytest

import graphs
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu

PAIR = {"MM_DEBUG": "1", "MM_KERNEL": "pair"}


def _holes(wl):
    """lfmmi_denominator(600, 40, seed=5) with one more pdf than its states use, and pdf 3 left with a single state."""
    g = wl.lfmmi_denominator(600, 40, seed=5)
    s2p = np.array(g.state2pdf).copy()
    three = np.flatnonzero(s2p == 3)
    s2p[three[1:]] = 4
    return dataclasses.replace(g, name="lfmmi_600_40_holes", state2pdf=s2p.astype(np.asarray(g.state2pdf).dtype), P=g.P + 1)


# name -> (graph, what kernels() must say, environment of the batch, seed offset, {(B, N): (lengths, seed offset) in place of the defaults})
GRAPHS = {
    "nj2": (lambda wl: wl.lfmmi_denominator(600, 40, seed=5), "mm_fbp_kernel<2", None, 0, {(3, 6): ((6, 4, 1), 0)}),
    "nj4": (lambda wl: wl.lfmmi_denominator(600, 200, seed=5), "mm_fbp_kernel<4", None, 4,
            {(2, 3): ((3, 1), 15), (2, 5): ((5, 2), 4), (3, 6): ((6, 4, 1), 4)}),
    "loop": (lambda wl: wl.lfmmi_denominator(600, 10, seed=5), "mm_fbp_kernel<2", None, 1, {}),
    "holes": (_holes, "mm_fbp_kernel<2", None, 0, {}),
    "small": (lambda wl: wl.random_fsm(100, 12, 20.0, seed=5), "up to 127 states", PAIR, 0, {}),
}
SHAPES = [(1, 2, (2,)), (2, 3, (3, 1)), (3, 4, (4, 2, 0)), (2, 5, (5, 5)), (3, 6, (6, 3, 1)), (2, 9, (9, 4))]
_cache = {}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def compiled(mm, wl, gname):
    if gname not in _cache:
        g = GRAPHS[gname][0](wl)
        _cache[gname] = (g, mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P)))
    return _cache[gname]


def batch_of(mm, cf, B, env):
    return _with_env(env, lambda: mm.batch(*([cf] * B))) if env else mm.batch(*([cf] * B))


def run(bf, V, lens):
    gam, ttl = bf.pdfposteriors(V, lens)
    return np.asarray(gam.cpu() if hasattr(gam, "cpu") else gam), np.asarray(ttl.cpu() if hasattr(ttl, "cpu") else ttl)


def against_oracle(oracle, g, V, lens, gam, ttl, what):
    o, oc = oracle
    g_ref, t_ref = oc.batch_shared(graphs.to_oracle(o, g), g.state2pdf, g.P, V, lens, dtype=np.float64, nthreads=4)
    ok = np.isfinite(t_ref) & (lens > 0)  # (no frame, or a length no path through the graph has: gamma = 0 and ttl = zero(K))
    assert ok[0]
    print(what, "worst log-posterior error / bar:", check_gamma(gam[ok], g_ref[ok], lens[ok]), "ttl error:", np.abs(ttl[ok] - t_ref[ok]).max())
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=1e-4)
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()
    return g_ref


@pytest.mark.parametrize("B,N,lens", SHAPES)
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_plain_emissions(mm, wl, oracle, torch, gname, B, N, lens):
    g, cf = compiled(mm, wl, gname)
    _, kernel, env, k, other = GRAPHS[gname]
    lens, k = other.get((B, N), (lens, k))
    rng = np.random.default_rng(1000 * k + B * 100 + N)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.asarray(lens, dtype=np.int32)
    bf = batch_of(mm, cf, B, env)
    assert "mm_fbp_kernel<" in bf.kernels() and kernel in bf.kernels(), bf.kernels()
    gam, ttl = run(bf, V, lens)
    redo = bf.last_redo_count()
    against_oracle(oracle, g, V, lens, gam, ttl, f"{gname} B={B} N={N} lens={tuple(lens)} marked={redo}")
    assert redo == 0
    if gname == "holes":  # the pdf without a state
        assert (gam[..., g.P - 1] == 0).all()
    # two calls on the same batch: the same bits
    gam2, ttl2 = run(bf, V, lens)
    assert bf.last_redo_count() == 0
    assert np.array_equal(gam, gam2) and np.array_equal(ttl, ttl2, equal_nan=True)


@pytest.mark.parametrize("B,N,lens", [(2, 6, (6, 6)), (3, 5, (5, 5, 1))])
def test_an_emission_of_minus_infinity(mm, wl, oracle, torch, B, N, lens):
    """One frame of utterance 0 has -inf for one pdf: its factor is exactly 0 and the pdf sums divide by it.  That posterior is
    exactly 0, nothing is NaN, and the other utterance of the pair (utterance 1: the two longest are paired) gets the bits it gets
    without it.  No call may mark an utterance: a NaN frame sum would, and the exact kernels would then put the right values
    there.  (-inf itself raises no mark: stage() leaves it out of the step's smallest factor.)"""
    g, cf = compiled(mm, wl, "nj2")
    rng = np.random.default_rng(1000 + 7 * B + N)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.asarray(lens, dtype=np.int32)
    bf = batch_of(mm, cf, B, None)
    assert "mm_fbp_kernel<2" in bf.kernels()
    plain, _ = run(bf, V, lens)
    assert bf.last_redo_count() == 0
    for frame in (1, N - 2):  # (a frame of the forward agent's phase B and one of the backward agent's)
        W = V.copy()
        W[0, frame, 5] = -np.inf
        gam, ttl = run(bf, W, lens)
        assert bf.last_redo_count() == 0
        assert np.isfinite(gam).all() and not np.isnan(ttl).any()  # (ttl = -inf: the length no path of the graph has)
        assert gam[0, frame, 5] == 0
        assert np.array_equal(gam[1], plain[1])
        against_oracle(oracle, g, W, lens, gam, ttl, f"-inf at frame {frame}")


@pytest.mark.parametrize("B,N,lens", [(2, 6, (6, 5)), (3, 9, (9, 9, 2))])
def test_a_factor_below_the_linear_range(mm, wl, oracle, torch, B, N, lens):
    """pdf 2 at -60 in every frame: a factor below MM_LINF_EMIN.  The result meets the bar whichever kernels compute it."""
    g, cf = compiled(mm, wl, "nj2")
    rng = np.random.default_rng(11 * B + N)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    V[:, :, 2] = -60.0
    lens = np.asarray(lens, dtype=np.int32)
    bf = batch_of(mm, cf, B, None)
    gam, ttl = run(bf, V, lens)
    against_oracle(oracle, g, V, lens, gam, ttl, f"pdf at -60, B={B} N={N}")
