"""Lattice path sampling (mm_latticesample_f32) without a GPU: the bindings of the new entry, the argument checks that need no device,
the float64 restatement of tests/latsample_reference.py -- the header's definition -- against the enumeration of every lattice path of
tiny utterances (the yardstick of the GPU tests, checked here by the Bernstein rule), the open-chain cap of every case the GPU file
puts to the decision rule, and lattices.lattice_sampled_risk on made-up samples.  The cases of tests/test_gpu_latticesample.py are
built here."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import latpost_reference as lp
import latsample_reference as ls
import lattice_reference as lr
from sample_reference import bernstein_ratio
from test_gpu_latticebest import _one_pair_fsm
from test_lattice import INF, chain_graph, emissions, entries_case, stub_batch
from test_latticeposteriors import CELL_COUNTS, record_scores, small_graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_DIST = 65536


# ---- the cases the GPU tests run
def _case(name, fs, gs, V, lens, br, extra, K, seed, offsets=None, arc=None, nrec=None):
    return SimpleNamespace(name=name, fs=fs, gs=gs, V=V, lens=lens, lat=br, extra=extra, K=K, seed=seed, offsets=br.offsets if offsets is None else offsets,
                           arc=br.arc if arc is None else arc, nrec=nrec)


def reference_of(c, K=None, ks=None):
    return ls.reference(c.fs, c.gs, c.V, c.lens, c.offsets, c.arc, c.extra, c.K if K is None else K, c.seed, nrec=c.nrec, ks=ks)


def tiny_cases(mm, wl):
    """The distribution cases: wl.random_fsm(S, 3, 2.0, seed) tropical, N = 6, the beam = inf lattice of the reference, extra NULL
    and given; one case with parallel entries between pairs of states (test_lattice.entries_case, its short utterance)."""
    out = []
    for S, seed, L in ((5, 1, 6), (5, 4, 6), (6, 2, 5), (6, 4, 5)):
        g = wl.random_fsm(S, 3, 2.0, seed)
        f = wl.to_fsm(mm, g, semiring="tropical")
        V = emissions(100 + seed, 1, 6, g.P, rounded=False, scale=1.0)
        lens = np.array([L], dtype=np.int32)
        br = lr.batch_reference([f], [g], V, lens, INF)
        for extra in (None, record_scores(seed, br.arc.size)):
            out.append(_case(f"random_fsm({S}, seed {seed}), extra {extra is not None}", [f], [g], V, lens, br, extra, K_DIST, 7 + seed))
    f, g, V, lens = entries_case(mm, 40)
    V, lens = (0.5 * V[1:2]).astype(np.float32), lens[1:2]
    br = lr.batch_reference([f], [g], V, lens, INF)
    out.append(_case("parallel entries", [f], [g], V, lens, br, 0.5 * record_scores(3, br.arc.size), K_DIST, 5))
    return out


def rand40_case(mm, wl, K=64, seed=3):
    """The 40-state random graph, B = 3, N = 6, the beam = inf lattice of V, under another V and an extra."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    V = emissions(31, B, N, g.P, rounded=False, scale=1.0)
    br = lr.batch_reference([f] * B, [g] * B, V, None, INF)
    return _case("40 states", [f] * B, [g] * B, emissions(32, B, N, g.P, rounded=False, scale=1.0), None, br, record_scores(8, br.arc.size, 0.5), K, seed)


def doctored_cases(mm, wl):
    """rand40_case through the raw entry: entry indices -1, nnz and the phony self-loop's; offsets that decrease, are negative and
    reach behind nrec; a lattice cut by cap (nrec below the total)."""
    c = rand40_case(mm, wl, K=8)
    f = c.fs[0]
    N = c.V.shape[1]
    sy = lr.system(f)
    off = c.lat.offsets
    arc = c.arc.copy()
    arc[int(off[1])], arc[int(off[N + 2]) + 1], arc[int(off[2 * N + 4])] = -1, f.nnz, int(np.flatnonzero(sy.phony)[0])
    nrec = int(off[N + 3]) + 2  # (utterance 0 whole, utterance 1 cut inside its fourth cell, utterance 2 without records)
    bad = off.copy()
    bad[0], bad[N + 2], bad[2 * N + 1] = -5, bad[N + 1] - 3, 2 ** 40
    return [_case("entries out of range", c.fs, c.gs, c.V, None, c.lat, c.extra, 8, 11, arc=arc),
            _case("a lattice cut by cap", c.fs, c.gs, c.V, None, c.lat, c.extra, 8, 12, arc=arc, nrec=nrec),
            _case("clamped offsets", c.fs, c.gs, c.V, None, c.lat, c.extra, 8, 13, offsets=bad, arc=arc, nrec=nrec)]


def cell_case(mm, n, K=8, equal=False):
    """Cells of exactly n records: latbest's one-pair FSM of n parallel entries, B = 2, N = 4."""
    f, g = _one_pair_fsm(mm, n, equal)
    B, N = 2, 4
    lens = np.array([4, 3], dtype=np.int32)
    V = emissions(n, B, N, g.P, rounded=False, scale=1.0)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, INF)
    return _case(f"{n} parallel entries", [f] * B, [g] * B, V, lens, br, None if equal else record_scores(n, br.arc.size, 0.5), K, 21 + n)


def chain_case(mm, wl):
    g = chain_graph(wl, 3000)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 5, 4), np.array([5, 3], dtype=np.int32)
    br = lr.batch_reference([f, f], [g, g], V, lens, 1.0)
    return _case("chain of 3000", [f, f], [g, g], emissions(4, 2, 5, 4, rounded=False), lens, br, None, 8, 9)


def capture_cases(mm, wl):
    """The two replays of the graph-capture test: rand40_case under a new V and a new extra each."""
    c = rand40_case(mm, wl)
    B, N = c.V.shape[0], c.V.shape[1]
    return [SimpleNamespace(**{**vars(c), "name": f"replay {s}", "V": emissions(s, B, N, c.gs[0].P, rounded=False, scale=1.0), "extra": record_scores(s, c.arc.size, 0.5)})
            for s in (41, 42)]


def decision_cases(mm, wl):
    """Every case the GPU file puts to the decision rule: the two small graphs at B = 3, N = 12, lens (12, 9, 0), beam 6, extra NULL
    and given, K = 8; the 40-state lattice at K = 64; the cell sizes; the thread-count cells at K = 70; the chain; the doctored
    inputs; the replays of the graph capture."""
    out = []
    B, N = 3, 12
    lens = np.array([N, N - 3, 0], dtype=np.int32)
    for which, (g, f) in enumerate(small_graphs(mm, wl)):
        V = emissions(40 + which, B, N, g.P, rounded=False, scale=1.0)
        br = lr.batch_reference([f] * B, [g] * B, V, lens, 6.0)
        for extra in (None, record_scores(4, br.arc.size)):
            out.append(_case(f"{g.name}, extra {extra is not None}", [f] * B, [g] * B, emissions(50 + which, B, N, g.P, rounded=False, scale=1.0), lens, br, extra, 8,
                             30 + which))
    out.append(rand40_case(mm, wl))
    out += [cell_case(mm, n) for n in CELL_COUNTS]
    out += [cell_case(mm, n, K=70) for n in (257, 1025)]
    out.append(chain_case(mm, wl))
    return out + doctored_cases(mm, wl) + capture_cases(mm, wl)


def edit_distance(a, b):
    """The Levenshtein distance of two sequences."""
    d = list(range(len(b) + 1))
    for x in a:
        prev, d[0] = d[0], d[0] + 1
        for q, y in enumerate(b, 1):
            prev, d[q] = d[q], min(d[q] + 1, d[q - 1] + 1, prev + (x != y))
    return d[-1]


def sampled_risk_gradients(costs, rec, path, s2p, g, shape, nrec):
    """lattice_sampled_risk's backward by its formula: (dV [B, N, P], dextra [nrec]) float64 for the upstream gradient g [B]."""
    costs = np.asarray(costs, dtype=np.float64)
    B, K = costs.shape
    w = (costs - (costs.sum(1, keepdims=True) - costs) / (K - 1)) / K
    gV, gE = np.zeros(shape), np.zeros(nrec)
    for b in range(B):
        for k in range(K):
            for n in range(path.shape[2]):
                if path[b, k, n] >= 0:
                    gV[b, n, s2p[b][path[b, k, n]]] += g[b] * w[b, k]
                    gE[rec[b, k, n]] += g[b] * w[b, k]
    return gV, gE, w


# ---- the tests
@pytest.fixture(autouse=True)
def _the_entry(mm):
    """Every test of this file is about mm_latticesample_f32, the yardsticks included: none passes without the entry."""
    assert "mm_latticesample_f32" in mm.SYMBOLS and hasattr(mm.BatchedFSM, "latticesample")


def test_entry_is_bound(mm):
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_latticesample_f32" in mm.SYMBOLS and len(lib.mm_latticesample_f32.argtypes) == 23
    assert callable(mm.latticesample) and hasattr(mm.BatchedFSM, "latticesample")
    assert mm.LatticeSamples._fields == ("rec", "path", "logprob", "logz")
    assert callable(mm.lattices.lattice_sampled_risk) and mm.lattice_sampled_risk is mm.lattices.lattice_sampled_risk
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_latticesample_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr and "22 = mm_latticesample_f32" in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_latticesample_f32, LIB\)", src) and "function latticesample(" in src
    # the generator's two functions live in one header that both translation units include
    csrc = os.path.join(ROOT, "markovmodels.jl_amd", "csrc")
    assert "philox_4x32_10(unsigned k0" in open(os.path.join(csrc, "mm_philox.h")).read()
    for name in ("mm_kernel_sample.hip", "mm_kernel_latsample.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "mm_philox.h"' in text and "philox_4x32_10(unsigned k0" not in text, name


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: offsets or logz NULL (-1), a negative nrec (-1), arc or fwd NULL
    with records to read (-1), nsamples below 1 (-1), rec and path both NULL (-1), strides of rec, path and logprob that overlap (-2);
    with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))

    def call(offsets=p, arc=p, nrec=4, extra=None, K=3, seed=1, fwd=fp, rec=p, rsb=24, rsk=8, path=None, psb=0, psk=0, logprob=None, lsb=0, logz=fp, N=8):
        return lib.mm_latticesample_f32(None, fp, 8, 1, None, N, offsets, arc, nrec, extra, K, seed, fwd, rec, rsb, rsk, path, psb, psk, logprob, lsb, logz, None)

    for kw in ({"offsets": None}, {"logz": None}, {"arc": None}, {"fwd": None}):
        assert call(**kw) == -1 and b"is NULL" in lib.mm_last_error(), kw
    assert call(nrec=-1) == -1 and b"nrec" in lib.mm_last_error()
    for K in (0, -5):
        assert call(K=K) == -1 and b"nsamples" in lib.mm_last_error()
    assert call(rec=None) == -1 and b"both NULL" in lib.mm_last_error()
    assert call(rsk=7) == -2 and b"rec_stride_k" in lib.mm_last_error()
    assert call(rsb=23) == -2 and b"rec_stride_b" in lib.mm_last_error()
    assert call(path=p, psb=24, psk=7) == -2 and b"path_stride_k" in lib.mm_last_error()
    assert call(path=p, psb=23, psk=8) == -2 and b"path_stride_b" in lib.mm_last_error()
    assert call(logprob=fp, lsb=2) == -2 and b"lp_stride_b" in lib.mm_last_error()
    assert call(K=64 * 65535 + 1, rsb=8 * (64 * 65535 + 1)) == -4 and b"samples" in lib.mm_last_error()
    assert call() == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(arc=None, fwd=None, nrec=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (an empty lattice needs neither)
    assert call(rec=None, path=p, psb=24, psk=8, logprob=fp, lsb=3, extra=fp) == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(psk=0, psb=0, lsb=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (strides of outputs not asked for are not looked at)


def test_generator_restatement():
    """Philox-4x32-10 against the known-answer vectors of Random123 (the first word), unit_open's ends, and the range of g the header
    states."""
    assert int(ls.philox_4x32_10(0, 0, 0, 0, 0, 0)) == 0x6627E8D5
    assert int(ls.philox_4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == 0x408F276D
    assert int(ls.philox_4x32_10(0xA4093822, 0x299F31D0, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)) == 0xD16CFE09
    lo, hi = ls.unit_open(0), ls.unit_open(0xFFFFFFFF)
    assert lo == 2.0 ** -24 and hi == 1 - 2.0 ** -24 and np.float32(lo) == lo and np.float32(hi) == hi
    assert abs(ls.gumbel(lo) + 2.81) < 0.01 and abs(ls.gumbel(hi) - 16.64) < 0.01
    assert ls.seed_key(-1) == (0xFFFFFFFF, 0xFFFFFFFF) and ls.seed_key(2 ** 32 + 5) == (5, 1)


def test_reference_sampler_against_the_enumeration(mm, wl):
    """The yardstick: on the tiny cases the restatement's K = 65 536 record sequences have the enumeration's frequencies by the
    Bernstein rule (ratio <= 1), none lies outside the enumeration, logprob is the enumeration's, and parallel records between one
    pair of states are told apart -- the case with parallel entries holds such records with different posteriors."""
    seen_parallel = False
    for c in tiny_cases(mm, wl):
        f, g = c.fs[0], c.gs[0]
        N, L = c.V.shape[1], int(c.lens[0])
        paths, logp, logz = ls.enumerate_paths(f, g.state2pdf, g.P, c.V[0], L, N, lp.cells(c.offsets, c.arc.size, 0, N), c.arc, c.extra)
        assert 2 <= paths.shape[0] <= 20000, (c.name, paths.shape)
        ref = reference_of(c)
        assert abs(ref.logz[0] - logz) <= 1e-12 * max(1, abs(logz)), c.name
        assert (ref.rec[0, :, L:] == -1).all() and (ref.path[0, :, L:] == -1).all()
        freq, outside = ls.path_frequencies(paths, ref.rec[0, :, :L])
        ratio = bernstein_ratio(freq, np.exp(logp), c.K)
        print(f"{c.name}: {paths.shape[0]} paths, Bernstein ratio {ratio:.3f}, open chains {ref.open.mean():.2e}")
        assert outside == 0 and ratio <= 1, (c.name, outside, ratio)
        index = {tuple(p): q for q, p in enumerate(paths.tolist())}
        for k in range(0, c.K, 997):
            assert abs(ref.logprob[0, k] - logp[index[tuple(ref.rec[0, k, :L])]]) <= 1e-12, (c.name, k)
        sy = lr.system(f)
        assert np.array_equal(ref.path[0, :, :L], sy.i[c.arc[ref.rec[0, :, :L]]])
        # parallel records of one (source, destination) in one cell, each with its own posterior
        post = lp.reference(c.fs, c.gs, c.V, c.lens, c.offsets, c.arc, c.extra).post
        for lo, hi in lp.cells(c.offsets, c.arc.size, 0, N)[:L]:
            pairs = {}
            for r in range(lo, hi):
                if post[r] > -np.inf:
                    pairs.setdefault((sy.i[c.arc[r]], sy.j[c.arc[r]]), []).append(r)
            for rs in pairs.values():
                if len(rs) > 1 and np.ptp(post[rs]) > 0.1:
                    seen_parallel = True
                    cnt = np.array([(ref.rec[0, :, :L] == r).sum() for r in rs]) / c.K
                    assert bernstein_ratio(cnt, np.exp(post[rs]), c.K, M=c.arc.size) <= 1, (c.name, rs)
    assert seen_parallel


def test_open_chain_cap_of_every_gpu_case(mm, wl):
    """The condition of the decision rule, from the restatement alone: at most 5 % of the chains of every case the GPU file runs
    hold an open decision (the seeds are chosen so); an utterance with a path has none of its chains dying."""
    for c in decision_cases(mm, wl) + tiny_cases(mm, wl):
        ref = reference_of(c, K=min(c.K, 4096))
        share = ref.open.mean()
        print(f"{c.name}: K {ref.open.shape[1]}, open chains {int(ref.open.sum())} of {ref.open.size}")
        assert share <= 0.05, (c.name, share)
        for b in range(len(c.fs)):
            L = ref.uts[b].L if np.isfinite(ref.logz[b]) else 0
            assert (ref.rec[b, :, :L] >= 0).all() and (ref.rec[b, :, L:] == -1).all(), (c.name, b)
    # the RNG contract's calls (K = 3, 64, 65, 130 and another seed) on the 40-state lattice
    for K, seed in ((130, 3), (130, 4)):
        assert reference_of(rand40_case(mm, wl, K, seed)).open.mean() <= 0.05


def test_prefix_property_of_the_restatement(mm, wl):
    """A sample depends on its index alone: the restatement at ks = (5, 64, 129) equals rows 5, 64 and 129 of K = 130."""
    c = rand40_case(mm, wl, K=130)
    full = reference_of(c)
    part = reference_of(c, ks=np.array([5, 64, 129]))
    assert np.array_equal(part.rec, full.rec[:, [5, 64, 129]]) and np.array_equal(part.logprob, full.logprob[:, [5, 64, 129]])
    assert not np.array_equal(full.rec[0], full.rec[1])  # (equal utterances at different positions)


def test_edit_distance():
    assert edit_distance([1, 2, 3], [1, 2, 3]) == 0 and edit_distance([1, 2, 3], [2, 3, 1]) == 2 and edit_distance([], [4, 4]) == 2
    assert edit_distance([1, 2, 3, 4], [1, 3, 4, 4]) == 2 and edit_distance([5, 5, 5], [6, 6, 6]) == 3


def test_sampled_risk_backward_on_made_up_samples(mm, wl):
    """lattices.lattice_sampled_risk on CPU tensors and made-up samples: the forward is the mean cost (0 without a path), the backward
    the formula -- g[b] w_k scattered to V at (b, n, pdf(path[b, k, n])) and to extra at rec[b, k, n] -- and the leave-one-out weights
    of every utterance sum to 0; costs take no gradient; K = 1 and samples without path are refused."""
    import torch

    g, f = small_graphs(mm, wl)[1]
    B, N, K = 3, 6, 5
    bf = stub_batch(mm, [f] * B, [g] * B)
    rng = np.random.default_rng(0)
    nrec = 50
    S = f.S1 - 1
    path = rng.integers(0, S, (B, K, N)).astype(np.int32)
    rec = rng.integers(0, nrec, (B, K, N)).astype(np.int64)
    path[1, :, 4:] = -1
    rec[1, :, 4:] = -1
    path[2], rec[2] = -1, -1  # (no path)
    logz = np.array([-3.0, -5.0, -np.inf], dtype=np.float32)
    costs = rng.integers(0, 7, (B, K)).astype(np.float32)
    samples = mm.LatticeSamples(torch.from_numpy(rec), torch.from_numpy(path), None, torch.from_numpy(logz))
    V = torch.zeros((B, N, g.P), requires_grad=True)
    extra = torch.zeros(nrec, requires_grad=True)
    ct = torch.from_numpy(costs).requires_grad_(True)
    risk = mm.lattices.lattice_sampled_risk(bf, None, V, samples, ct, extra)
    assert np.array_equal(risk.detach().numpy(), np.array([costs[0].mean(), costs[1].mean(), 0], dtype=np.float32))
    up = np.array([1.5, -2.0, 3.0], dtype=np.float32)
    risk.backward(torch.from_numpy(up))
    gV, gE, w = sampled_risk_gradients(costs, rec, path, [np.asarray(g.state2pdf)] * B, up, (B, N, g.P), nrec)
    assert np.abs(w.sum(1)).max() <= 1e-12 and np.abs(w).max() > 0.1
    assert np.allclose(V.grad.numpy(), gV, rtol=0, atol=1e-5) and np.allclose(extra.grad.numpy(), gE, rtol=0, atol=1e-5)
    assert (V.grad.numpy()[2] == 0).all() and (V.grad.numpy()[1, 4:] == 0).all() and ct.grad is None
    assert np.abs(V.grad.numpy().sum(axis=2)).max() <= 1e-5  # (every frame's weights sum to 0 over the pdfs)
    V2 = torch.zeros((B, N, g.P), requires_grad=True)
    mm.lattices.lattice_sampled_risk(bf, None, V2, samples, ct).sum().backward()  # (extra None)
    assert np.allclose(V2.grad.numpy(), sampled_risk_gradients(costs, rec, path, [np.asarray(g.state2pdf)] * B, np.ones(B), (B, N, g.P), nrec)[0], rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        mm.lattices.lattice_sampled_risk(bf, None, V, mm.LatticeSamples(samples.rec[:, :1], samples.path[:, :1], None, samples.logz), ct[:, :1])
    with pytest.raises(ValueError):
        mm.lattices.lattice_sampled_risk(bf, None, V, mm.LatticeSamples(samples.rec, None, None, samples.logz), ct)
    with pytest.raises(ValueError):
        mm.lattices.lattice_sampled_risk(bf, None, V, samples, ct[:, :3])
