"""Posterior path sampling (mm_samplepaths_f32) on the MI355X: the exact distribution over the state sequences of tiny graphs
(Bernstein rule of tests/sample_reference.py), pdf marginals at real sizes against the float64 oracle, validity and log-probability
of every sampled path, the random-number contract, hipGraph capture, edges and error codes."""
import ctypes as C
import os

import numpy as np
import pytest

import graphs
import sample_reference as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_EXACT = 65536
K_SIZE = 512


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib").lib


def _batch(mm, wl, gs):
    fs = [wl.to_fsm(mm, g) for g in gs]
    return fs, mm.batch(*[mm.compile(f, mm.statemap(g.state2pdf, g.P)) for f, g in zip(fs, gs)])


def _exact_check(gr, support, logp, paths, lp, L, tag):
    """One utterance's samples [K, N] (and log-probabilities) against the enumeration: support, Bernstein rule, logprob."""
    assert (paths[:, L:] == -1).all()
    smp = paths[:, :L]
    freq, outside = sr.frequencies(gr, support, smp)
    ratio = sr.bernstein_ratio(freq, np.exp(logp), smp.shape[0])
    print(f"{tag}: support {support.shape[0]}, {outside} samples outside it, worst cell at {ratio:.3f} of the bound")
    assert outside == 0
    assert ratio <= 1.0
    if lp is not None:
        sc = sr.path_codes(gr, support)
        order = np.argsort(sc)
        ref = logp[order][np.searchsorted(sc[order], sr.path_codes(gr, smp))]
        err = np.abs(lp.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        print(f"{tag}: logprob worst relative error {err.max():.2e}")
        assert (err <= 1e-4).all()


# ---- 1. the exact distribution
@pytest.mark.parametrize("case", range(len(sr.TINY_CASES)))
def test_exact_distribution_on_tiny_graphs(mm, wl, torch, case):
    _exact_tiny_run(mm, wl, case)


def _exact_tiny_run(mm, wl, case):
    """The case above; returns the batch it ran."""
    S, seed, N, L = sr.TINY_CASES[case]
    g, f64, V = sr.tiny_case(mm, wl, S, seed, N)
    gr = sr.Graph(g, f64)
    support, logp, logZ = sr.enumerate_posterior(gr, V, L)
    _, bf = _batch(mm, wl, [g, g])
    Vb = np.stack([V, V]).astype(np.float32)
    paths, ttl, lp = bf.samplepaths(Vb, [L, L], nsamples=K_EXACT, seed=1234 + case, want_logprob=True)
    assert paths.shape == (2, K_EXACT, N) and paths.dtype == np.int32 and lp.shape == (2, K_EXACT)
    assert np.allclose(ttl, logZ, rtol=1e-5, atol=1e-5)
    for b in range(2):
        _exact_check(gr, support, logp, paths[b], lp[b], L, f"case {case} utterance {b}")
    assert not np.array_equal(paths[0], paths[1])  # (independent streams: the key is the position in the batch)
    return bf


# ---- 2. / 3. marginals, validity and logprob at real sizes
def _size_check(mm, wl, oracle, gs, V, lens, K=K_SIZE, marginals=True, seed=5):
    o, oc = oracle
    fs, bf = _batch(mm, wl, gs)
    B, N, P = V.shape
    paths, ttl, lp = bf.samplepaths(V, lens, nsamples=K, seed=seed, want_logprob=True)
    _, t2 = bf.pdfposteriors(V, lens)
    worst = 0.0
    for b in range(B):
        g, f, L = gs[b], fs[b], int(lens[b])
        gr = sr.Graph(g, f)
        Vhat = np.full((P + 1, N + 1), -np.inf)
        Vhat[:P, :L] = V[b, :L].astype(np.float64).T
        Vhat[P, L:] = 0.0
        gamma, z = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64)  # gamma [P, N]
        # ttl: the bar arc_reference.check applies to it, and pdfposteriors' own value
        assert np.isclose(ttl[b], z, rtol=1e-5, atol=1e-5 * max(1.0, abs(z)) + 1e-4), (ttl[b], z)
        assert np.isclose(ttl[b], t2[b], rtol=1e-5, atol=1e-5 * max(1.0, abs(z)) + 1e-4), (ttl[b], t2[b])
        pb = paths[b]
        assert (pb[:, L:] == -1).all() and (pb[:, :L] >= 0).all() and (pb[:, :L] < gr.fin).all()
        # validity: starts in a state of alpha_hat, every step a stored arc, the last state has an omega entry
        smp = pb[:, :L].astype(np.int64)
        assert np.isfinite(gr.a[smp[:, 0]]).all()
        for n in range(L - 1):
            assert np.isfinite(gr.weight(smp[:, n], smp[:, n + 1])).all(), (b, n)
        assert np.isfinite(gr.weight(smp[:, -1], np.full(K, gr.fin))).all()
        score = sr.path_logprob(gr, V[b].astype(np.float64), smp)
        err = np.abs(lp[b].astype(np.float64) - (score - z)) / np.maximum(abs(z), np.abs(score))
        print(f"utterance {b}: len {L}, log Z {z:.3f}, logprob worst error {err.max():.2e} of max(|log Z|, |score|)")
        assert (err <= 1e-4).all()
        if marginals:
            s2p = np.asarray(g.state2pdf, dtype=np.int64)
            occ = np.zeros((L, P))
            pdf = s2p[smp]  # [K, L]
            for n in range(L):
                occ[n] = np.bincount(pdf[:, n], minlength=P)
            r = sr.bernstein_ratio(occ / K, gamma[:, :L].T, K, M=B * N * P)
            worst = max(worst, r)
            print(f"utterance {b}: pdf occupancy worst cell at {r:.3f} of the bound")
    assert worst <= 1.0
    return bf, paths, lp


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph(mm, wl, oracle, torch, sharp):
    g = wl.lfmmi_denominator()
    B, N = 4, 1500
    x = np.random.default_rng(3).standard_normal((B, N, g.P))
    V = (torch.log_softmax(torch.from_numpy(10.0 * x), dim=-1).numpy() if sharp else x).astype(np.float32)
    lens = np.array([N - 37 * k for k in range(B)], dtype=np.int32)
    _size_check(mm, wl, oracle, [g] * B, V, lens)


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, oracle, torch, name):
    g = wl.load_npz_graph(os.path.join(HERE, "golden", name + ".npz"))
    B, N = 3, 700
    V = np.random.default_rng(11).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([N, 611, 430], dtype=np.int32) if name.startswith("den") else np.array([N, 650, 500], dtype=np.int32)
    _size_check(mm, wl, oracle, [g] * B, V, lens)


def test_distinct_graphs_in_their_own_order(mm, wl, oracle, torch):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    _size_check(mm, wl, oracle, gs, V, lens)


def test_bigv_graph(mm, wl, oracle, torch):
    """A graph beyond the LDS: the alpha~ rows are gathered from global memory."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    N = 40
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([40, 29], dtype=np.int32)
    bf, _, _ = _size_check(mm, wl, oracle, [g, g], V, lens, marginals=False)
    assert "mm_sample_kernel<global>" in bf.kernels("sample")


def test_more_samples_than_one_workgroup_and_in_arc_lists_beyond_a_wave(mm, wl, oracle, torch):
    """A dense ergodic graph of 200 states: every in-list has 200 entries (four chunks of 64 lanes); K = 200 is several
    workgroups per utterance."""
    g = wl.dense_ergodic(200)
    N = 30
    V = np.random.default_rng(8).standard_normal((2, N, g.P)).astype(np.float32)
    _size_check(mm, wl, oracle, [g, g], V, np.array([30, 17], dtype=np.int32), K=200)


# ---- 4. the random-number contract
def test_rng_contract(mm, wl, torch):
    cases = [sr.TINY_CASES[0], sr.TINY_CASES[3], sr.TINY_CASES[7]]
    N = 6
    built = [sr.tiny_case(mm, wl, S, seed, N) for S, seed, _, _ in cases]
    gs = [t[0] for t in built]
    lens = [c[3] for c in cases]
    V = np.stack([t[2] for t in built]).astype(np.float32)
    _, bf = _batch(mm, wl, gs)
    p1, t1, l1 = bf.samplepaths(V, lens, nsamples=64, seed=99, want_logprob=True)
    p2, t2, l2 = bf.samplepaths(V, lens, nsamples=64, seed=99, want_logprob=True)
    assert np.array_equal(p1, p2) and np.array_equal(l1, l2) and np.array_equal(t1, t2)  # the same seed: the same bits
    p8, _, l8 = bf.samplepaths(V, lens, nsamples=8, seed=99, want_logprob=True)
    assert np.array_equal(p8, p1[:, :8]) and np.array_equal(l8, l1[:, :8])  # K = 8 is the prefix of K = 64
    # ... and of every larger K, whatever launch geometry the engine picks for it (1, 2, 4 or 8 chains per wave)
    p2k, _, l2k = bf.samplepaths(V, lens, nsamples=2048, seed=99, want_logprob=True)
    p4k, _, l4k = bf.samplepaths(V, lens, nsamples=4096, seed=99, want_logprob=True)
    assert np.array_equal(p2k[:, :64], p1) and np.array_equal(l2k[:, :64], l1)
    assert np.array_equal(p4k[:, :2048], p2k) and np.array_equal(l4k[:, :2048], l2k)
    p3, _ = bf.samplepaths(V, lens, nsamples=64, seed=100)
    assert not np.array_equal(p3, p1)  # another seed
    pn, _ = bf.samplepaths(V, lens, nsamples=64, seed=-(2**63))
    assert not np.array_equal(pn, p1) and (pn[:, :, 0] >= 0).all()
    # the utterances in another order: position 0 -> 2, 1 -> 0, 2 -> 1.  The keys are positions, so an utterance's samples change
    # with its position -- and at each position they still follow its posterior
    perm = [1, 2, 0]
    _, bq = _batch(mm, wl, [gs[i] for i in perm])
    pa, _, la = bf.samplepaths(V, lens, nsamples=K_EXACT, seed=99, want_logprob=True)
    assert np.array_equal(pa[:, :4096], p4k) and np.array_equal(la[:, :4096], l4k)
    pq, _, lq = bq.samplepaths(V[perm], [lens[i] for i in perm], nsamples=K_EXACT, seed=99, want_logprob=True)
    for pos, i in enumerate(perm):
        assert not np.array_equal(pq[pos], pa[i])
    for i in range(3):
        gr = sr.Graph(built[i][0], built[i][1])
        support, logp, _ = sr.enumerate_posterior(gr, built[i][2], lens[i])
        _exact_check(gr, support, logp, pa[i], la[i], lens[i], f"utterance {i} at position {i}")
        _exact_check(gr, support, logp, pq[perm.index(i)], lq[perm.index(i)], lens[i], f"utterance {i} at position {perm.index(i)}")


# ---- 5. hipGraph
def test_graph_capture(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    # a capture before any eager call: the forms are not on the device, and are never built during a capture
    _, fresh = _batch(mm, wl, [g] * 6)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.samplepaths(V, lens, nsamples=16, seed=3, want_logprob=True)
    assert ei.value.code == -1 and "not on the device yet" in str(ei.value)
    # after one eager call: capture, replay, the eager result
    _, bf = _batch(mm, wl, [g] * 6)
    p0, t0, l0 = bf.samplepaths(V, lens, nsamples=16, seed=3, want_logprob=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p2, t2, l2 = bf.samplepaths(V, lens, nsamples=16, seed=3, want_logprob=True)
    for _ in range(2):
        p2.zero_()
        t2.zero_()
        l2.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(p2, p0) and torch.equal(t2, t0) and torch.equal(l2, l0)
    assert (p0[0] >= 0).all() and (p0[4, :, 7:] == -1).all()


# ---- 6. edges and errors
def test_edges(mm, wl, torch):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([N, 0, 1, N - 2, N - 5], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((5, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf  # a frame with -inf entries: those pdfs are never drawn there
    V[3, 4, :] = -np.inf   # no accepting path
    fs, bf = _batch(mm, wl, [g] * 5)
    K = 100
    paths, ttl, lp = bf.samplepaths(V, lens, nsamples=K, seed=1, want_logprob=True)
    _, t2 = bf.pdfposteriors(V, lens)
    assert (np.isfinite(ttl) == np.isfinite(t2)).all() and np.allclose(ttl[np.isfinite(t2)], t2[np.isfinite(t2)], rtol=1e-5, atol=1e-4)
    for b in (1, 3):  # no frame / no path
        assert (paths[b] == -1).all() and np.isneginf(lp[b]).all() and np.isneginf(ttl[b])
    gr = sr.Graph(g, fs[0])
    s2p = np.asarray(g.state2pdf)
    for b in (0, 2, 4):
        L = int(lens[b])
        smp = paths[b, :, :L].astype(np.int64)
        assert (smp >= 0).all() and (paths[b, :, L:] == -1).all() and np.isfinite(lp[b]).all()
        score = sr.path_logprob(gr, V[b].astype(np.float64), smp)
        assert np.isfinite(score).all()
        assert np.allclose(lp[b], score - float(ttl[b]), rtol=1e-4, atol=1e-4 * abs(float(ttl[b])))
    assert (s2p[paths[0, :, 7]] >= 3).all()
    assert np.isfinite(gr.a[paths[2, :, 0]]).all() and np.isfinite(gr.weight(paths[2, :, 0], np.full(K, gr.fin))).all()  # len 1


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N, K = 10, 4
    V = torch.zeros((2, N, g.P), device="cuda")
    paths = torch.zeros((2, K, N), dtype=torch.int32, device="cuda")
    lp = torch.zeros((2, K), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, p=paths.data_ptr(), k=K, psb=K * N, psk=N, lptr=lp.data_ptr(), lsb=K):
        return lib.mm_samplepaths_f32(h, V.data_ptr(), N * g.P, g.P, None, N, k, 0, p, psb, psk, lptr, lsb, None, st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * 2))
    assert call(tb._h) == -4
    assert b"log" in lib.mm_last_error()
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * 2))
    assert call(lb._h, p=None) == -1
    assert call(lb._h, k=0) == -1
    assert call(lb._h, psk=N - 1) == -2
    assert call(lb._h, psb=K * N - 1) == -2
    assert call(lb._h, lsb=K - 1) == -2
    assert call(lb._h, lptr=None, lsb=0) == 0
    assert call(lb._h) == 0
    torch.cuda.synchronize()
    assert (paths >= 0).all() and (paths < g.S).all() and torch.isfinite(lp).all()
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("sample")


# ---- 7. the kernels of the call
def test_kernels_names(mm, wl, torch):
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    _, bf = _batch(mm, wl, [g, g])
    s = bf.kernels("sample")
    assert "mm_log_kernel<MODE_FB" in s and "mm_sample_kernel<lds>" in s


def test_module_level_samplepaths(mm, wl, torch):
    S, seed, N, L = sr.TINY_CASES[0]
    g, f64, V = sr.tiny_case(mm, wl, S, seed, N)
    gr = sr.Graph(g, f64)
    f = wl.to_fsm(mm, g)
    bf = mm.batch(mm.compile(f, mm.statemap(g.state2pdf, g.P)))
    P = g.P
    Vh = np.full((P + 1, N + 1), -np.inf, dtype=np.float32)
    Vh[:P, :L] = V[:L].T
    Vh[P, L:] = 0.0
    paths, lps = mm.samplepaths(bf, [Vh], nsamples=32, seed=4)
    assert len(paths) == 1 and paths[0].shape == (32, L) and lps[0].shape == (32,)
    support, logp, _ = sr.enumerate_posterior(gr, V, L)
    _, outside = sr.frequencies(gr, support, paths[0])
    assert outside == 0
    ref, _, _ = bf.samplepaths(V[None].astype(np.float32), [L], nsamples=32, seed=4, want_logprob=True)
    assert np.array_equal(ref[0, :, :L], paths[0])
