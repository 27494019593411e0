"""Lattice posteriors (mm_latticeposteriors_f32) on the MI355X against the float64 restatement of tests/latpost_reference.py.  The
lattices come from BatchedFSM.lattice on the device; the reference always computes over the records the device was given, so no
record is excused.

The bar (latpost_reference.check) is the project's parity bar: on p = exp(post) and on gamma |dp| <= 1e-4 max(p_ref, 1e-6); where
p_ref > 1e-30, |d log p| <= 1e-4 max(1, |log p_ref|); logz to 1e-4 relative; -inf exactly where the reference has -inf; zeros exactly
past len.  Where every cell holds one record and the inputs are multiples of 1/16 the results are exact."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import latpost_reference as lp
import lattice_reference as lr
from test_gpu_lattice import _batch, _bits, _lib
from test_lattice import INF, chain_graph, distinct_case, emissions, entries_case
from test_latticeposteriors import CELL_COUNTS, record_scores, small_graphs
from test_viterbiwindow import on_grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _run(bf, fs, gs, lat, V2, lens, extra=None, what="", want_gamma=True):
    """One call against the reference over the same records; returns (result, reference)."""
    res = bf.latticeposteriors(lat, V2, lens, extra, want_gamma=want_gamma)
    ref = lp.reference(fs, gs, V2, lens, lat.offsets, lat.arc, extra)
    assert res.post.dtype == np.float32 and res.logz.dtype == np.float32 and res.post.shape == lat.arc.shape
    lp.check(res.post, res.logz, res.gamma, ref, what)
    return res, ref


def _raw(mm, torch, bf, Vt, lt, offsets, arc, nrec, extra, post, logz, gamma):
    B, N, P = Vt.shape
    return _lib(mm).lib.mm_latticeposteriors_f32(bf._h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), lt.data_ptr() if lt is not None else None, N,
                                                 offsets.data_ptr(), arc.data_ptr(), nrec, extra.data_ptr() if extra is not None else None,
                                                 post.data_ptr(), logz.data_ptr(), gamma.data_ptr() if gamma is not None else None,
                                                 gamma.stride(0) if gamma is not None else 0, gamma.stride(1) if gamma is not None else 0,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def rand40(mm, wl):
    """The 40-state random graph, B = 3, N = 6, its batch and the beam = inf lattice of V."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    V = emissions(31, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    return g, f, V, bf, bf.lattice(V, INF, None)


@pytest.mark.parametrize("which", [0, 1])
def test_parity_at_the_smallest_shapes(mm, wl, torch, which):
    """A 3-state left-to-right graph and a 40-state random graph, B = 3, N = 6, lens [6, 1, 0] and NULL, beams 0 (weights and
    emissions on the 1/16 grid), 2 and inf, under a V that is not the lattice's, extra NULL and given, gamma NULL and given; then gamma
    through the raw entry into a buffer with strides of its own, whose padding stays untouched."""
    g, f = small_graphs(mm, wl)[which]
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    B, N = 3, 6
    for lens in (np.array([6, 1, 0], dtype=np.int32), None):
        for beam in (0.0, 2.0, INF):
            gg, ff = (gx, fx) if beam == 0.0 else (g, f)
            V = emissions(which + 1, B, N, g.P, rounded=beam == 0.0, scale=1.0)
            V2 = emissions(which + 5, B, N, g.P, rounded=False, scale=1.5)
            bf = _batch(mm, [ff] * B, [gg] * B)
            lat = bf.lattice(V, beam, lens)
            assert lat.arc.size >= (N if lens is None else 0)
            for extra in (None, record_scores(2, lat.arc.size)):
                what = f"{g.name}, lens {None if lens is None else lens.tolist()}, beam {beam}, extra {extra is not None}"
                res, ref = _run(bf, [ff] * B, [gg] * B, lat, V2, lens, extra, what)
                nog = bf.latticeposteriors(lat, V2, lens, extra, want_gamma=False)
                assert nog.gamma is None and _bits(nog.post, res.post) and _bits(nog.logz, res.logz), what
                if lens is not None:
                    assert np.isneginf(res.logz[2]) and (res.gamma[2] == 0).all() and (res.gamma[1, 1:] == 0).all()
    # gamma with strides: [B, N + 1, P + 3]
    Vt = torch.from_numpy(V2).cuda()
    P = g.P
    buf = torch.full((B, N + 1, P + 3), 7.0, device="cuda")
    post = torch.empty(lat.arc.size, device="cuda")
    logz = torch.empty(B, device="cuda")
    offs, arc, ex = torch.from_numpy(lat.offsets).cuda(), torch.from_numpy(lat.arc).cuda(), torch.from_numpy(extra).cuda()
    assert _raw(mm, torch, bf, Vt, None, offs, arc, lat.arc.size, ex, post, logz, buf) == 0
    torch.cuda.synchronize()
    assert _bits(buf[:, :N, :P].cpu().numpy(), res.gamma) and _bits(post.cpu().numpy(), res.post) and _bits(logz.cpu().numpy(), res.logz)
    assert (buf[:, N] == 7.0).all() and (buf[:, :, P:] == 7.0).all()


def _one_pair_fsm(mm, n):
    """One real state with n parallel self-loops of different weights and an arc into the final state: every record of a cell shares
    its source and its destination -- every thread, wave and pass of a step on ONE accumulator."""
    w = -3.0 * np.random.default_rng(n).random(n)
    f = mm.FSM.from_fields([0], [0.0], [0, n, n + 2], [0] * n + [0, 1], np.concatenate([w, [-0.5, 0.0]]).astype(np.float32), [0], semiring="tropical")
    return f, SimpleNamespace(state2pdf=np.array([0], dtype=np.int32), P=2)


@pytest.mark.parametrize("n", CELL_COUNTS)
def test_cell_sizes_around_the_workgroup(mm, wl, torch, n):
    """Cells of exactly n records (n parallel self-loops of one state, beam inf): the wave, workgroup and second-pass edges of the
    forward-backward (1024 threads) and of the per-pdf sums (256), with the worst contention there is -- one target state for the
    whole cell.  Then the FSMs of n stored entries of test_lattice.entries_case: n entries spread over 17 state pairs."""
    f, g = _one_pair_fsm(mm, n)
    B, N = 2, 4
    lens = np.array([4, 3], dtype=np.int32)
    V = emissions(n, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, INF, lens)
    assert (lat.counts[0, :3] == n).all() and lat.counts[0, 3] == 1
    _run(bf, [f] * B, [g] * B, lat, V, lens, None, f"{n} parallel self-loops")
    _run(bf, [f] * B, [g] * B, lat, emissions(n + 1, B, N, g.P, rounded=False), lens, record_scores(n, lat.arc.size, 2.0), f"{n} parallel self-loops, extra")
    if n in (257, 1025):
        f, g, V, lens = entries_case(mm, n)
        B = V.shape[0]
        bf = _batch(mm, [f] * B, [g] * B)
        lat = bf.lattice(V, INF, lens)
        assert lat.counts.max() >= n // 2
        _run(bf, [f] * B, [g] * B, lat, emissions(n + 2, B, V.shape[1], g.P, rounded=False), lens, record_scores(n, lat.arc.size), f"{n} entries")


def test_distinct_graphs_and_a_long_chain(mm, wl, torch):
    """Four different graphs (state and arc offsets per utterance; utterance 1 has no path, its lattice is empty) at beam 2 and
    inf; a chain of 3000 states with N = 5: all but a few of the states in LDS are never touched."""
    gs, fs, V, lens = distinct_case(mm, wl)
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, fs, gs)
    V2 = emissions(22, B, N, 5, rounded=False, scale=1.0)
    for beam in (2.0, INF):
        lat = bf.lattice(V, beam, lens)
        res, _ = _run(bf, fs, gs, lat, V2, lens, record_scores(4, lat.arc.size, 0.5), f"distinct graphs, beam {beam}")
        assert np.isneginf(res.logz[1]) and np.isfinite(res.logz[[0, 2, 3]]).all()
    g = chain_graph(wl, 3000)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 5, 4), np.array([5, 3], dtype=np.int32)
    bf = _batch(mm, [f, f], [g, g])
    lat = bf.lattice(V, 1.0, lens)
    i, _, _ = ar.fsm_entries(f)
    assert (i[lat.arc] > 2900).any() and (i[lat.arc] < 10).any() and lat.arc.size < 200
    res, _ = _run(bf, [f, f], [g, g], lat, emissions(4, 2, 5, 4, rounded=False), lens, None, "chain of 3000")
    assert np.isfinite(res.logz).all()


def test_dead_input(mm, wl, torch, rand40):
    """-inf in V removes records: post is -inf exactly there and the rest is renormalised; a frame that emits nothing removes every
    path of ONE utterance: logz -inf, post -inf, gamma zero, nothing NaN, the other utterances bit for bit what they were; entry
    indices -1, nnz and the phony self-loop's are dead records; nrec below the total is the truncated lattice and nothing at or behind
    post[nrec] is written."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    base, _ = _run(bf, fs, gs, lat, V, None, None, "the lattice's own V")
    assert np.isfinite(base.logz).all() and np.isfinite(base.post).all()
    V2 = V.copy()
    V2[:, 2, 0] = -np.inf
    V2[0, 4, 1:3] = -np.inf
    res, ref = _run(bf, fs, gs, lat, V2, None, None, "-inf in V")
    dead = np.isneginf(res.post)
    assert np.isfinite(res.logz).all() and 0 < dead.sum() < dead.size
    for c in range(B * N):
        lo, hi = lat.offsets[c], lat.offsets[c + 1]
        assert abs(np.exp(res.post[lo:hi].astype(np.float64)).sum() - 1) <= 1e-4, c
    V3 = V.copy()
    V3[1, 3, :] = -np.inf
    res, ref = _run(bf, fs, gs, lat, V3, None, None, "an utterance loses every path")
    lo, hi = lat.offsets[N], lat.offsets[2 * N]
    assert np.isneginf(res.logz[1]) and np.isneginf(res.post[lo:hi]).all() and (res.gamma[1] == 0).all()
    keep = np.r_[0:lo, hi : lat.arc.size]
    assert _bits(res.post[keep], base.post[keep]) and _bits(res.logz[[0, 2]], base.logz[[0, 2]]) and _bits(res.gamma[[0, 2]], base.gamma[[0, 2]])
    # doctored records
    sy = lr.system(f)
    arc = lat.arc.copy()
    at = [int(lat.offsets[1]), int(lat.offsets[N + 2]) + 1, int(lat.offsets[2 * N + 4])]
    arc[at[0]], arc[at[1]], arc[at[2]] = -1, f.nnz, int(np.flatnonzero(sy.phony)[0])
    doctored = mm.Lattice(lat.counts, lat.offsets, arc, lat.score, lat.best)
    res, ref = _run(bf, fs, gs, doctored, V, None, record_scores(8, arc.size, 0.5), "doctored records")
    assert np.isneginf(res.post[at]).all() and np.isfinite(res.logz).all()
    # nrec below the total, through the raw entry
    nrec = int(lat.offsets[N + 3]) + 2  # (utterance 0 whole, utterance 1 cut inside its fourth cell, utterance 2 without records)
    Vt = torch.from_numpy(V).cuda()
    offs, arct = torch.from_numpy(lat.offsets).cuda(), torch.from_numpy(lat.arc).cuda()
    post = torch.full((lat.arc.size,), 7.0, device="cuda")
    logz = torch.empty(B, device="cuda")
    gamma = torch.empty((B, N, g.P), device="cuda")
    assert _raw(mm, torch, bf, Vt, None, offs, arct, nrec, None, post, logz, gamma) == 0
    torch.cuda.synchronize()
    assert (post[nrec:] == 7.0).all()
    ref = lp.reference(fs, gs, V, None, lat.offsets, lat.arc, None, nrec=nrec)
    lp.check(post[:nrec].cpu().numpy(), logz.cpu().numpy(), gamma.cpu().numpy(), ref, "nrec below the total")
    assert _bits(logz[:1].cpu().numpy(), base.logz[:1]) and np.isneginf(logz[1:].cpu().numpy()).all()
    # offsets that decrease, are negative or reach behind nrec: clamped
    bad = lat.offsets.copy()
    bad[0], bad[N + 2], bad[2 * N + 1] = -5, bad[N + 1] - 3, 2 ** 40  # (utterance 0 keeps its records; utterance 1 loses a cell)
    post.fill_(7.0)
    assert _raw(mm, torch, bf, Vt, None, torch.from_numpy(bad).cuda(), arct, nrec, None, post, logz, gamma) == 0
    torch.cuda.synchronize()
    assert (post[nrec:] == 7.0).all()
    ref = lp.reference(fs, gs, V, None, bad, lat.arc, None, nrec=nrec)
    lp.check(post[:nrec].cpu().numpy(), logz.cpu().numpy(), gamma.cpu().numpy(), ref, "clamped offsets")
    assert _bits(logz[:1].cpu().numpy(), base.logz[:1]) and np.isneginf(logz[1:].cpu().numpy()).all()


def test_exactness_where_it_exists(mm, wl, torch):
    """Weights and emissions on the 1/16 grid, beam 0, a unique best path: every cell holds one record, and with extra NULL and the
    lattice's own V post is exactly 0, gamma exactly 0 / 1 and logz the lattice's best, bit for bit."""
    g = on_grid(small_graphs(mm, wl)[1][0])
    f = wl.to_fsm(mm, g, semiring="tropical")
    B, N = 3, 8
    lens = np.array([8, 5, 0], dtype=np.int32)
    V = emissions(0, B, N, g.P)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, 0.0, lens)
    assert np.array_equal(lat.counts, (np.arange(N)[None] < lens[:, None]).astype(np.int32))
    res = bf.latticeposteriors(lat, V, lens)
    assert (res.post == 0).all() and res.post.size == 13 and _bits(res.logz, lat.best) and np.isneginf(res.logz[2])
    i, _, _ = ar.fsm_entries(f)
    want = np.zeros((B, N, g.P), dtype=np.float32)
    for b in range(B):
        for t in range(int(lens[b])):
            want[b, t, g.state2pdf[i[lat.arc[lat.offsets[b * N + t]]]]] = 1.0
    assert _bits(res.gamma, want)


def test_cross_check_with_pdfposteriors(mm, wl, torch, rand40):
    """An independent kernel: at beam = inf under the same V the lattice holds every arc with a finite score, so logz and gamma are
    those of pdfposteriors on a log batch of the same arcs.  Both sides are float32 kernels held to 1e-4 against float64: they agree
    within 2e-4 (logz relative, gamma relative to max(gamma, 1e-6))."""
    g, f, V, bf, lat = rand40
    B = V.shape[0]
    res = bf.latticeposteriors(lat, V)
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    gamma, ttl = lb.pdfposteriors(V)
    dz = np.abs(res.logz.astype(np.float64) - ttl) / np.abs(ttl)
    dg = np.abs(res.gamma.astype(np.float64) - gamma) / np.maximum(gamma, 1e-6)
    print(f"against pdfposteriors: |dlogz| {dz.max():.3g}, |dgamma| {dg.max():.3g}")
    assert np.isfinite(ttl).all() and dz.max() <= 2e-4 and dg.max() <= 2e-4


def test_bit_identity(mm, wl, torch):
    """Two calls return the same bits in post, logz and gamma: 257 parallel entries on one accumulator, unrounded inputs."""
    f, g = _one_pair_fsm(mm, 257)
    B, N = 2, 4
    V = emissions(1, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, INF, None)
    extra = record_scores(5, lat.arc.size)
    a = bf.latticeposteriors(lat, V, None, extra)
    for _ in range(3):
        b = bf.latticeposteriors(lat, V, None, extra)
        assert _bits(a.post, b.post) and _bits(a.logz, b.logz) and _bits(a.gamma, b.gamma)
    assert np.isfinite(a.post).all() and lat.arc.size == 2 * (3 * 257 + 1)


def test_graph_capture(mm, wl, torch, rand40):
    """A capture before a first call is refused with MM_ERR_INVALID (the arc table is not made during a capture); a capture after it
    replays, and follows V and extra overwritten in place."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    Vt = torch.from_numpy(V).cuda()
    et = torch.zeros(lat.arc.size, device="cuda")
    fresh = _batch(mm, fs, gs)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.latticeposteriors(tl, Vt, None, et)
    assert ei.value.code == -1, str(ei.value)
    first = fresh.latticeposteriors(tl, Vt, None, et)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fresh.latticeposteriors(tl, Vt, None, et)
    for seed in (41, 42):
        Vn, en = emissions(seed, B, N, g.P, rounded=False, scale=1.0), record_scores(seed, lat.arc.size)
        Vt.copy_(torch.from_numpy(Vn).cuda())
        et.copy_(torch.from_numpy(en).cuda())
        out.post.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        ref = lp.reference(fs, gs, Vn, None, lat.offsets, lat.arc, en)
        lp.check(out.post.cpu().numpy(), out.logz.cpu().numpy(), out.gamma.cpu().numpy(), ref, f"replay {seed}")
        again = fresh.latticeposteriors(tl, Vt, None, et)
        assert torch.equal(again.post, out.post) and torch.equal(again.logz, out.logz) and torch.equal(again.gamma, out.gamma)
    assert np.isfinite(first.logz.cpu().numpy()).all()


def test_limits_and_refusals(mm, wl, torch, rand40):
    """A chain one step over the state cap of the LDS is refused with MM_ERR_UNSUPPORTED and the cap in the message; the largest
    that fits runs and matches; log batches are refused; kernels() names the launches; a lattice cut by max_arcs and an extra of
    the wrong length raise."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    k = bf.kernels("latticeposteriors")
    assert "mm_latpost_fb_kernel<1024>" in k and "mm_latpost_gamma_kernel<256>" in k and "exceed" not in k, k
    cap = int(re.search(r"state cap (\d+)", k).group(1))
    assert 10000 < cap and 64 + 16 * cap <= 160 * 1024 < 64 + 16 * (cap + 4)
    Vc, lens = emissions(3, 2, 3, 4), np.array([3, 2], dtype=np.int32)
    for S, fits in ((cap - 4, True), (cap, False)):  # (the padded count is S + 2 rounded up to a multiple of 4)
        gc = chain_graph(wl, S)
        fc = wl.to_fsm(mm, gc, semiring="tropical")
        bc = _batch(mm, [fc, fc], [gc, gc])
        latc = bc.lattice(Vc, 1.0, lens)
        assert ("exceed" in bc.kernels("latticeposteriors")) == (not fits)
        if fits:
            res, _ = _run(bc, [fc, fc], [gc, gc], latc, emissions(4, 2, 3, 4, rounded=False), lens, None, f"chain of {S}")
            assert np.isfinite(res.logz).all()
        else:
            with pytest.raises(mm.MarkovModelsAMDError) as ei:
                bc.latticeposteriors(latc, Vc, lens)
            assert ei.value.code == -4 and str(cap) in str(ei.value), str(ei.value)
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        lb.latticeposteriors(lat, V)
    assert ei.value.code == -4 and "tropical" in str(ei.value)
    with pytest.raises(mm.MarkovModelsAMDError):
        lb.kernels("latticeposteriors")
    with pytest.raises(TypeError):
        mm.latticeposteriors(lb, lat, [np.zeros((g.P + 1, N + 1), dtype=np.float32)] * B)
    cut = mm.Lattice(lat.counts, lat.offsets, lat.arc[:-3], lat.score[:-3], lat.best)
    with pytest.raises(ValueError):
        bf.latticeposteriors(cut, V)
    with pytest.raises(mm.DimensionMismatch):
        bf.latticeposteriors(lat, V, None, np.zeros(lat.arc.size - 1, dtype=np.float32))
    with pytest.raises(mm.DimensionMismatch):
        bf.latticeposteriors(mm.Lattice(lat.counts, lat.offsets[:-1], lat.arc, lat.score, lat.best), V)
    # the module-level call, in lattice's call shape
    res = mm.latticeposteriors(bf, lat, [mm.expand(V[b].T, N, "tropical") for b in range(B)])
    lp.check(res.post, res.logz, res.gamma, lp.reference([f] * B, [g] * B, V, None, lat.offsets, lat.arc), "module level")


def test_lattice_loglik_gradients(mm, wl, torch):
    """lattices.lattice_loglik: the gradients of sum_b c_b logz_b against V and extra are c_b gamma_b and c_b exp(post) of the
    float64 restatement (whose own gradients the CPU tests check by finite differences), at the bar of gamma and of p; zero for the
    utterance without a path, whatever its c."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    V = emissions(12, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, 4.0, lens)
    V2 = emissions(13, B, N, g.P, rounded=False, scale=1.0)
    V2[2, 3, :] = -np.inf  # (utterance 2 loses every path under the second model)
    extra = record_scores(6, lat.arc.size, 0.5)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    Vt = torch.from_numpy(V2).cuda().requires_grad_(True)
    et = torch.from_numpy(extra).cuda().requires_grad_(True)
    lt = torch.from_numpy(lens).cuda()
    logz = mm.lattices.lattice_loglik(bf, tl, Vt, et, lt)
    c = np.array([1.5, -2.0, 3.0], dtype=np.float32)
    logz.backward(torch.from_numpy(c).cuda())
    ref = lp.reference([f] * B, [g] * B, V2, lens, lat.offsets, lat.arc, extra)
    assert np.isneginf(ref.logz[2]) and np.isfinite(ref.logz[:2]).all()
    got = logz.detach().cpu().numpy()
    assert np.isneginf(got[2]) and (np.abs(got[:2] - ref.logz[:2]) <= 1e-4 * np.abs(ref.logz[:2])).all()
    gV, gE = Vt.grad.cpu().numpy().astype(np.float64), et.grad.cpu().numpy().astype(np.float64)
    owner = np.searchsorted(lat.offsets[::N][:B], np.arange(lat.arc.size), side="right") - 1
    wantV = ref.gamma * c[:, None, None]
    wantE = np.where(np.isneginf(ref.post), 0.0, np.exp(ref.post)) * c[owner]
    assert (gV[2] == 0).all() and (gE[owner == 2] == 0).all() and not np.isnan(gV).any() and not np.isnan(gE).any()
    assert (np.abs(gV - wantV) <= 1e-4 * np.abs(c)[:, None, None] * np.maximum(ref.gamma, 1e-6)).all()
    assert (np.abs(gE - wantE) <= 1e-4 * np.abs(c[owner]) * np.maximum(np.abs(wantE / c[owner]), 1e-6)).all()
    # without extra: one gradient
    Vt2 = torch.from_numpy(V2).cuda().requires_grad_(True)
    mm.lattice_loglik(bf, tl, Vt2, None, lt)[:2].sum().backward()
    ref0 = lp.reference([f] * B, [g] * B, V2, lens, lat.offsets, lat.arc)
    assert (np.abs(Vt2.grad.cpu().numpy()[:2] - ref0.gamma[:2]) <= 1e-4 * np.maximum(ref0.gamma[:2], 1e-6)).all() and (Vt2.grad[2] == 0).all()


def test_lattice_prune_round_trip(mm, wl, torch, rand40):
    """decode.lattice_prune on device tensors: the pruned lattice goes back into latticeposteriors and equals the reference over the
    pruned records; lattice_arcs reads it and lattice_fsm's graph of it still compiles and decodes."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    V2 = emissions(51, B, N, g.P, rounded=False, scale=1.0)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    res = bf.latticeposteriors(tl, torch.from_numpy(V2).cuda())
    pr = mm.decode.lattice_prune(tl, res.post, 0.02)
    assert all(x.is_cuda for x in pr[:4]) and 0 < pr.arc.numel() < lat.arc.size and int(pr.offsets[-1]) == pr.arc.numel()
    host = mm.Lattice(*(x.cpu().numpy() for x in pr))
    keep = res.post.cpu().numpy() >= np.float32(np.log(0.02))
    assert np.array_equal(host.arc, lat.arc[keep]) and host.counts.sum() == keep.sum()
    again, _ = _run(bf, fs, gs, host, V2, None, None, "the pruned lattice")
    assert np.isfinite(again.logz).all() and (again.logz <= res.logz.cpu().numpy() + 1e-5).all()
    t, k, src, dst, s = mm.decode.lattice_arcs(bf, host, 1)
    assert k.size == host.counts[1].sum()
    lf, s2p = mm.decode.lattice_fsm(bf, host, 1)
    lb = mm.batch(mm.compile(lf, mm.statemap(s2p, g.P)))
    _, sc = lb.viterbi(np.ascontiguousarray(V[1:2]), None)
    assert np.isfinite(sc).all() and sc[0] <= lat.best[1]  # (a path of the pruned graph is a path of the graph)
