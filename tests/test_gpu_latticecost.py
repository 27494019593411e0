"""Lattice expected cost (mm_latticecost_f32) on the MI355X against the float64 restatement of tests/latcost_reference.py.  The
lattices come from BatchedFSM.lattice on the device; the reference always computes over the records the device was given.

The bars (latcost_reference.check): risk within 1e-4 sum_r exp(post_ref) |cost| + 1e-6 L max |cost|; diff and grad within
1e-4 |ref| + a G_b, G_b the utterance's largest |ref| of that output and a = latcost_reference.DIFF_ABS_A, ten times the float32 floor
measured on the CPU (profiles/latticecost_floor.json); post, logz and gamma by latpost_reference.check and bit for bit those of
mm_latticeposteriors_f32; exact zeros where the reference has them.  Where every cell holds one record and the costs are multiples
of 1/16 the risk is the exact sum and diff and grad are exactly 0."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import cost_reference as cr
import latcost_reference as lc
import lattice_reference as lr
from test_gpu_lattice import _batch, _bits, _lib
from test_gpu_parity import _with_env
from test_lattice import INF, chain_graph, distinct_case, emissions, entries_case, grid
from test_latticecost import SHIFT, cell_case, risk_case, shift_case, smallest_cases
from test_latticeposteriors import CELL_COUNTS, record_scores, small_graphs
from test_viterbiwindow import on_grid

pytestmark = pytest.mark.gpu
FIELDS = ("risk", "diff", "post", "logz", "grad", "gamma")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _run(bf, fs, gs, lat, V2, lens, cost, extra=None, what="", same_as_posteriors=True):
    """One call with grad and gamma against the reference over the same records; returns (result, reference)."""
    res = bf.latticecost(lat, V2, cost, lens, extra, want_grad=True, want_gamma=True)
    ref = lc.reference(fs, gs, V2, lens, lat.offsets, lat.arc, cost, extra)
    assert all(getattr(res, k).dtype == np.float32 for k in FIELDS) and res.diff.shape == lat.arc.shape and res.post.shape == lat.arc.shape
    lc.check(res, ref, cost, lens, lat.offsets, what)
    if same_as_posteriors:
        base = bf.latticeposteriors(lat, V2, lens, extra)
        assert _bits(res.post, base.post) and _bits(res.logz, base.logz) and _bits(res.gamma, base.gamma), what
    return res, ref


def _raw(mm, torch, bf, Vt, lt, offsets, arc, nrec, extra, cost, risk, diff, post, logz, grad, gamma):
    B, N, P = Vt.shape
    s = grad if grad is not None else gamma
    ptr = lambda t: t.data_ptr() if t is not None else None
    return _lib(mm).lib.mm_latticecost_f32(bf._h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), ptr(lt), N, offsets.data_ptr(), arc.data_ptr(), nrec, ptr(extra),
                                           ptr(cost), risk.data_ptr(), ptr(diff), ptr(post), logz.data_ptr(), ptr(grad), ptr(gamma),
                                           s.stride(0) if s is not None else 0, s.stride(1) if s is not None else 0,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _identities(res, cost, lat, lens, N, what):
    """The header's identities on the device's own outputs, each within the summed bars of its terms: a cell's diff and a row of
    grad sum to 0 within (terms) x (1e-4 + a) x the largest |diff| of the utterance; risk = sum exp(post) cost within the risk's bar
    plus 1e-4 of the sum of the terms' magnitudes."""
    B = res.risk.size
    own = lc.owners(lat.offsets, lat.arc.size, B, N)
    a = lc.DIFF_ABS_A
    d = res.diff.astype(np.float64)
    p = np.exp(res.post.astype(np.float64))
    c = cost.astype(np.float64)
    for b in range(B):
        m = own == b
        G = float(np.abs(d[m]).max()) if m.any() else 0.0
        L = N if lens is None else int(min(max(lens[b], 0), N))
        for t in range(N):
            lo, hi = lat.offsets[b * N + t], lat.offsets[b * N + t + 1]
            assert abs(d[lo:hi].sum()) <= (hi - lo) * (1e-4 + a) * G, (what, b, t)
            assert abs(res.grad[b, t].astype(np.float64).sum()) <= (hi - lo + 1) * (1e-4 + a) * G, (what, b, t)
        terms = float((p[m] * np.abs(c[m])).sum())
        bar = 2e-4 * terms + 1e-6 * L * (float(np.abs(c[m]).max()) if m.any() else 0.0)
        assert abs(res.risk[b] - float((p[m] * c[m]).sum())) <= bar, (what, b, res.risk[b], float((p[m] * c[m]).sum()), bar)


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
    """A 3-state left-to-right graph and a 40-state random graph, B = 3, N = 6, lens [6, 1, 0] and NULL, beams 0 (weights, emissions
    and costs on the 1/16 grid: risk the exact sum, diff and grad exactly 0), 2 and inf, under a V that is not the lattice's, extra
    NULL and given, grad / gamma NULL and given; then grad and gamma through the raw entry into buffers with strides of their own,
    whose padding stays untouched."""
    B, N = 3, 6
    for what, fs, gs, V, V2, lens, beam in smallest_cases(mm, wl, which):
        bf = _batch(mm, fs, gs)
        lat = bf.lattice(V, beam, lens)
        cost = record_scores(3, lat.arc.size)
        cost = grid(cost) if beam == 0.0 else cost
        for extra in (None, record_scores(2, lat.arc.size)):
            res, ref = _run(bf, fs, gs, lat, V2, lens, cost, extra, f"{what}, extra {extra is not None}")
            _identities(res, cost, lat, lens, N, what)
            for wg, wm in ((False, False), (True, False), (False, True)):
                part = bf.latticecost(lat, V2, cost, lens, extra, want_grad=wg, want_gamma=wm)
                assert (part.grad is None) == (not wg) and (part.gamma is None) == (not wm)
                assert all(getattr(part, k) is None or _bits(getattr(part, k), getattr(res, k)) for k in FIELDS), what
            if lens is not None:
                assert np.isneginf(res.logz[2]) and res.risk[2] == 0 and (res.grad[2] == 0).all() and (res.grad[1, 1:] == 0).all()
            if beam == 0.0:
                own = lc.owners(lat.offsets, lat.arc.size, B, N)
                assert (res.diff == 0).all() and (res.grad == 0).all()
                assert all(res.risk[b] == np.float32(cost[own == b].astype(np.float64).sum()) for b in range(B)), (what, res.risk)
    # grad and gamma with strides: [B, N + 1, P + 3], one pair of strides for both
    P = gs[0].P
    Vt = torch.from_numpy(V2).cuda()
    bufs = [torch.full((B, N + 1, P + 3), 7.0, device="cuda") for _ in range(2)]
    risk, logz = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    diff, post = torch.empty(lat.arc.size, device="cuda"), torch.empty(lat.arc.size, device="cuda")
    offs, arc, ex, ct = (torch.from_numpy(x).cuda() for x in (lat.offsets, lat.arc, extra, cost))
    assert _raw(mm, torch, bf, Vt, None, offs, arc, lat.arc.size, ex, ct, risk, diff, post, logz, bufs[0], bufs[1]) == 0
    torch.cuda.synchronize()
    assert _bits(bufs[0][:, :N, :P].cpu().numpy(), res.grad) and _bits(bufs[1][:, :N, :P].cpu().numpy(), res.gamma)
    assert _bits(diff.cpu().numpy(), res.diff) and _bits(risk.cpu().numpy(), res.risk) and _bits(post.cpu().numpy(), res.post)
    assert all((buf[:, N] == 7.0).all() and (buf[:, :, P:] == 7.0).all() for buf in bufs)


def _cells(mm, bf, n, what):
    fs, gs, V, V2, lens = cell_case(mm, n)
    lat = bf.lattice(V, INF, lens)
    assert (lat.counts[0, :3] == n).all() and lat.counts[0, 3] == 1
    res, _ = _run(bf, fs, gs, lat, V, lens, record_scores(n + 7, lat.arc.size), None, f"{n} parallel self-loops{what}")
    _run(bf, fs, gs, lat, V2, lens, record_scores(n + 8, lat.arc.size), record_scores(n, lat.arc.size, 2.0), f"{n} parallel self-loops, extra{what}")
    return res


@pytest.mark.parametrize("n", CELL_COUNTS)
def test_cell_sizes_around_the_workgroup(mm, wl, torch, n):
    """Cells of exactly n records (n parallel self-loops of one state, beam inf), signed costs: the wave, workgroup and second-turn
    edges of the forward-backward (1024 threads) and of the per-pdf sums (256), one target state -- one probability sum and one
    signed cost sum -- under the whole cell.  Then the FSMs of n stored entries of test_lattice.entries_case."""
    fs, gs, _, _, _ = cell_case(mm, n)
    _cells(mm, _batch(mm, fs, gs), n, "")
    if n in (257, 1025):
        f, g, V, lens = entries_case(mm, n)
        B = V.shape[0]
        bf = _batch(mm, [f] * B, [g] * B)
        lat = bf.lattice(V, INF, lens)
        assert lat.counts.max() >= n // 2
        cost = record_scores(n + 7, lat.arc.size)
        res, _ = _run(bf, [f] * B, [g] * B, lat, emissions(n + 2, B, V.shape[1], g.P, rounded=False), lens, cost, record_scores(n, lat.arc.size), f"{n} entries")
        _identities(res, cost, lat, lens, V.shape[1], f"{n} entries")


@pytest.mark.parametrize("nt", [256, 512, 1024])
def test_thread_counts(mm, wl, torch, nt):
    """The three instances of the forward-backward (MM_LATPOST_NT under MM_DEBUG, read when the batch is made), each in a fresh
    batch, on the cells of 257 and 1025 records: one, two and five turns of a thread over a cell.  All three return the same bits
    (nothing depends on which thread holds a record), and kernels() names the instance."""
    out = []
    for n in (257, 1025):
        fs, gs, _, _, _ = cell_case(mm, n)
        bf = _with_env({"MM_DEBUG": "1", "MM_LATPOST_NT": str(nt)}, lambda: _batch(mm, fs, gs))
        k = bf.kernels("latticecost")
        assert f"mm_latcost_fb_kernel<{nt}>" in k and "mm_latcost_grad_kernel<256>" in k and "exceed" not in k, k
        res = _cells(mm, bf, n, f", {nt} threads")
        base = _cells(mm, _batch(mm, fs, gs), n, ", the default")
        assert all(_bits(getattr(res, key), getattr(base, key)) for key in FIELDS), (n, nt)


def test_distinct_graphs_and_a_long_chain(mm, wl, torch):
    """Four different graphs (state and arc offsets per utterance; utterance 1 has no path: risk 0 and every output zero) at beam 2
    and inf; a chain of 3000 states with N = 5: all but a few of the states in LDS are never touched."""
    gs, fs, V, lens = distinct_case(mm, wl)
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, fs, gs)
    V2 = emissions(22, B, N, 5, rounded=False, scale=1.0)
    for beam in (2.0, INF):
        lat = bf.lattice(V, beam, lens)
        cost = record_scores(14, lat.arc.size)
        res, _ = _run(bf, fs, gs, lat, V2, lens, cost, record_scores(4, lat.arc.size, 0.5), f"distinct graphs, beam {beam}")
        assert np.isneginf(res.logz[1]) and res.risk[1] == 0 and (res.grad[1] == 0).all() and (res.gamma[1] == 0).all()
        assert np.isfinite(res.logz[[0, 2, 3]]).all() and (res.diff[lc.owners(lat.offsets, lat.arc.size, B, N) == 1] == 0).all()
        _identities(res, cost, lat, lens, N, f"distinct graphs, beam {beam}")
    g = chain_graph(wl, 3000)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 5, 4), np.array([5, 3], dtype=np.int32)
    bf = _batch(mm, [f, f], [g, g])
    lat = bf.lattice(V, 1.0, lens)
    i, _, _ = ar.fsm_entries(f)
    assert (i[lat.arc] > 2900).any() and (i[lat.arc] < 10).any() and lat.arc.size < 200
    res, _ = _run(bf, [f, f], [g, g], lat, emissions(4, 2, 5, 4, rounded=False), lens, record_scores(5, lat.arc.size), None, "chain of 3000")
    assert np.isfinite(res.logz).all()


def test_bit_identity(mm, wl, torch):
    """Four calls return the same bits in all six outputs: 257 parallel entries on one accumulator, unrounded inputs, signed costs."""
    fs, gs, V, _, _ = cell_case(mm, 257)
    bf = _batch(mm, fs, gs)
    lat = bf.lattice(V, INF, None)
    extra, cost = record_scores(5, lat.arc.size), record_scores(6, lat.arc.size)
    a = bf.latticecost(lat, V, cost, None, extra, want_grad=True, want_gamma=True)
    for _ in range(3):
        b = bf.latticecost(lat, V, cost, None, extra, want_grad=True, want_gamma=True)
        assert all(_bits(getattr(a, k), getattr(b, k)) for k in FIELDS)
    assert np.isfinite(a.diff).all() and np.abs(a.diff).max() > 0 and lat.arc.size == 2 * (3 * 257 + 1)


def test_shift_of_the_costs(mm, wl, torch):
    """Centring: the 40-state graph, B = 2, N = 200, beam 3, costs c and c + 64 per record.  A path's cost grows to 64 x 200; the
    risk shifts by 64 len within the risk's bar, and diff and grad of the shifted call meet the bar against the reference of the
    UNSHIFTED costs -- the same G_b, the shift does not enter it.  (A recursion that carried ca and cb uncentred in float32 would
    lose 2^-24 x 12 800 = 7.6e-4 of a diff of order 1.)"""
    fs, gs, V, lens, beam = shift_case(mm, wl)
    bf = _batch(mm, fs, gs)
    lat = bf.lattice(V, beam, lens)
    c = record_scores(62, lat.arc.size)
    res, ref = _run(bf, fs, gs, lat, V, lens, c, None, "N = 200, beam 3")
    assert lat.arc.size > 5000 and np.isfinite(res.logz).all()
    shifted = bf.latticecost(lat, V, c + np.float32(SHIFT), lens, want_grad=True, want_gamma=True)
    want = SimpleNamespace(**{**vars(ref), "risk": ref.risk + SHIFT * lens})
    lc.check(shifted, want, c + np.float32(SHIFT), lens, lat.offsets, "N = 200, beam 3, costs + 64")
    _identities(shifted, c + np.float32(SHIFT), lat, lens, V.shape[1], "costs + 64")


def test_cross_check_with_expectedcost(mm, wl, torch, rand40):
    """An independent kernel: at beam = inf with cost = pdf_costs(D) the risk and its gradient against V are mm_expectedcost_f32's
    on a log batch of the same arcs.  Both sides are float32 kernels held to their bars against float64: they agree within the sum
    of the two bars (risk: 2 x (1e-4 sum gamma |D| + 1e-6 L max |D|); grad: 2e-4 |grad| + (a_lattice + a_item) G_b)."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    D = np.random.default_rng(8).standard_normal((B, N, g.P)).astype(np.float32)
    idx = mm.lattices.record_index(bf, lat)
    cost = mm.lattices.pdf_costs(idx, D)
    res = bf.latticecost(lat, V, cost, want_gamma=True)
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    risk, grad, ttl = lb.expectedcost(V, D)
    for b in range(B):
        bar = 2 * (1e-4 * float((res.gamma[b].astype(np.float64) * np.abs(D[b])).sum()) + 1e-6 * N * float(np.abs(D[b]).max()))
        G = float(np.abs(grad[b]).max())
        e = np.abs(res.grad[b].astype(np.float64) - grad[b])
        print(f"against expectedcost, b = {b}: |drisk| {abs(float(res.risk[b]) - float(risk[b])):.3g} (bar {bar:.3g}), |dgrad| / G {e.max() / G:.3g}")
        assert abs(float(res.risk[b]) - float(risk[b])) <= bar
        assert (e <= 2e-4 * np.abs(grad[b]) + (lc.DIFF_ABS_A + cr.GRAD_ABS_A) * G).all()
        assert abs(float(res.logz[b]) - float(ttl[b])) <= 2e-4 * abs(float(ttl[b]))


def test_dead_input(mm, wl, torch, rand40):
    """Doctored values: entry indices -1, nnz and the phony self-loop's are dead records (diff 0, post -inf); nrec below the total is
    the truncated lattice and nothing at or behind nrec is written; offsets that decrease, are negative or reach behind nrec are
    clamped; lens beyond N are N; a frame that emits nothing removes every path of ONE utterance and leaves the others bit for bit
    what they were; Python refuses a lattice cut by max_arcs."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    cost = record_scores(21, lat.arc.size)
    base, _ = _run(bf, fs, gs, lat, V, None, cost, None, "the lattice's own V")
    V3 = V.copy()
    V3[1, 3, :] = -np.inf
    res, _ = _run(bf, fs, gs, lat, V3, None, cost, None, "an utterance loses every path")
    lo, hi = lat.offsets[N], lat.offsets[2 * N]
    assert np.isneginf(res.logz[1]) and res.risk[1] == 0 and (res.diff[lo:hi] == 0).all() and (res.grad[1] == 0).all()
    keep = np.r_[0:lo, hi : lat.arc.size]
    assert _bits(res.diff[keep], base.diff[keep]) and _bits(res.risk[[0, 2]], base.risk[[0, 2]]) and _bits(res.grad[[0, 2]], base.grad[[0, 2]])
    big, _ = _run(bf, fs, gs, lat, V, np.array([N + 5, N, 2 ** 30], dtype=np.int32), cost, None, "lens beyond N")
    assert all(_bits(getattr(big, k), getattr(base, k)) for k in FIELDS)
    sy = lr.system(f)
    arc = lat.arc.copy()
    at = [int(lat.offsets[1]), int(lat.offsets[N + 2]) + 1, int(lat.offsets[2 * N + 4])]
    arc[at[0]], arc[at[1]], arc[at[2]] = -1, f.nnz, int(np.flatnonzero(sy.phony)[0])
    doctored = mm.Lattice(lat.counts, lat.offsets, arc, lat.score, lat.best)
    res, _ = _run(bf, fs, gs, doctored, V, None, cost, record_scores(8, arc.size, 0.5), "doctored records")
    assert np.isneginf(res.post[at]).all() and (res.diff[at] == 0).all() and np.isfinite(res.logz).all()
    # nrec below the total, through the raw entry: a lattice cut by max_arcs
    nrec = int(lat.offsets[N + 3]) + 2  # (utterance 0 whole, utterance 1 cut inside its fourth cell, utterance 2 without records)
    Vt = torch.from_numpy(V).cuda()
    offs, arct, ct = torch.from_numpy(lat.offsets).cuda(), torch.from_numpy(lat.arc).cuda(), torch.from_numpy(cost).cuda()
    post, diff = torch.full((lat.arc.size,), 7.0, device="cuda"), torch.full((lat.arc.size,), 7.0, device="cuda")
    risk, logz = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    grad, gamma = torch.empty((B, N, g.P), device="cuda"), torch.empty((B, N, g.P), device="cuda")
    for what, o in (("nrec below the total", lat.offsets), ("clamped offsets", None)):
        if o is None:
            o = lat.offsets.copy()
            o[0], o[N + 2], o[2 * N + 1] = -5, o[N + 1] - 3, 2 ** 40  # (utterance 0 keeps its records; utterance 1 loses a cell)
        post.fill_(7.0)
        diff.fill_(7.0)
        assert _raw(mm, torch, bf, Vt, None, torch.from_numpy(o).cuda(), arct, nrec, None, ct, risk, diff, post, logz, grad, gamma) == 0
        torch.cuda.synchronize()
        assert (post[nrec:] == 7.0).all() and (diff[nrec:] == 7.0).all()
        ref = lc.reference(fs, gs, V, None, o, lat.arc, cost, None, nrec=nrec)
        got = SimpleNamespace(risk=risk.cpu().numpy(), diff=diff.cpu().numpy(), post=post.cpu().numpy(), logz=logz.cpu().numpy(), grad=grad.cpu().numpy(),
                              gamma=gamma.cpu().numpy())
        lc.check(got, ref, cost, None, o, what)
        assert _bits(got.risk[:1], base.risk[:1]) and _bits(got.grad[0], base.grad[0]) and np.isneginf(got.logz[1:]).all() and (got.risk[1:] == 0).all()
    cut = mm.Lattice(lat.counts, lat.offsets, lat.arc[:-3], lat.score[:-3], lat.best)
    with pytest.raises(ValueError):
        bf.latticecost(cut, V, cost[:-3])
    with pytest.raises(mm.DimensionMismatch):
        bf.latticecost(lat, V, cost[:-1])


def test_limits_and_refusals(mm, wl, torch, rand40):
    """kernels() names the launches, the bytes per state and the state cap, which satisfies the LDS formula against 160 KB and
    covers config 5's 5004 padded states; a chain at the cap runs and matches, four padded states more are refused with
    MM_ERR_UNSUPPORTED and the cap in the message; log batches are refused; the module-level call."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    k = bf.kernels("latticecost")
    assert "mm_latcost_fb_kernel<1024>" in k and "mm_latcost_grad_kernel<256>" in k and "exceed" not in k, k
    cap, per = int(re.search(r"state cap (\d+)", k).group(1)), int(re.search(r"(\d+) bytes of LDS per state", k).group(1))
    assert per == 28 and 80 + per * cap <= 160 * 1024 < 80 + per * (cap + 4) and 5004 <= cap and cap % 4 == 0
    Vc, lens = emissions(3, 2, 3, 4), np.array([3, 2], dtype=np.int32)
    for S, fits in ((cap - 4, True), (cap, False)):  # (the padded count is S + 2 rounded up to a multiple of 4)
        gc = chain_graph(wl, S)
        fc = wl.to_fsm(mm, gc, semiring="tropical")
        bc = _batch(mm, [fc, fc], [gc, gc])
        latc = bc.lattice(Vc, 1.0, lens)
        assert ("exceed" in bc.kernels("latticecost")) == (not fits) and "exceed" not in bc.kernels("latticeposteriors")
        cost = record_scores(S, latc.arc.size)
        if fits:
            res, _ = _run(bc, [fc, fc], [gc, gc], latc, emissions(4, 2, 3, 4, rounded=False), lens, cost, None, f"chain of {S}")
            assert np.isfinite(res.logz).all()
        else:
            with pytest.raises(mm.MarkovModelsAMDError) as ei:
                bc.latticecost(latc, Vc, cost, lens)
            assert ei.value.code == -4 and str(cap) in str(ei.value), str(ei.value)
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    cost = record_scores(1, lat.arc.size)
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        lb.latticecost(lat, V, cost)
    assert ei.value.code == -4 and "tropical" in str(ei.value)
    with pytest.raises(mm.MarkovModelsAMDError):
        lb.kernels("latticecost")
    with pytest.raises(TypeError):
        mm.latticecost(lb, lat, [np.zeros((g.P + 1, N + 1), dtype=np.float32)] * B, cost)
    res = mm.latticecost(bf, lat, [mm.expand(V[b].T, N, "tropical") for b in range(B)], cost)
    assert res.gamma is None
    lc.check(res, lc.reference([f] * B, [g] * B, V, None, lat.offsets, lat.arc, cost), cost, None, lat.offsets, "module level")


def test_graph_capture(mm, wl, torch, rand40):
    """A capture before a first call is refused with MM_ERR_INVALID (the arc table is not made during a capture); a capture after it
    replays, and follows V, extra and cost overwritten in place."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    Vt = torch.from_numpy(V).cuda()
    et, ct = torch.zeros(lat.arc.size, device="cuda"), torch.ones(lat.arc.size, device="cuda")
    fresh = _batch(mm, fs, gs)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.latticecost(tl, Vt, ct, None, et)
    assert ei.value.code == -1, str(ei.value)
    first = fresh.latticecost(tl, Vt, ct, None, et, want_gamma=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fresh.latticecost(tl, Vt, ct, None, et, want_gamma=True)
    for seed in (41, 42):
        Vn, en, cn = emissions(seed, B, N, g.P, rounded=False, scale=1.0), record_scores(seed, lat.arc.size), record_scores(seed + 9, lat.arc.size)
        Vt.copy_(torch.from_numpy(Vn).cuda())
        et.copy_(torch.from_numpy(en).cuda())
        ct.copy_(torch.from_numpy(cn).cuda())
        out.diff.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        ref = lc.reference(fs, gs, Vn, None, lat.offsets, lat.arc, cn, en)
        lc.check(SimpleNamespace(**{k: getattr(out, k).cpu().numpy() for k in FIELDS}), ref, cn, None, lat.offsets, f"replay {seed}")
        again = fresh.latticecost(tl, Vt, ct, None, et, want_gamma=True)
        assert all(torch.equal(getattr(again, k), getattr(out, k)) for k in FIELDS)
    assert np.allclose(first.risk.cpu().numpy(), N, rtol=0, atol=1e-4)  # (a cost of 1 per record: the risk is the length)


def test_lattice_risk_gradients_and_smbr(mm, wl, torch):
    """lattices.lattice_risk: the gradients of sum_b w_b risk_b against V, extra and cost are w_b grad_b, w_b diff and w_b exp(post)
    of the float64 restatement (whose own gradients the CPU tests check by finite differences), at the bars of grad, diff and p;
    zero for the utterance without a path, whatever its w.  lattice_smbr_loss on the alignment of the best path: the risk is at
    least -len, and exactly -len at beam 0 on the 1/16 grid, where the lattice is that path."""
    fs, gs, V, V2, lens, beam = risk_case(mm, wl)
    g, f = gs[0], fs[0]
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, fs, gs)
    lat = bf.lattice(V, beam, lens)
    extra, cost = record_scores(6, lat.arc.size, 0.5), record_scores(16, lat.arc.size)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    Vt = torch.from_numpy(V2).cuda().requires_grad_(True)
    et = torch.from_numpy(extra).cuda().requires_grad_(True)
    ct = torch.from_numpy(cost).cuda().requires_grad_(True)
    lt = torch.from_numpy(lens).cuda()
    risk = mm.lattices.lattice_risk(bf, tl, Vt, ct, et, lt)
    w = np.array([1.5, -2.0, 3.0], dtype=np.float32)
    risk.backward(torch.from_numpy(w).cuda())
    ref = lc.reference(fs, gs, V2, lens, lat.offsets, lat.arc, cost, extra)
    assert np.isneginf(ref.logz[2]) and np.isfinite(ref.logz[:2]).all() and risk[2].item() == 0
    own = lc.owners(lat.offsets, lat.arc.size, B, N)
    gV, gE, gC = (t.grad.cpu().numpy().astype(np.float64) for t in (Vt, et, ct))
    assert (gV[2] == 0).all() and (gE[own == 2] == 0).all() and (gC[own == 2] == 0).all() and not any(np.isnan(x).any() for x in (gV, gE, gC))
    a = lc.DIFF_ABS_A
    p = np.where(np.isneginf(ref.post), 0.0, np.exp(ref.post))
    for b in range(2):
        m = own == b
        Gd, Gg, _ = lc.scales(ref, lat.offsets)[b]
        assert (np.abs(gV[b] - w[b] * ref.grad[b]) <= abs(w[b]) * (1e-4 * np.abs(ref.grad[b]) + a * Gg)).all(), b
        assert (np.abs(gE[m] - w[b] * ref.diff[m]) <= abs(w[b]) * (1e-4 * np.abs(ref.diff[m]) + a * Gd)).all(), b
        assert (np.abs(gC[m] - w[b] * p[m]) <= abs(w[b]) * 1e-4 * np.maximum(p[m], 1e-6)).all(), b
    # sMBR against the best path's own alignment
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    bx = _batch(mm, [fx] * B, [gx] * B)
    Vg = emissions(0, B, N, g.P)
    path, _ = bx.viterbi(Vg, lens)
    ali = np.where(path >= 0, np.asarray(gx.state2pdf)[np.clip(path, 0, None)], -1)
    for beam, exact in ((0.0, True), (3.0, False)):
        latg = bx.lattice(Vg, beam, lens)
        tg = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in latg))
        Vx = torch.from_numpy(Vg).cuda().requires_grad_(True)
        loss = mm.lattice_smbr_loss(bx, tg, Vx, torch.from_numpy(ali).cuda(), lt)
        got = loss.detach().cpu().numpy()
        assert (got >= -lens - 1e-4).all() and (got <= 0).all(), (beam, got)
        if exact:
            assert np.array_equal(got, -lens.astype(np.float32)), got
        else:
            assert (got > -lens).any()
        loss.sum().backward()
        assert np.isfinite(Vx.grad.cpu().numpy()).all() and (not exact or (Vx.grad == 0).all())
