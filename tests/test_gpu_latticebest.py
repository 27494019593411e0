"""Lattice best paths (mm_latticebest_f32) on the MI355X against the float32 restatement of tests/latbest_reference.py: BIT EQUALITY
on best, score, rec and path, on grid and unrounded inputs alike -- float adds and a maximum leave no tolerance to set.  The lattices
come from BatchedFSM.lattice on the device; the restatement always computes over the records the device was given."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import arc_reference as ar
import latbest_reference as lb
import lattice_reference as lr
from test_gpu_lattice import _batch, _bits, _lib
from test_gpu_parity import _with_env
from test_lattice import INF, chain_graph, distinct_case, emissions, entries_case
from test_latticebest import unique_best_seed
from test_latticeposteriors import CELL_COUNTS, record_scores, small_graphs
from test_viterbiwindow import on_grid

pytestmark = pytest.mark.gpu
FIELDS = ("best", "score", "rec", "path")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _same(res, ref, what=""):
    """best, score (where a cell covers the record), rec and path, bit for bit; nothing NaN."""
    seen = ~np.isnan(ref.score)
    assert res.best.dtype == np.float32 and res.score.dtype == np.float32 and not np.isnan(res.best).any(), what
    assert _bits(res.best, ref.best), (what, res.best, ref.best)
    bad = np.flatnonzero(np.asarray(res.score)[seen].view(np.uint32) != ref.score[seen].view(np.uint32))
    assert bad.size == 0, (what, bad[:10], np.asarray(res.score)[seen][bad[:10]], ref.score[seen][bad[:10]])
    if res.rec is not None:
        assert res.rec.dtype == np.int64 and res.path.dtype == np.int32
        assert np.array_equal(res.rec, ref.rec), (what, res.rec, ref.rec)
        assert np.array_equal(res.path, ref.path), (what, res.path, ref.path)


def _run(bf, fs, gs, lat, V2, lens, extra=None, what="", want_path=True):
    res = bf.latticebest(lat, V2, lens, extra, want_path=want_path)
    ref = lb.reference(fs, gs, V2, lens, lat.offsets, lat.arc, extra)
    assert res.score.shape == lat.arc.shape
    _same(res, ref, what)
    return res, ref


def _raw(mm, torch, bf, Vt, lt, offsets, arc, nrec, extra, best, score, rec, path):
    B, N, P = Vt.shape
    return _lib(mm).lib.mm_latticebest_f32(bf._h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), lt.data_ptr() if lt is not None else None, N,
                                           offsets.data_ptr(), arc.data_ptr(), nrec, extra.data_ptr() if extra is not None else None,
                                           best.data_ptr(), score.data_ptr(), rec.data_ptr() if rec is not None else None,
                                           rec.stride(0) if rec is not None else 0, path.data_ptr() if path is not None else None,
                                           path.stride(0) if path is not None else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def rand40(mm, wl):
    """The 40-state random graph, B = 3, N = 6, its batch and the beam = inf lattice of V."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    V = emissions(31, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    return g, f, V, bf, bf.lattice(V, INF, None)


@pytest.mark.parametrize("which", [0, 1])
def test_bit_equality_at_the_smallest_shapes(mm, wl, torch, which):
    """A 3-state left-to-right graph and a 40-state random graph, B = 3, N = 6, lens [6, 1, 0] and NULL, beams 0 (weights and
    emissions on the 1/16 grid), 2 and inf, under a V that is not the lattice's, extra NULL and given, rec / path NULL and given; then
    rec and path through the raw entry into buffers with strides of their own, whose padding stays untouched."""
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
                nop = bf.latticebest(lat, V2, lens, extra, want_path=False)
                assert nop.rec is None and nop.path is None and _bits(nop.best, res.best) and _bits(nop.score, res.score), what
                if lens is not None:
                    assert np.isneginf(res.best[2]) and (res.rec[2] == -1).all() and (res.path[1, 1:] == -1).all()
    # rec and path with strides: [B, N + 3] and [B, N + 1]
    Vt = torch.from_numpy(V2).cuda()
    recb = torch.full((B, N + 3), 7, dtype=torch.int64, device="cuda")
    pathb = torch.full((B, N + 1), 7, dtype=torch.int32, device="cuda")
    score = torch.empty(lat.arc.size, device="cuda")
    best = torch.empty(B, device="cuda")
    offs, arc, ex = torch.from_numpy(lat.offsets).cuda(), torch.from_numpy(lat.arc).cuda(), torch.from_numpy(extra).cuda()
    assert _raw(mm, torch, bf, Vt, None, offs, arc, lat.arc.size, ex, best, score, recb, pathb) == 0
    torch.cuda.synchronize()
    assert np.array_equal(recb[:, :N].cpu().numpy(), res.rec) and np.array_equal(pathb[:, :N].cpu().numpy(), res.path)
    assert _bits(score.cpu().numpy(), res.score) and _bits(best.cpu().numpy(), res.best)
    assert (recb[:, N:] == 7).all() and (pathb[:, N:] == 7).all()
    # one of the two alone
    pathb.fill_(7)
    assert _raw(mm, torch, bf, Vt, None, offs, arc, lat.arc.size, ex, best, score, None, pathb) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pathb[:, :N].cpu().numpy(), res.path) and (pathb[:, N:] == 7).all()


def _one_pair_fsm(mm, n, equal=False):
    """One real state with n parallel self-loops (different weights, or all equal) and an arc into the final state: every record of a
    cell shares its source and its destination -- every thread and wave of a step on ONE accumulator and ONE trace key."""
    w = np.full(n, -0.75) if equal else -3.0 * np.random.default_rng(n).random(n)
    f = mm.FSM.from_fields([0], [0.0], [0, n, n + 2], [0] * n + [0, 1], np.concatenate([w, [-0.5, 0.0]]).astype(np.float32), [0], semiring="tropical")
    return f, SimpleNamespace(state2pdf=np.array([0], dtype=np.int32), P=2)


@pytest.mark.parametrize("n", CELL_COUNTS)
def test_cell_sizes_around_the_workgroup(mm, wl, torch, n):
    """Cells of exactly n records (n parallel self-loops of one state, beam inf): the wave, workgroup and second-turn edges, one
    target state and one trace key for the whole cell.  With different weights; then with all weights equal, where the tie rule
    must return the LOWEST record of every cell.  Then the FSMs of n stored entries of test_lattice.entries_case."""
    B, N = 2, 4
    lens = np.array([4, 3], dtype=np.int32)
    for equal in (False, True):
        f, g = _one_pair_fsm(mm, n, equal)
        V = emissions(n, B, N, g.P, rounded=False, scale=1.0)
        bf = _batch(mm, [f] * B, [g] * B)
        lat = bf.lattice(V, INF, lens)
        assert (lat.counts[0, :3] == n).all() and lat.counts[0, 3] == 1
        res, _ = _run(bf, [f] * B, [g] * B, lat, V, lens, None, f"{n} parallel self-loops, equal {equal}")
        if equal:
            for b in range(B):
                L = int(lens[b])
                assert np.array_equal(res.rec[b, :L], lat.offsets[b * N : b * N + L]), (n, b, res.rec[b])
        _run(bf, [f] * B, [g] * B, lat, emissions(n + 1, B, N, g.P, rounded=False), lens, record_scores(n, lat.arc.size, 2.0), f"{n} parallel self-loops, extra")
    if n in (257, 1025):
        f, g, V, lens = entries_case(mm, n)
        B = V.shape[0]
        bf = _batch(mm, [f] * B, [g] * B)
        lat = bf.lattice(V, INF, lens)
        assert lat.counts.max() >= n // 2
        _run(bf, [f] * B, [g] * B, lat, V, lens, None, f"{n} entries, the lattice's V (ties between parallels)")
        _run(bf, [f] * B, [g] * B, lat, emissions(n + 2, B, V.shape[1], g.P, rounded=False), lens, record_scores(n, lat.arc.size), f"{n} entries")


def test_distinct_graphs_and_a_long_chain(mm, wl, torch):
    """Four different graphs (state and arc offsets per utterance; utterance 1 has no path, its lattice is empty: best -inf, rec and
    path all -1) at beam 2 and inf; a chain of 3000 states with N = 5: all but a few of the states in LDS are never touched."""
    gs, fs, V, lens = distinct_case(mm, wl)
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, fs, gs)
    V2 = emissions(22, B, N, 5, rounded=False, scale=1.0)
    for beam in (2.0, INF):
        lat = bf.lattice(V, beam, lens)
        res, _ = _run(bf, fs, gs, lat, V2, lens, record_scores(4, lat.arc.size, 0.5), f"distinct graphs, beam {beam}")
        assert np.isneginf(res.best[1]) and np.isfinite(res.best[[0, 2, 3]]).all()
        assert (res.rec[1] == -1).all() and (res.path[1] == -1).all() and lat.counts[1].sum() == 0
        for b in (0, 2, 3):
            assert (res.rec[b, : lens[b]] >= lat.offsets[b * N]).all() and (res.rec[b, : lens[b]] < lat.offsets[(b + 1) * N]).all()
    g = chain_graph(wl, 3000)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 5, 4), np.array([5, 3], dtype=np.int32)
    bf = _batch(mm, [f, f], [g, g])
    lat = bf.lattice(V, 1.0, lens)
    i, _, _ = ar.fsm_entries(f)
    assert (i[lat.arc] > 2900).any() and (i[lat.arc] < 10).any() and lat.arc.size < 200
    res, _ = _run(bf, [f, f], [g, g], lat, emissions(4, 2, 5, 4, rounded=False), lens, None, "chain of 3000")
    assert np.isfinite(res.best).all()


@pytest.mark.parametrize("nt", [256, 512, 1024])
def test_thread_counts(mm, wl, torch, nt):
    """The three instances (MM_LATPOST_NT under MM_DEBUG, read when the batch is made), each in a fresh batch, on the cells of 257
    and 1025 records: one, two and five turns of a thread over a cell.  All return the restatement's bits, so each other's, and
    kernels() names the instance."""
    B, N = 2, 4
    lens = np.array([4, 3], dtype=np.int32)
    for n in (257, 1025):
        f, g = _one_pair_fsm(mm, n)
        V = emissions(n, B, N, g.P, rounded=False, scale=1.0)
        bf = _with_env({"MM_DEBUG": "1", "MM_LATPOST_NT": str(nt)}, lambda: _batch(mm, [f] * B, [g] * B))
        k = bf.kernels("latticebest")
        assert f"mm_latbest_kernel<{nt}>" in k and "exceed" not in k, k
        lat = bf.lattice(V, INF, lens)
        extra = record_scores(n, lat.arc.size)
        res, _ = _run(bf, [f] * B, [g] * B, lat, V, lens, extra, f"{n} records, {nt} threads")
        base = _batch(mm, [f] * B, [g] * B).latticebest(lat, V, lens, extra)
        assert all(_bits(getattr(res, key), getattr(base, key)) for key in FIELDS), (n, nt)


def test_bit_identity(mm, wl, torch):
    """Two calls return the same bits in every output: 257 parallel entries on one accumulator, unrounded inputs."""
    f, g = _one_pair_fsm(mm, 257)
    B, N = 2, 4
    V = emissions(1, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, INF, None)
    extra = record_scores(5, lat.arc.size)
    a = bf.latticebest(lat, V, None, extra)
    for _ in range(2):
        b = bf.latticebest(lat, V, None, extra)
        assert all(_bits(getattr(a, key), getattr(b, key)) for key in FIELDS)
    assert np.isfinite(a.score).all() and lat.arc.size == 2 * (3 * 257 + 1)


def test_doctored_input(mm, wl, torch, rand40):
    """Through the raw entry, against the restatement over the same doctored arrays: entry indices -1, nnz and the phony
    self-loop's; offsets that decrease, are negative and reach behind nrec; nrec below the total; lens outside [0, N]; records no
    cell covers keep their sentinel."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    sy = lr.system(f)
    arc = lat.arc.copy()
    at = [int(lat.offsets[1]), int(lat.offsets[N + 2]) + 1, int(lat.offsets[2 * N + 4])]
    arc[at[0]], arc[at[1]], arc[at[2]] = -1, f.nnz, int(np.flatnonzero(sy.phony)[0])
    doctored = mm.Lattice(lat.counts, lat.offsets, arc, lat.score, lat.best)
    res, _ = _run(bf, fs, gs, doctored, V, None, record_scores(8, arc.size, 0.5), "doctored records")
    assert np.isneginf(res.score[at]).all() and np.isfinite(res.best).all() and not np.isin(res.rec, at).any()
    Vt = torch.from_numpy(V).cuda()
    arct = torch.from_numpy(arc).cuda()
    nrec = int(lat.offsets[N + 3]) + 2  # (utterance 0 whole, utterance 1 cut inside its fourth cell, utterance 2 without records)
    bad = lat.offsets.copy()
    bad[0], bad[N + 2], bad[2 * N + 1] = -5, bad[N + 1] - 3, 2 ** 40
    gap = lat.offsets.copy()
    gap[0], gap[-1] = 2, gap[-1] - 2  # (the first two records and the last two: no cell covers them)
    for what, offsets, n, lens in (("nrec below the total", lat.offsets, nrec, None), ("clamped offsets", bad, nrec, None),
                                   ("lens outside [0, N]", lat.offsets, arc.size, np.array([N + 5, -2, 3], dtype=np.int32)),
                                   ("records no cell covers", gap, arc.size, None)):
        score = torch.full((arc.size,), 7.0, device="cuda")
        best = torch.empty(B, device="cuda")
        rec = torch.empty((B, N), dtype=torch.int64, device="cuda")
        path = torch.empty((B, N), dtype=torch.int32, device="cuda")
        lt = torch.from_numpy(lens).cuda() if lens is not None else None
        assert _raw(mm, torch, bf, Vt, lt, torch.from_numpy(offsets).cuda(), arct, n, None, best, score, rec, path) == 0
        torch.cuda.synchronize()
        ref = lb.reference(fs, gs, V, lens, offsets, arc, None, nrec=n)
        got = SimpleNamespace(best=best.cpu().numpy(), score=score[:n].cpu().numpy(), rec=rec.cpu().numpy(), path=path.cpu().numpy())
        _same(got, ref, what)
        assert (score[n:] == 7.0).all() and (got.score[np.isnan(ref.score)] == 7.0).all(), what
        if what == "records no cell covers":
            assert np.isnan(ref.score).sum() == 4 and np.isfinite(ref.best).all()


def test_consequences(mm, wl, torch):
    """(a) best is the float32 sum along the returned path in the recursion's order, on unrounded inputs.  (b) extra NULL, the
    lattice's own V, grid inputs: best and score are the lattice's.  (c) there score[rec] == 0 and every cell's maximum is 0.  (d) a
    unique best path (seeds chosen so that the beam-0 reference lattice holds one record per cell for EVERY utterance with a path:
    asserted, nobody is excused): path is viterbi's.  (e) extra = -inf on the records of the best path changes rec, and never names
    them.  (f) best <= logz of latticeposteriors, up to the two roundings."""
    g, f = small_graphs(mm, wl)[1]
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    # (a), (f): unrounded
    V = emissions(12, B, N, g.P, rounded=False, scale=1.0)
    bf = _batch(mm, [f] * B, [g] * B)
    lat = bf.lattice(V, 4.0, lens)
    V2 = emissions(13, B, N, g.P, rounded=False, scale=1.0)
    extra = record_scores(6, lat.arc.size, 0.5)
    res, ref = _run(bf, [f] * B, [g] * B, lat, V2, lens, extra, "unrounded")
    sy = lr.system(f)
    w = sy.w.astype(np.float32)
    for b in range(B):
        L = int(lens[b])
        assert np.isfinite(res.best[b])
        acc = np.float32(sy.pi[res.path[b, 0]]) + V2[b, 0, g.state2pdf[res.path[b, 0]]]
        for t in range(L):
            r = res.rec[b, t]
            j = sy.j[lat.arc[r]]
            e = V2[b, t + 1, g.state2pdf[j]] if t < L - 1 else np.float32(0)
            acc = np.float32(acc + np.float32(np.float32(w[lat.arc[r]] + extra[r]) + e))
        assert _bits(np.float32(acc), res.best[b]), (b, acc, res.best[b])
    post = bf.latticeposteriors(lat, V2, lens, extra, want_gamma=False)
    slack = (N + 2) * 2.0 ** -24 * ref.amax + 1e-4 * np.abs(post.logz)  # (the adds behind best; latticeposteriors' parity bar)
    assert (res.best <= post.logz + slack).all(), (res.best, post.logz)
    # (b), (c): grid
    bx = _batch(mm, [fx] * B, [gx] * B)
    Vg = emissions(4, B, N, g.P)
    for beam in (0.0, 2.0, INF):
        lg = bx.lattice(Vg, beam, lens)
        rg, _ = _run(bx, [fx] * B, [gx] * B, lg, Vg, lens, None, f"grid, beam {beam}")
        assert _bits(rg.best, lg.best) and _bits(rg.score, lg.score)
        for b in range(B):
            L = int(lens[b])
            assert (rg.score[rg.rec[b, :L]] == 0).all()
            assert all(rg.score[lg.offsets[b * N + t] : lg.offsets[b * N + t + 1]].max() == 0 for t in range(L))
    # (d): a unique best path
    seed, Vu = unique_best_seed(mm, wl, gx, fx, B, N, lens)
    br = lr.batch_reference([fx] * B, [gx] * B, Vu, lens, 0.0)
    assert np.isfinite(br.best).all() and np.array_equal(br.counts, (np.arange(N)[None] < lens[:, None]).astype(np.int32)), seed
    lu = bx.lattice(Vu, 3.0, lens)
    ru, _ = _run(bx, [fx] * B, [gx] * B, lu, Vu, lens, None, "unique best path")
    vpath, vscore = bx.viterbi(Vu, lens)
    assert np.array_equal(ru.path, vpath) and _bits(ru.best, np.asarray(vscore, dtype=np.float32))
    # (e): remove one record of utterance 0's best path (test_latticebest.test_gpu_case_conditions: the lattice holds a way round)
    gone = int(ru.rec[0, 2])
    ex = np.zeros(lu.arc.size, dtype=np.float32)
    ex[gone] = -np.inf
    re_, _ = _run(bx, [fx] * B, [gx] * B, lu, Vu, lens, ex, "extra = -inf on a record of the best path")
    assert not (re_.rec == gone).any() and np.array_equal(re_.rec[1:], ru.rec[1:]) and not np.array_equal(re_.rec[0], ru.rec[0])
    assert np.isneginf(re_.score[gone]) and np.isfinite(re_.best[0]) and re_.best[0] < ru.best[0]


def test_limits_and_refusals(mm, wl, torch, rand40):
    """A chain one step over the state cap of the LDS is refused with MM_ERR_UNSUPPORTED and the cap in the message; the largest that
    fits runs and matches; log batches are refused; kernels() names the launch, the bytes per state and the cap; a lattice cut by
    max_arcs and an extra of the wrong length raise; the module-level call."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    k = bf.kernels("latticebest")
    assert "mm_latbest_kernel<1024>" in k and "12 bytes of LDS per state" in k and "exceed" not in k, k
    cap = int(re.search(r"state cap (\d+)", k).group(1))
    assert 13000 < cap and 64 + 12 * cap <= 160 * 1024 < 64 + 12 * (cap + 4)
    Vc, lens = emissions(3, 2, 3, 4), np.array([3, 2], dtype=np.int32)
    for S, fits in ((cap - 4, True), (cap, False)):  # (the padded count is S + 2 rounded up to a multiple of 4)
        gc = chain_graph(wl, S)
        fc = wl.to_fsm(mm, gc, semiring="tropical")
        bc = _batch(mm, [fc, fc], [gc, gc])
        latc = bc.lattice(Vc, 1.0, lens)
        assert ("exceed" in bc.kernels("latticebest")) == (not fits)
        if fits:
            res, _ = _run(bc, [fc, fc], [gc, gc], latc, emissions(4, 2, 3, 4, rounded=False), lens, None, f"chain of {S}")
            assert np.isfinite(res.best).all()
        else:
            with pytest.raises(mm.MarkovModelsAMDError) as ei:
                bc.latticebest(latc, Vc, lens)
            assert ei.value.code == -4 and str(cap) in str(ei.value), str(ei.value)
    lg = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        lg.latticebest(lat, V)
    assert ei.value.code == -4 and "tropical" in str(ei.value)
    with pytest.raises(mm.MarkovModelsAMDError):
        lg.kernels("latticebest")
    with pytest.raises(TypeError):
        mm.latticebest(lg, lat, [np.zeros((g.P + 1, N + 1), dtype=np.float32)] * B)
    cut = mm.Lattice(lat.counts, lat.offsets, lat.arc[:-3], lat.score[:-3], lat.best)
    with pytest.raises(ValueError):
        bf.latticebest(cut, V)
    with pytest.raises(mm.DimensionMismatch):
        bf.latticebest(lat, V, None, np.zeros(lat.arc.size - 1, dtype=np.float32))
    with pytest.raises(mm.DimensionMismatch):
        bf.latticebest(mm.Lattice(lat.counts, lat.offsets[:-1], lat.arc, lat.score, lat.best), V)
    res = mm.latticebest(bf, lat, [mm.expand(V[b].T, N, "tropical") for b in range(B)])
    _same(res, lb.reference([f] * B, [g] * B, V, None, lat.offsets, lat.arc), "module level")


def test_graph_capture(mm, wl, torch, rand40):
    """A capture after a first call replays, and follows V and extra overwritten in place."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    fs, gs = [f] * B, [g] * B
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    Vt = torch.from_numpy(V).cuda()
    et = torch.zeros(lat.arc.size, device="cuda")
    fresh = _batch(mm, fs, gs)
    first = fresh.latticebest(tl, Vt, None, et)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fresh.latticebest(tl, Vt, None, et)
    for seed in (41, 42):
        Vn, en = emissions(seed, B, N, g.P, rounded=False, scale=1.0), record_scores(seed, lat.arc.size)
        Vt.copy_(torch.from_numpy(Vn).cuda())
        et.copy_(torch.from_numpy(en).cuda())
        out.score.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        got = SimpleNamespace(**{key: getattr(out, key).cpu().numpy() for key in FIELDS})
        _same(got, lb.reference(fs, gs, Vn, None, lat.offsets, lat.arc, en), f"replay {seed}")
    assert np.isfinite(first.best.cpu().numpy()).all()


def test_rescore_and_onebest_on_the_device(mm, wl, torch, rand40):
    """decode.lattice_rescore on device tensors keeps tensors on the device and equals the host form; the re-pruned lattice goes
    back in; decode.lattice_onebest reads the path."""
    g, f, V, bf, lat = rand40
    B, N = V.shape[0], V.shape[1]
    V2 = emissions(51, B, N, g.P, rounded=False, scale=1.0)
    extra = record_scores(9, lat.arc.size)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    rs = mm.decode.lattice_rescore(bf, tl, torch.from_numpy(V2).cuda(), torch.from_numpy(extra).cuda(), beam=2.0)
    assert all(x.is_cuda for x in rs) and 0 < rs.arc.numel() < lat.arc.size and int(rs.offsets[-1]) == rs.arc.numel()
    host = mm.decode.lattice_rescore(bf, lat, V2, extra, beam=2.0)
    assert all(_bits(a.cpu().numpy(), b) for a, b in zip(rs, host))
    ref = lb.reference([f] * B, [g] * B, V2, None, lat.offsets, lat.arc, extra)
    keep = ref.score >= np.float32(-2.0)
    assert _bits(host.arc, lat.arc[keep]) and _bits(host.score, ref.score[keep]) and _bits(host.best, ref.best)
    res, _ = _run(bf, [f] * B, [g] * B, host, V2, None, extra[keep], "the re-pruned lattice")
    assert _bits(res.best, ref.best)
    t, k, src, dst = mm.decode.lattice_onebest(bf, host, res, 1)
    assert t.size == N and np.array_equal(src, res.path[1]) and np.array_equal(src[1:], dst[:-1]) and dst[-1] == f.S1 - 1


def test_lattice_best_score_gradients(mm, wl, torch):
    """lattices.lattice_best_score: the gradients of sum_b c_b best_b against extra and V are c_b times the indicators of rec and of
    (b, n, pdf(path[b, n])); zero for the utterance without a path.  On grid inputs with a unique best path best(V + h e) - best(V)
    is exactly h on the path's cells and 0 off them, h = 1/16 (the runner-up lies at least 1/16 below)."""
    g, f = small_graphs(mm, wl)[1]
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    seed, V = unique_best_seed(mm, wl, gx, fx, B, N, lens)
    V = V.copy()
    bf = _batch(mm, [fx] * B, [gx] * B)
    lat = bf.lattice(V, 4.0, lens)
    V2 = V.copy()
    V2[2, 3, :] = -np.inf  # (utterance 2 loses every path)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lat))
    lt = torch.from_numpy(lens).cuda()
    Vt = torch.from_numpy(V2).cuda().requires_grad_(True)
    et = torch.zeros(lat.arc.size, device="cuda").requires_grad_(True)
    best = mm.lattices.lattice_best_score(bf, tl, Vt, et, lt)
    c = np.array([1.5, -2.0, 3.0], dtype=np.float32)
    best.backward(torch.from_numpy(c).cuda())
    ref = lb.reference([fx] * B, [gx] * B, V2, lens, lat.offsets, lat.arc)
    assert _bits(best.detach().cpu().numpy(), ref.best) and np.isneginf(ref.best[2]) and np.isfinite(ref.best[:2]).all()
    wantV = np.zeros_like(V2)
    wantE = np.zeros(lat.arc.size, dtype=np.float32)
    for b in range(2):
        for n in range(int(lens[b])):
            wantV[b, n, gx.state2pdf[ref.path[b, n]]] += c[b]
            wantE[ref.rec[b, n]] += c[b]
    assert _bits(Vt.grad.cpu().numpy(), wantV) and _bits(et.grad.cpu().numpy(), wantE)
    # exact differences, utterance 0 under the lattice's own V
    base = bf.latticebest(lat, V, lens)
    h = np.float32(1 / 16)
    for n in range(N):
        for p in range(gx.P):
            Vp = V.copy()
            Vp[0, n, p] += h
            d = bf.latticebest(lat, Vp, lens, want_path=False).best[0] - base.best[0]
            assert d == (h if gx.state2pdf[base.path[0, n]] == p else 0), (n, p, d)
