"""Beam-pruned best-path lattices (mm_lattice_f32) on the MI355X against the float32 mode of tests/lattice_reference.py: entry counts
at the wave, block and iteration edges of the compaction, the rows of a transition in global memory (by the switch and by size,
state indices beyond 16 bits), the recursions' instances, the scan's sizes, distinct graphs as CSC and as CSR, cap and its canaries,
repeats, hipGraph capture, error codes, the consequences (a), (c), (d) against the batch's other entries, and
decode.lattice_fsm end to end.

The bar is bit equality of counts, total, arc, score and best on inputs rounded to 1/16 with beams that are multiples of 1/16: every
sum of the definition is exact there, so there is no tolerance to measure.  One case runs unrounded inputs against the float64
restatement: an arc may differ only if its float64 score lies within tau = 2 (N + 3) 2^-24 max|alpha_ref| of -beam (the rounding
bound of the sums involved), scores agree within tau, and at most 1 % of the reference's kept arcs are excused that way."""
import ctypes as C

import numpy as np
import pytest

import arc_reference as ar
import lattice_reference as lr
from test_classpath import case_classes
from test_gpu_parity import _with_env
from test_lattice import ARC_COUNTS, INF, chain_graph, distinct_case, emissions, entries_case, scan_cases, unrounded_cases

pytestmark = pytest.mark.gpu
STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
BIGV = {"MM_DEBUG": "1", "MM_BIGV": "1"}
TWO_WAVES = {"MM_DEBUG": "1", "MM_NWAVES": "2"}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib")


def _batch(mm, fs, gs):
    """One compiled FSM per distinct FSM object."""
    cache = {}
    for f, g in zip(fs, gs):
        if id(f) not in cache:
            cache[id(f)] = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    return mm.batch(*[cache[id(f)] for f in fs])


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(lat, br, what=""):
    """counts, total, arc, score and best, bit for bit."""
    assert np.array_equal(lat.counts, br.counts), (what, lat.counts, br.counts)
    assert lat.counts.dtype == np.int32 and lat.offsets.dtype == np.int64 and lat.arc.dtype == np.int32 and lat.score.dtype == np.float32
    assert np.array_equal(lat.offsets, br.offsets) and int(lat.offsets[-1]) == br.arc.size, what
    assert np.array_equal(lat.arc, br.arc), what
    assert _bits(lat.score, br.score.astype(np.float32)) and not np.isnan(lat.score).any(), what
    assert _bits(lat.best, br.best.astype(np.float32)), (what, lat.best, br.best)


@pytest.fixture(scope="module")
def base(mm, wl):
    g, f, twin, V, lens = case_classes(mm, wl, rounded=True)
    return g, f, V, lens


BEAMS = (0.0, 2.0, 8.0, INF, -0.0625, float("nan"))


def test_base_case(mm, wl, torch, base):
    """40 states with parallel twins, B = 6, N = 40, lens with 1, 0 and a dead utterance: every beam, a beam per utterance, the
    module-level call."""
    g, f, V, lens = base
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, [f] * B, [g] * B)
    k = bf.kernels("lattice")
    assert all(s in k for s in ("mm_tropical_kernel<8,lds>", "mm_log_kernel<MODE_BETA,8,lds,TROP>", "mm_pick_final_kernel", "mm_lattice_prune_kernel<lds,count>",
                                "mm_lattice_scan_kernel", "mm_lattice_prune_kernel<lds,write>")), k
    for beam in BEAMS:
        lat = bf.lattice(V, beam, lens)
        _check(lat, lr.batch_reference([f] * B, [g] * B, V, lens, beam), f"beam {beam}")
        assert np.isneginf(lat.best[3]) and np.isneginf(lat.best[4]) and lat.counts[3].sum() == 0 and lat.counts[4].sum() == 0
        assert (lat.counts[1, lens[1]:] == 0).all()
        if not beam >= 0:
            assert lat.arc.size == 0 and np.isfinite(lat.best[0])
    per = np.array([0.0, 2.0, 8.0, INF, 1.0, -1.0], dtype=np.float32)
    _check(bf.lattice(V, per, lens), lr.batch_reference([f] * B, [g] * B, V, lens, per), "a beam per utterance")
    _check(bf.lattice(V, 2.0, None), lr.batch_reference([f] * B, [g] * B, V, None, 2.0), "lens NULL")
    lat = mm.lattice(bf, [mm.expand(V[b].T, int(lens[b]), "tropical") for b in range(B)], 2.0)
    _check(lat, lr.batch_reference([f] * B, [g] * B, V, lens, 2.0), "module level")


@pytest.mark.parametrize("n", ARC_COUNTS)
def test_entry_counts(mm, wl, torch, n):
    """FSMs of exactly n stored entries: beam inf (whole waves of kept entries), 0 (ties, both of two duplicated parallels), a
    middling beam and a negative one."""
    f, g, V, lens = entries_case(mm, n)
    B = V.shape[0]
    bf = _batch(mm, [f] * B, [g] * B)
    for beam in (INF, 0.0, 0.5, -1.0):
        br = lr.batch_reference([f] * B, [g] * B, V, lens, beam)
        _check(bf.lattice(V, beam, lens), br, f"{n} entries, beam {beam}")
        assert (br.arc.size == 0) == (beam < 0)


@pytest.mark.parametrize("env,names", [(STREAMED, ("mm_tropical_kernel<0,lds>", "MODE_BETA,0,", "prune_kernel<lds,count>")),
                                       (TWO_WAVES, ("mm_tropical_kernel<8,lds>", "MODE_BETA,8,lds", "prune_kernel<lds,write>")),
                                       (BIGV, ("mm_tropical_kernel<8,global>", "MODE_BETA,8,global", "prune_kernel<global,count>", "prune_kernel<global,write>"))])
def test_instances(mm, wl, torch, base, env, names):
    """The recursions' streamed and two-wave instances, and everything in global memory by the switch; kernels() names what ran."""
    g, f, V, lens = base
    B = V.shape[0]
    bf = _with_env(env, lambda: _batch(mm, [f] * B, [g] * B))
    k = bf.kernels("lattice")
    assert all(s in k for s in names), k
    for beam in (0.0, 2.0, INF):
        _check(bf.lattice(V, beam, lens), lr.batch_reference([f] * B, [g] * B, V, lens, beam), f"{names[0]}, beam {beam}")


@pytest.mark.parametrize("S", [45000, 70000])
def test_rows_beyond_the_lds(mm, wl, torch, S):
    """A chain of 45 000 states, N = 3: the two rows of a transition exceed the LDS and are gathered from global memory by the plan;
    70 000 states: state indices beyond 16 bits on the kept arcs."""
    g = chain_graph(wl, S)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 3, 4), np.array([3, 2], dtype=np.int32)
    bf = _batch(mm, [f, f], [g, g])
    k = bf.kernels("lattice")
    # (the forward recursion streams a graph of this many items; the backward instance holds 16-bit indices up to 65 534 states)
    assert "prune_kernel<global,count>" in k and "mm_tropical_kernel<0,global>" in k and ("MODE_BETA,0,global" in k) == (S > 65534), k
    for beam in (1.0, INF):
        br = lr.batch_reference([f, f], [g, g], V, lens, beam)
        assert np.isfinite(br.best).all()
        _check(bf.lattice(V, beam, lens), br, f"chain of {S}, beam {beam}")


def test_scan_sizes(mm, wl, torch):
    """B * N = 1, 255, 256, 257 and 3 x 700 cells on a 3-state graph, lens mixed among 0, 1, < N and N."""
    s = np.arange(3)
    g = wl.GraphSpec("three", 3, np.array([0, 2]), np.array([0.0, -0.5]), np.concatenate([s, [0, 1, 2]]), np.concatenate([s, [1, 2, 0]]),
                     np.array([-0.5, -0.25, -0.75, -0.125, -0.375, -1.0]), np.array([0, 2]), np.array([-1.0, 0.0]), np.array([0, 1, 0], dtype=np.int32), 2)
    f = wl.to_fsm(mm, g, semiring="tropical")
    for B, N, lens in scan_cases():
        lens = np.array(lens, dtype=np.int32)
        V = emissions(B * N, B, N, g.P)
        bf = _batch(mm, [f] * B, [g] * B)
        br = lr.batch_reference([f] * B, [g] * B, V, lens, 1.0)
        assert br.arc.size >= lens.sum() and np.isfinite(br.best[lens > 0]).all()
        _check(bf.lattice(V, 1.0, lens), br, f"B = {B}, N = {N}")


def _csr_compiled(mm, f, g):
    """The FSM handed over as CSR(T_hat): rows by source, the entries of a row by destination.  Returns (CompiledFSM, perm): the
    handle's entry k is entry perm[k] of f."""
    lib = _lib(mm)
    i, j, w = ar.fsm_entries(f)
    perm = np.lexsort((j, i))
    S1 = f.S1
    rowptr = np.zeros(S1 + 1, dtype=np.int64)
    np.add.at(rowptr, i + 1, 1)
    rowptr = np.cumsum(rowptr)
    col, val = np.ascontiguousarray(j[perm], dtype=np.int64), np.ascontiguousarray(w[perm], dtype=np.float32)
    aidx, aval = np.ascontiguousarray(f.alpha_idx, dtype=np.int64), np.ascontiguousarray(f.alpha_val, dtype=np.float32)
    cm = mm.statemap(g.state2pdf, g.P)
    s2p = np.ascontiguousarray(cm.state2pdf, dtype=np.int32)
    h = C.c_void_p()
    lib.check(lib.lib.mm_fsm_create(lib.MM_TROPICAL, S1, f.nnz, lib.MM_CSR, 8, 0, 4, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, aidx.shape[0],
                                    aidx.ctypes.data, aval.ctypes.data, s2p.ctypes.data, g.P + 1, C.byref(h)))
    return mm.CompiledFSM._from_handle(f, cm, h), perm


def test_distinct_graphs_csc_and_csr(mm, wl, torch):
    """Four graphs with state and arc offsets, an utterance without a path between two that have one; then the same FSMs created
    from CSR arrays: the records come in the CSR entry order."""
    gs, fs, V, lens = distinct_case(mm, wl)
    B = len(gs)
    for beam in (0.0, 2.0, INF):
        br = lr.batch_reference(fs, gs, V, lens, beam)
        assert np.isneginf(br.best[1]) and np.isfinite(br.best[[0, 2, 3]]).all() and br.counts[1].sum() == 0
        _check(_batch(mm, fs, gs).lattice(V, beam, lens), br, f"distinct graphs, beam {beam}")
    made = [_csr_compiled(mm, f, g) for f, g in zip(fs, gs)]
    lat = mm.batch(*[c for c, _ in made]).lattice(V, 2.0, lens)
    br = lr.batch_reference(fs, gs, V, lens, 2.0)
    assert np.array_equal(lat.counts, br.counts) and _bits(lat.best, br.best.astype(np.float32))
    N = V.shape[1]
    for b in range(B):
        inv = np.argsort(made[b][1])  # entry of f -> the handle's entry
        for t in range(N):
            lo, hi = br.offsets[b * N + t], br.offsets[b * N + t + 1]
            want = inv[br.arc[lo:hi]]
            order = np.argsort(want)
            assert np.array_equal(lat.arc[lo:hi], want[order]) and _bits(lat.score[lo:hi], br.score[lo:hi][order].astype(np.float32)), (b, t)


def _raw(mm, torch, bf, Vt, lt, beam_t, counts, total, best, arc, score, cap, csb=None):
    B, N, P = Vt.shape
    return _lib(mm).lib.mm_lattice_f32(bf._h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), lt.data_ptr() if lt is not None else None, N,
                                       beam_t.data_ptr() if beam_t is not None else None, counts.data_ptr() if counts is not None else None,
                                       N if csb is None else csb, total.data_ptr() if total is not None else None,
                                       best.data_ptr() if best is not None else None, arc.data_ptr() if arc is not None else None,
                                       score.data_ptr() if score is not None else None, cap, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_cap_and_canaries(mm, wl, torch, base):
    """The count-only call; cap = total, total - 1 and 1: nothing at or behind arc[cap] / score[cap] is touched and the prefix is the
    full call's; counts with a stride; best NULL; max_arcs too small raises, large enough returns the full lattice."""
    g, f, V, lens = base
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, [f] * B, [g] * B)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, 2.0)
    n = br.arc.size
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    beam = torch.full((B,), 2.0, device="cuda")
    counts = torch.full((B, N + 3), -7, dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert _raw(mm, torch, bf, Vt, lt, beam, counts, total, None, None, None, 0, csb=N + 3) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == n and np.array_equal(counts[:, :N].cpu().numpy(), br.counts) and (counts[:, N:] == -7).all()
    for cap in (n, n - 1, 1):
        arc = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
        score = torch.full((n + 8,), 7.0, device="cuda")
        best = torch.zeros(B, device="cuda")
        total.zero_()
        assert _raw(mm, torch, bf, Vt, lt, beam, counts, total, best, arc, score, cap, csb=N + 3) == 0
        torch.cuda.synchronize()
        assert int(total.item()) == n and np.array_equal(counts[:, :N].cpu().numpy(), br.counts)
        assert np.array_equal(arc[:cap].cpu().numpy(), br.arc[:cap]) and _bits(score[:cap].cpu().numpy(), br.score[:cap].astype(np.float32))
        assert (arc[cap:] == -7).all() and (score[cap:] == 7.0).all(), cap
        assert _bits(best.cpu().numpy(), br.best.astype(np.float32))
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        bf.lattice(V, 2.0, lens, max_arcs=n - 1)
    assert str(n) in str(ei.value)
    _check(bf.lattice(V, 2.0, lens, max_arcs=n + 100), br, "max_arcs")
    _check(bf.lattice(V, 2.0, lens, max_arcs=n), br, "max_arcs = total")


def test_repeats_and_graph_capture(mm, wl, torch):
    """A repeated call returns the same bits (unrounded inputs); a capture after a first call replays them, and a replay after V and
    beam were overwritten in place follows them."""
    g, f, twin, V, lens = case_classes(mm, wl, rounded=False)
    g0, f0, _, V0, _ = case_classes(mm, wl, rounded=True)
    B, N = V.shape[0], V.shape[1]
    bf = _batch(mm, [f] * B, [g] * B)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    a, b = bf.lattice(Vt, 3.0, lt), bf.lattice(Vt, 3.0, lt)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a.arc.numel() > 100
    # the capturable form on the rounded twin of the case: one call into fixed buffers
    bf0 = _batch(mm, [f0] * B, [g0] * B)
    Vt = torch.from_numpy(V0).cuda()
    beam = torch.full((B,), 2.0, device="cuda")
    V1 = emissions(77, B, N, g0.P)
    runs = ((V0, 2.0), (V1, 8.0), (V0, 0.0))
    cap = max(lr.batch_reference([f0] * B, [g0] * B, Vn, lens, bm).arc.size for Vn, bm in runs) + 16
    first = bf0.lattice(Vt, beam, lt, max_arcs=cap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = bf0.lattice(Vt, beam, lt, max_arcs=cap)
    for Vn, bm in runs:
        Vt.copy_(torch.from_numpy(Vn).cuda())
        beam.fill_(bm)
        out.arc.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        br = lr.batch_reference([f0] * B, [g0] * B, Vn, lens, bm)
        n = br.arc.size
        assert n <= cap and int(out.offsets[-1].item()) == n
        got = mm.Lattice(out.counts.cpu().numpy(), out.offsets.cpu().numpy(), out.arc[:n].cpu().numpy(), out.score[:n].cpu().numpy(), out.best.cpu().numpy())
        _check(got, br, f"replay, beam {bm}")
        assert (out.arc[n:] == -7).all()
    assert first.arc.numel() < cap


def test_capture_before_a_first_call_is_refused(mm, wl, torch, base):
    """Neither the arc table nor the workspace is made during a capture."""
    g, f, V, lens = base
    fresh = _batch(mm, [f] * 3, [g] * 3)
    Vt = torch.from_numpy(V[:3]).cuda()
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.lattice(Vt, 2.0, None, max_arcs=64)
    assert ei.value.code == -1, str(ei.value)
    _check(fresh.lattice(V[:3], 2.0, None), lr.batch_reference([f] * 3, [g] * 3, V[:3], None, 2.0), "after the refused capture")


def test_error_codes(mm, wl, torch):
    lib = _lib(mm).lib
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    Vt = torch.zeros((B, N, P), device="cuda")
    beam = torch.ones(B, device="cuda")
    counts = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    arc = torch.zeros(64, dtype=torch.int32, device="cuda")
    score = torch.zeros(64, device="cuda")
    raw = lambda bf, **kw: _raw(mm, torch, bf, Vt, None, **{**dict(beam_t=beam, counts=counts, total=total, best=None, arc=arc, score=score, cap=64), **kw})
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert raw(lb) == -4 and b"tropical" in lib.mm_last_error()
    with pytest.raises(mm.MarkovModelsAMDError):
        lb.kernels("lattice")
    with pytest.raises(mm.MarkovModelsAMDError):
        lb.lattice(Vt, 1.0)
    with pytest.raises(TypeError):
        mm.lattice(lb, [np.zeros((P + 1, N + 1), dtype=np.float32)] * B, 1.0)
    ft = wl.to_fsm(mm, g, semiring="tropical")
    tb = _batch(mm, [ft] * B, [g] * B)
    assert raw(tb, beam_t=None) == -1 and raw(tb, counts=None) == -1 and raw(tb, total=None) == -1
    assert raw(tb, csb=N - 1) == -2
    assert raw(tb, score=None) == -1 and raw(tb, arc=None) == -1 and raw(tb, cap=-1) == -1
    assert raw(tb, arc=None, score=None, cap=5) == -1
    assert raw(tb) == 0 and raw(tb, arc=None, score=None, cap=0) == 0
    torch.cuda.synchronize()
    with pytest.raises(mm.DimensionMismatch):
        tb.lattice(Vt, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        tb.lattice(Vt, 1.0, max_arcs=-2)


def test_consequences_on_the_device(mm, wl, torch, base):
    """(a) the entries classpath takes (every entry a class of its own) are kept with score 0 at any beam >= 0; (c) the kept sets
    are nested in the beam; (d) the maximum of the kept scores into (j, frame t + 2) is maxstateposteriors' mu wherever
    mu >= -beam, bit for bit; bestpath on decode.lattice_fsm's graph returns the original score, bit for bit."""
    g, f, V, lens = base
    B, N = V.shape[0], V.shape[1]
    i, j, _ = ar.fsm_entries(f)
    S1 = f.S1
    bf = _batch(mm, [f] * B, [g] * B)
    bf.set_path_classes(np.arange(f.nnz, dtype=np.int32), f.nnz)
    _, entries, score = bf.classpath(V, None, lens)
    mu = bf.maxstateposteriors(V, lens)  # [B * S1, N + 1]
    prev = None
    for beam in (0.0, 2.0, 8.0, INF):
        lat = bf.lattice(V, beam, lens)
        assert _bits(lat.best, score)
        recs = []
        for b in range(B):
            t, k, src, dst, s = mm.decode.lattice_arcs(bf, lat, b)
            assert np.array_equal(src, i[k]) and np.array_equal(dst, j[k])
            recs.append(set(zip(t.tolist(), k.tolist())))
            sc = dict(zip(zip(t.tolist(), k.tolist()), s.tolist()))
            for tt in range(int(lens[b])):
                if np.isfinite(score[b]):
                    assert sc[(tt, int(entries[b, tt]))] == 0.0, (b, tt)  # (a)
                m = np.full(S1, -np.inf, dtype=np.float32)
                np.maximum.at(m, dst[t == tt], s[t == tt])
                mub = mu[b * S1 : (b + 1) * S1, tt + 1]
                want = mub >= -np.float32(beam)
                assert _bits(m[want], mub[want]) and np.isneginf(m[~want]).all(), (b, beam, tt)  # (d)
        if prev is not None:
            assert all(p <= r for p, r in zip(prev, recs))  # (c)
        prev = recs
        if beam == 2.0:
            for b in (0, 1, 5):
                lf, s2p = mm.decode.lattice_fsm(bf, lat, b)
                lb = mm.batch(mm.compile(lf, mm.statemap(s2p, g.P)))
                L = int(lens[b])
                _, sc2 = lb.viterbi(np.ascontiguousarray(V[b : b + 1, :L]), None)
                assert _bits(sc2, score[b : b + 1]), (b, sc2, score[b])


def test_unrounded_inputs_against_float64(mm, wl, torch):
    """random_fsm(30, 5, 3.0, seed=9) and lexicon_fsm(80, seed=2), standard-normal V, beams 2 and 8: an arc may differ from the
    float64 restatement only if its float64 score lies within tau = 2 (N + 3) 2^-24 max|alpha_ref| of -beam; scores agree within tau;
    the excused arcs are at most 1 % of the reference's kept ones."""
    for g, f, V, lens in unrounded_cases(mm, wl):
        B, N = V.shape[0], V.shape[1]
        bf = _batch(mm, [f] * B, [g] * B)
        for beam in (2.0, 8.0):
            lat = bf.lattice(V, beam, lens)
            excused = kept = 0
            for b in range(B):
                t, k, _, _, s = mm.decode.lattice_arcs(bf, lat, b)
                r64 = lr.reference(f, g.state2pdf, g.P, V[b], int(lens[b]), N, beam, np.float64)
                L = int(lens[b])
                e, n, tol = lr.compare_unrounded([k[t == tt] for tt in range(L)], [s[t == tt] for tt in range(L)], r64, beam, N)
                assert (t < L).all() and abs(float(lat.best[b]) - float(r64.best)) <= tol
                excused, kept = excused + e, kept + n
            print(f"{g.name}: beam {beam}: {kept} arcs kept by the reference, {excused} excused, tau {tol:.3g}")
            assert kept > 0 and excused <= 0.01 * kept, (g.name, beam, excused, kept)
