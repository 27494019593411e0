"""Lattice expected cost (mm_latticecost_f32) without a GPU: the bindings of the new entry, the argument checks that need no device,
the float64 restatement of tests/latcost_reference.py -- the header's definition -- against brute-force enumeration of every lattice
path of hand-built graphs and of the 40-state graph, with doctored records, against central finite differences of its own risk (grad
= d risk / d V, diff = d risk / d extra, exp(post) = d risk / d cost), the header's identities, mm_expectedcost_f32's reference on
the full lattice, the committed float32 floor against the constant of the bar, and lattices.record_index / pdf_costs on host arrays.
The cases of tests/test_gpu_latticecost.py are built here (floor_cases: what tools/measure_latticecost_floor.py measures)."""
import ctypes as C
import json
import os
import re
from types import SimpleNamespace

import numpy as np

import arc_reference as ar
import cost_reference as cr
import latcost_reference as lc
import latpost_reference as lp
import lattice_reference as lr
from test_lattice import INF, chain_graph, distinct_case, emissions, entries_case, grid, hand_graphs, stub_batch
from test_latticeposteriors import CELL_COUNTS, record_scores, small_graphs
from test_viterbiwindow import on_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = 64.0  # the shift case: costs c and c + 64 per record (exact in float32)


# ---- the cases the GPU tests run
def one_pair_fsm(mm, n):
    """One real state with n parallel self-loops of different weights and an arc into the final state (the construction of
    test_gpu_latticeposteriors._one_pair_fsm): every record of a cell on ONE accumulator."""
    w = -3.0 * np.random.default_rng(n).random(n)
    f = mm.FSM.from_fields([0], [0.0], [0, n, n + 2], [0] * n + [0, 1], np.concatenate([w, [-0.5, 0.0]]).astype(np.float32), [0], semiring="tropical")
    return f, SimpleNamespace(state2pdf=np.array([0], dtype=np.int32), P=2)


def smallest_cases(mm, wl, which):
    """(what, fs, gs, V, V2, lens, beam) of the smallest shapes: B = 3, N = 6, lens [6, 1, 0] and None, beams 0 (grid), 2, inf."""
    g, f = small_graphs(mm, wl)[which]
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    B, N = 3, 6
    for lens in (np.array([6, 1, 0], dtype=np.int32), None):
        for beam in (0.0, 2.0, INF):
            gg, ff = (gx, fx) if beam == 0.0 else (g, f)
            V = emissions(which + 1, B, N, g.P, rounded=beam == 0.0, scale=1.0)
            V2 = emissions(which + 5, B, N, g.P, rounded=False, scale=1.5)
            yield f"{g.name}, lens {None if lens is None else lens.tolist()}, beam {beam}", [ff] * B, [gg] * B, V, V2, lens, beam


def cell_case(mm, n):
    """n parallel self-loops, B = 2, N = 4, lens [4, 3]: (fs, gs, V, V2, lens)."""
    f, g = one_pair_fsm(mm, n)
    B, N = 2, 4
    return [f] * B, [g] * B, emissions(n, B, N, g.P, rounded=False, scale=1.0), emissions(n + 1, B, N, g.P, rounded=False), np.array([4, 3], dtype=np.int32)


def shift_case(mm, wl):
    """The 40-state graph, B = 2, N = 200, beam 3: (fs, gs, V, lens, beam)."""
    g, f = small_graphs(mm, wl)[1]
    return [f] * 2, [g] * 2, emissions(61, 2, 200, g.P, rounded=False, scale=1.0), np.array([200, 173], dtype=np.int32), 3.0


def risk_case(mm, wl):
    """lattice_risk's case: the 40-state graph, B = 3, N = 6, beam 4; utterance 2 loses every path under the second V."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    V = emissions(12, B, N, g.P, rounded=False, scale=1.0)
    V2 = emissions(13, B, N, g.P, rounded=False, scale=1.0)
    V2[2, 3, :] = -np.inf
    return [f] * B, [g] * B, V, V2, lens, 4.0


def floor_cases(mm, wl):
    """(what, fs, gs, V2, lens, offsets, arc, extra, cost) of the GPU tests' inputs, the lattices by tests/lattice_reference.py."""
    def lat(fs, gs, V, lens, beam):
        br = lr.batch_reference(fs, gs, V, lens, beam)
        return br.offsets, br.arc

    for which in (0, 1):
        for what, fs, gs, V, V2, lens, beam in smallest_cases(mm, wl, which):
            offs, arc = lat(fs, gs, V, lens, beam)
            c = record_scores(3, arc.size)
            yield what, fs, gs, V2, lens, offs, arc, record_scores(2, arc.size), grid(c) if beam == 0.0 else c
    for n in CELL_COUNTS:
        fs, gs, V, V2, lens = cell_case(mm, n)
        offs, arc = lat(fs, gs, V, lens, INF)
        yield f"{n} parallel self-loops", fs, gs, V2, lens, offs, arc, record_scores(n, arc.size, 2.0), record_scores(n + 7, arc.size)
    for n in (257, 1025):
        f, g, V, lens = entries_case(mm, n)
        B = V.shape[0]
        offs, arc = lat([f] * B, [g] * B, V, lens, INF)
        yield f"{n} entries", [f] * B, [g] * B, emissions(n + 2, B, V.shape[1], g.P, rounded=False), lens, offs, arc, record_scores(n, arc.size), record_scores(n + 7, arc.size)
    gs, fs, V, lens = distinct_case(mm, wl)
    for beam in (2.0, INF):
        offs, arc = lat(fs, gs, V, lens, beam)
        yield f"distinct graphs, beam {beam}", fs, gs, emissions(22, V.shape[0], V.shape[1], 5, rounded=False, scale=1.0), lens, offs, arc, record_scores(4, arc.size, 0.5), record_scores(14, arc.size)
    g = chain_graph(wl, 3000)
    f = wl.to_fsm(mm, g, semiring="tropical")
    V, lens = emissions(3, 2, 5, 4), np.array([5, 3], dtype=np.int32)
    offs, arc = lat([f, f], [g, g], V, lens, 1.0)
    yield "chain of 3000", [f, f], [g, g], emissions(4, 2, 5, 4, rounded=False), lens, offs, arc, None, record_scores(5, arc.size)
    fs, gs, V, V2, lens, beam = risk_case(mm, wl)
    offs, arc = lat(fs, gs, V, lens, beam)
    yield "lattice_risk", fs, gs, V2, lens, offs, arc, record_scores(6, arc.size, 0.5), record_scores(16, arc.size)
    fs, gs, V, lens, beam = shift_case(mm, wl)
    offs, arc = lat(fs, gs, V, lens, beam)
    c = record_scores(62, arc.size)
    yield "shift: N = 200, beam 3", fs, gs, V, lens, offs, arc, None, c
    yield "shift: N = 200, beam 3, costs + 64", fs, gs, V, lens, offs, arc, None, c + np.float32(SHIFT)


def floor_ratio(ref64, ref32, offsets):
    """Worst |grad_f32 - grad_f64| / G_b, per utterance G_b of the float64 side; the utterances whose grad is degenerate
    (latcost_reference.scales: rounding noise around a structural 0) have no G_b and are left out."""
    worst = 0.0
    for b, (Gd, G, degenerate) in enumerate(lc.scales(ref64, offsets)):
        if G > 0 and not degenerate:
            worst = max(worst, float(np.abs(ref32.grad[b] - ref64.grad[b]).max()) / G)
    return worst


def floor_ratio_diff(ref64, ref32, offsets):
    """Worst |diff_f32 - diff_f64| / G_b."""
    worst = 0.0
    B, N = ref64.grad.shape[:2]
    own = lc.owners(offsets, ref64.diff.size, B, N)
    for b in range(B):
        m = own == b
        G = float(np.abs(ref64.diff[m]).max()) if m.any() else 0.0
        if G > 0:
            worst = max(worst, float(np.abs(ref32.diff[m] - ref64.diff[m]).max()) / G)
    return worst


# ---- the tests
def test_entry_is_bound(mm):
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_latticecost_f32" in mm.SYMBOLS and len(lib.mm_latticecost_f32.argtypes) == 20
    assert callable(mm.latticecost) and hasattr(mm.BatchedFSM, "latticecost")
    assert mm.LatticeCost._fields == ("risk", "diff", "post", "logz", "grad", "gamma")
    for name in ("lattice_risk", "record_index", "pdf_costs", "lattice_smbr_loss"):
        assert callable(getattr(mm.lattices, name)) and getattr(mm, name) is getattr(mm.lattices, name)
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_latticecost_f32(" in hdr and "20 = mm_latticecost_f32" in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_latticecost_f32, LIB\)", src) and "function latticecost(" in src


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: offsets, logz or risk NULL (-1), a negative nrec (-1), arc, cost,
    diff or post NULL with records to read (-1), strides that overlap rows with grad or gamma given (-2); with those in order the
    NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))

    def call(offsets=p, arc=p, nrec=4, extra=None, cost=fp, risk=fp, diff=fp, post=fp, logz=fp, grad=None, gamma=None, gsb=0, gsn=0, N=8):
        return lib.mm_latticecost_f32(None, fp, 8, 1, None, N, offsets, arc, nrec, extra, cost, risk, diff, post, logz, grad, gamma, gsb, gsn, None)

    for kw in ({"offsets": None}, {"logz": None}, {"risk": None}, {"arc": None}, {"post": None}, {"cost": None}, {"diff": None}):
        assert call(**kw) == -1 and b"is NULL" in lib.mm_last_error(), kw
    assert call(nrec=-1) == -1 and b"nrec" in lib.mm_last_error()
    for kw in ({"grad": fp}, {"gamma": fp}, {"grad": fp, "gamma": fp}):
        assert call(gsb=8 * 4 - 1, gsn=4, **kw) == -2 and b"stride" in lib.mm_last_error()
        assert call(gsb=0, gsn=0, **kw) == -2 and b"stride" in lib.mm_last_error()
    assert call() == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(arc=None, post=None, cost=None, diff=None, nrec=0) == -1 and b"NULL batch" in lib.mm_last_error()  # (an empty lattice)
    assert call(grad=fp, gamma=fp, gsb=32, gsn=4, extra=fp) == -1 and b"NULL batch" in lib.mm_last_error()


def _lattices_of(f, g, V, L, N, beams=(INF, 1.0)):
    for beam in beams:
        r = lr.reference(f, g.state2pdf, g.P, V, L, N, beam)
        yield beam, np.concatenate([[0], np.cumsum(r.counts, dtype=np.int64)]), r.arc


def _against_enumeration(f, g, V, L, N, offsets, arc, extra, cost, what):
    ref = lc.reference([f], [g], V[None, :N], [L], offsets, arc, cost, extra)
    cl = lp.cells(offsets, arc.size, 0, N)
    risk, logz, mass, massA = lc.brute_force(f, g.state2pdf, g.P, V, L, N, cl, arc, cost, extra)
    assert np.isneginf(logz) == np.isneginf(ref.logz[0]), what
    if np.isneginf(logz):
        assert ref.risk[0] == 0 and (ref.diff[np.concatenate([np.arange(lo, hi) for lo, hi in cl] + [np.zeros(0, dtype=np.int64)])] == 0).all() and (ref.grad == 0).all(), what
        return False
    scale = max(1.0, float(np.abs(cost).sum()))
    assert abs(ref.risk[0] - risk) <= 1e-12 * scale, (what, ref.risk[0], risk)
    i, _, _ = ar.fsm_entries(f)
    want = np.zeros(arc.size)
    grad = np.zeros((N, g.P))
    for t, (lo, hi) in enumerate(cl[:L]):
        for r in range(lo, hi):
            if r in mass:
                want[r] = massA[r] - mass[r] * risk  # = post (E[A | through r] - risk)
                grad[t, g.state2pdf[i[arc[r]]]] += want[r]
    covered = np.concatenate([np.arange(lo, hi) for lo, hi in cl])
    assert np.allclose(ref.diff[covered], want[covered], rtol=0, atol=1e-11 * scale), what
    assert np.allclose(ref.grad[0], grad, rtol=0, atol=1e-11 * scale) and (ref.grad[0, L:] == 0).all(), what
    return True


def test_restatement_against_brute_force(mm, wl):
    """Every hand graph of test_lattice (parallel entries with ties, two state sequences, a dead end, no path, len 0 and 1) and the
    40-state graph at N = 4, the lattices of beam inf and 1 under ANOTHER V, extra NULL and given, -inf in V: risk, diff and grad of
    the restatement are the enumeration's risk, mass-weighted A minus mass times risk per record, and its sums by source pdf."""
    with_path = without = 0
    cases = [(name, f, SimpleNamespace(state2pdf=s2p, P=P), V, L, N) for name, f, s2p, P, V, L, N in hand_graphs(mm)]
    g, f = small_graphs(mm, wl)[1]
    cases.append((g.name, f, g, emissions(4, 1, 4, g.P)[0], 4, 4))
    for name, f, g, V, L, N in cases:
        for beam, offsets, arc in _lattices_of(f, g, V, L, N):
            V2 = grid(V + 0.5 * np.random.default_rng(len(name)).standard_normal(V.shape))
            V3 = V2.copy()
            if N > 2:
                V3[1, 0] = -np.inf
            for Vn in (V, V2, V3):
                for extra in (None, record_scores(7, arc.size)):
                    ok = _against_enumeration(f, g, Vn, L, N, offsets, arc, extra, record_scores(9, arc.size), (name, beam, extra is not None))
                    with_path += ok
                    without += not ok
    assert with_path > 20 and without > 0


def test_doctored_records_in_the_restatement(mm):
    """Entry indices -1, nnz and the phony self-loop's are dead records (diff 0); a smaller nrec is the truncated lattice: the
    restatement against the enumeration over the same doctored arrays."""
    name, f, s2p, P, V, L, N = hand_graphs(mm)[3]  # ("ties, len 5")
    g = SimpleNamespace(state2pdf=s2p, P=P)
    sy = lr.system(f)
    _, offsets, arc = next(_lattices_of(f, g, V, L, N, (INF,)))
    arc = arc.copy()
    lo1 = int(offsets[1])
    arc[lo1], arc[lo1 + 1], arc[lo1 + 2] = -1, sy.i.size, int(np.flatnonzero(sy.phony)[0])
    cost = record_scores(1, arc.size)
    assert _against_enumeration(f, g, V, L, N, offsets, arc, None, cost, "doctored")
    ref = lc.reference([f], [g], V[None, :N], [L], offsets, arc, cost)
    assert (ref.diff[lo1 : lo1 + 3] == 0).all() and np.isneginf(ref.post[lo1 : lo1 + 3]).all()
    cut = lc.reference([f], [g], V[None, :N], [L], offsets, arc, cost, nrec=int(offsets[3]))
    assert cut.diff.size == offsets[3] and cut.risk[0] == 0 and (cut.diff == 0).all() and (cut.grad == 0).all()
    bad = offsets.copy()
    bad[2] = bad[1] - 1  # (a decreasing offset: cell 1 is empty, the utterance loses its paths)
    assert not _against_enumeration(f, g, V, L, N, bad, arc, None, cost, "clamped")


def test_gradients_of_the_restatement_by_finite_differences(mm, wl):
    """grad = d risk / d V, diff = d risk / d extra and exp(post) = d risk / d cost: central differences of the restatement's own
    risk with a step of 2^-8 on inputs of the 1/16 grid.  The truncation error is h^2 / 6 times a third derivative of the risk, a
    fourth joint cumulant of A and indicators, at most about 8 max |A| in size with |A| <= 5 x 3 here: 3e-4; the risk is linear in
    cost, so that difference is exact to rounding."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 1, 5
    V = emissions(5, B, N, g.P)
    br = lr.batch_reference([f], [g], V, None, 3.0)
    extra, cost = grid(record_scores(3, br.arc.size)), grid(record_scores(4, br.arc.size))
    ref = lc.reference([f], [g], V, None, br.offsets, br.arc, cost, extra)
    assert np.isfinite(ref.logz[0]) and br.arc.size > 20 and np.abs(ref.diff).max() > 1e-2
    h = 2.0 ** -8
    risk = lambda Vn, en, cn: lc.reference([f], [g], Vn, None, br.offsets, br.arc, cn, en).risk[0]
    for n in range(N):
        for p in range(g.P):
            Vp, Vm = V.copy(), V.copy()
            Vp[0, n, p] += h
            Vm[0, n, p] -= h
            assert abs((risk(Vp, extra, cost) - risk(Vm, extra, cost)) / (2 * h) - ref.grad[0, n, p]) <= 3e-4, (n, p)
    for r in range(0, br.arc.size, 3):
        ep, em, cp, cm = extra.copy(), extra.copy(), cost.copy(), cost.copy()
        ep[r] += h
        em[r] -= h
        cp[r] += h
        cm[r] -= h
        assert abs((risk(V, ep, cost) - risk(V, em, cost)) / (2 * h) - ref.diff[r]) <= 3e-4, r
        assert abs((risk(V, extra, cp) - risk(V, extra, cm)) / (2 * h) - np.exp(ref.post[r])) <= 1e-9, r


def test_identities_on_the_restatement(mm, wl):
    """The header's identities: post / logz / gamma are latpost_reference's; every cell's diff and every row of grad sum to 0; risk =
    sum exp(post) cost; a cost constant within each cell gives risk = sum of the constants and diff = grad = 0; one record per cell
    on the 1/16 grid gives the exact sum and exact zeros -- in the float32 mode too."""
    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    lens = np.array([6, 4, 0], dtype=np.int32)
    V = emissions(9, B, N, g.P, rounded=False, scale=1.0)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, 3.0)
    cost, extra = record_scores(1, br.arc.size), record_scores(2, br.arc.size, 0.5)
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 2e-5)):
        ref = lc.reference([f] * B, [g] * B, V, lens, br.offsets, br.arc, cost, extra, dtype=dtype)
        base = lp.reference([f] * B, [g] * B, V, lens, br.offsets, br.arc, extra)
        assert np.array_equal(ref.post, base.post) and np.array_equal(ref.logz, base.logz) and np.array_equal(ref.gamma, base.gamma)
        own = lc.owners(br.offsets, br.arc.size, B, N)
        for c in range(B * N):
            lo, hi = br.offsets[c], br.offsets[c + 1]
            assert abs(ref.diff[lo:hi].sum()) <= tol * 10, (dtype, c)
        assert (np.abs(ref.grad.sum(axis=2)) <= tol * 10).all() and (ref.grad[1, 4:] == 0).all() and (ref.grad[2] == 0).all()
        for b in range(2):
            m = own == b
            assert abs(ref.risk[b] - (np.exp(ref.post[m]) * cost[m]).sum()) <= tol * 10, (dtype, b)
        assert ref.risk[2] == 0
        ct = np.repeat(np.arange(B * N) % 5 - 1.5, np.diff(br.offsets)).astype(np.float32)
        con = lc.reference([f] * B, [g] * B, V, lens, br.offsets, br.arc, ct, extra, dtype=dtype)
        for b in range(2):
            assert abs(con.risk[b] - sum((b * N + t) % 5 - 1.5 for t in range(lens[b]))) <= tol * 10
        assert np.abs(con.diff).max() <= tol * 10 and np.abs(con.grad).max() <= tol * 10
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    Vg = emissions(0, B, N, g.P)
    br = lr.batch_reference([fx] * B, [gx] * B, Vg, lens, 0.0)
    assert br.arc.size == 10
    cost = grid(record_scores(3, br.arc.size))
    for dtype in (np.float64, np.float32):
        ref = lc.reference([fx] * B, [gx] * B, Vg, lens, br.offsets, br.arc, cost, dtype=dtype)
        assert ref.risk[0] == cost[:6].astype(np.float64).sum() and ref.risk[1] == cost[6:].astype(np.float64).sum() and (ref.diff == 0).all() and (ref.grad == 0).all()


def test_full_lattice_against_the_expected_cost_reference(mm, wl, oracle):
    """At beam = inf the lattice holds every arc with a finite score, and with cost = pdf_costs(D) -- the frame cost of the source's
    pdf on every record -- risk and grad are those of mm_expectedcost_f32's reference on the same arcs as a log-semiring graph.
    That reference reads the graph's float64 weights, the restatement the FSM's float32 ones: a path's weight differs by at most
    (N + 1) weights x 2^-24 x 4 (the largest weight) = 1.7e-6, which bounds the difference of logz and of every posterior; risk and
    grad are posterior-weighted sums of A, |A| <= N max |D|, and are held to that times the bound."""
    o, oc = oracle
    g, f = small_graphs(mm, wl)[1]
    fl = wl.to_fsm(mm, g)
    B, N = 2, 6
    lens = np.array([6, 4], dtype=np.int32)
    V = emissions(3, B, N, g.P, rounded=False, scale=1.0)
    D = np.random.default_rng(8).standard_normal((B, N, g.P)).astype(np.float32)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, INF)
    idx = mm.lattices.record_index_host([f] * B, [g.state2pdf] * B, g.P, br.offsets, br.arc)
    cost = mm.lattices.pdf_costs(idx, D)
    ref = lc.reference([f] * B, [g] * B, V, lens, br.offsets, br.arc, cost)
    tol, A = (N + 1) * 2.0 ** -24 * 4.0, N * float(np.abs(D).max())
    for b in range(B):
        L = int(lens[b])
        risk, grad, gamma, logz = cr.reference(o, oc, g, fl, V[b].astype(np.float64), D[b].astype(np.float64), L, N)
        print(f"b = {b}: |dlogz| {abs(ref.logz[b] - logz):.3g}  |drisk| {abs(ref.risk[b] - risk):.3g}  |dgrad| {np.abs(ref.grad[b] - grad).max():.3g}  |dgamma| {np.abs(ref.gamma[b] - gamma).max():.3g}")
        assert np.isfinite(logz) and abs(ref.logz[b] - logz) <= tol
        assert abs(ref.risk[b] - risk) <= A * tol, (b, ref.risk[b], risk)
        assert np.allclose(ref.grad[b], grad, rtol=0, atol=A * tol) and np.allclose(ref.gamma[b], gamma, rtol=0, atol=tol)


def test_the_committed_floor_and_the_constant():
    """profiles/latticecost_floor.json is what tools/measure_latticecost_floor.py measured; the constant of the bar is 10 x its worst
    ratio, capped at 1e-4, and the shift case in float32 meets the bar it is held to on the device."""
    tab = json.load(open(os.path.join(ROOT, "profiles", "latticecost_floor.json")))
    worst = max(max(r["diff_err_over_G"], r["grad_err_over_G"]) for r in tab["rows"])
    assert worst == tab["worst_err_over_G"] and abs(lc.F32_FLOOR - worst) <= 0.01 * worst
    assert lc.DIFF_ABS_A == min(10 * lc.F32_FLOOR, 1e-4) and abs(tab["a"] - lc.DIFF_ABS_A) <= 0.01 * lc.DIFF_ABS_A
    shift = [r for r in tab["rows"] if "+ 64" in r["case"]]
    assert shift and all(max(r["diff_err_over_G"], r["grad_err_over_G"]) <= lc.DIFF_ABS_A and r["risk_err"] <= r["risk_bar"] for r in shift)
    assert all(r["risk_err"] <= r["risk_bar"] for r in tab["rows"])


def test_shift_case_in_float32_meets_the_bar(mm, wl):
    """The float32 mode on costs + 64 against the float64 reference of the unshifted costs: diff and grad within the bar, the risk
    shifted by 64 len within its bar -- checked here before the device is held to it."""
    fs, gs, V, lens, beam = shift_case(mm, wl)
    br = lr.batch_reference(fs, gs, V, lens, beam)
    c = record_scores(62, br.arc.size)
    ref = lc.reference(fs, gs, V, lens, br.offsets, br.arc, c)
    got = lc.reference(fs, gs, V, lens, br.offsets, br.arc, c + np.float32(SHIFT), dtype=np.float32)
    want = SimpleNamespace(**{**vars(ref), "risk": ref.risk + SHIFT * lens})
    lc.check(got, want, c + np.float32(SHIFT), lens, br.offsets, "float32 mode, costs + 64")


def test_record_index_and_pdf_costs_on_host_arrays(mm, wl):
    """record_index: utterance, transition and source pdf per record, the phony pdf P for entries outside the FSM; pdf_costs gathers
    D[b, t, pdf] with 0 for the phony pdf, on NumPy arrays and CPU tensors alike, differentiable in a tensor D."""
    import torch

    g, f = small_graphs(mm, wl)[1]
    B, N = 3, 6
    lens = np.array([6, 4, 0], dtype=np.int32)
    V = emissions(9, B, N, g.P)
    br = lr.batch_reference([f] * B, [g] * B, V, lens, 3.0)
    arc = br.arc.copy()
    arc[2], arc[5] = -1, f.nnz
    lat = mm.Lattice(br.counts, br.offsets, arc, br.score, br.best)
    bf = stub_batch(mm, [f] * B, [g] * B)
    bf.P = g.P
    idx = mm.lattices.record_index(bf, lat)
    assert all(isinstance(x, torch.Tensor) and x.dtype == torch.int64 for x in idx[:3]) and idx.P == g.P
    i, _, _ = ar.fsm_entries(f)
    cell = np.searchsorted(br.offsets[1:], np.arange(arc.size), side="right")
    assert np.array_equal(idx.b.numpy(), cell // N) and np.array_equal(idx.t.numpy(), cell % N)
    want = np.concatenate([np.asarray(g.state2pdf), [g.P]])[i[np.clip(arc, 0, f.nnz - 1)]]  # (the phony final state: the phony pdf)
    want[[2, 5]] = g.P
    assert np.array_equal(idx.pdf.numpy(), want)
    D = np.random.default_rng(1).standard_normal((B, N, g.P)).astype(np.float32)
    c = mm.lattices.pdf_costs(idx, D)
    assert isinstance(c, np.ndarray) and c.dtype == np.float32 and c[2] == 0 and c[5] == 0
    keep = np.ones(arc.size, dtype=bool)
    keep[[2, 5]] = False
    assert np.array_equal(c[keep], D[cell[keep] // N, cell[keep] % N, want[keep]])
    Dt = torch.from_numpy(D).requires_grad_(True)
    ct = mm.lattices.pdf_costs(idx, Dt)
    assert np.array_equal(ct.detach().numpy(), c)
    ct.sum().backward()
    cnt = np.zeros((B, N, g.P))
    np.add.at(cnt, (cell[keep] // N, cell[keep] % N, want[keep]), 1.0)
    assert np.array_equal(Dt.grad.numpy(), cnt.astype(np.float32))
