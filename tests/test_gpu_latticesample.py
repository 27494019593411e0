"""Lattice path sampling (mm_latticesample_f32) on the MI355X against tests/latsample_reference.py: the exact distribution of the record
sequences on tiny lattices (the enumeration of every path, the Bernstein rule), the decision rule of the restatement on every other
case -- a chain whose every decision is clear of float32 rounding equals the restatement's, record for record --, the RNG contract,
validity and logprob, the exact edges, doctored input, refusals, graph capture and lattices.lattice_sampled_risk.  The lattices are
the reference's (tests/lattice_reference.py), so a case is the same arrays here and in tests/test_latticesample.py, which asserts
the open-chain cap of every case from the restatement alone."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import latpost_reference as lp
import latsample_reference as ls
import lattice_reference as lr
from sample_reference import bernstein_ratio
from test_gpu_lattice import _batch, _bits, _lib
from test_gpu_parity import _with_env
from test_lattice import INF, as_lattice, chain_graph, distinct_case, emissions
from test_latticebest import unique_best_seed
from test_latticeposteriors import CELL_COUNTS, small_graphs
from test_latticesample import (capture_cases, cell_case, chain_case, decision_cases, doctored_cases, edit_distance, rand40_case, reference_of, sampled_risk_gradients,
                                tiny_cases)
from test_viterbiwindow import on_grid

pytestmark = pytest.mark.gpu
FIELDS = ("rec", "path", "logprob", "logz")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _draw(mm, c, bf=None, K=None, seed=None, **kw):
    bf = bf or _batch(mm, c.fs, c.gs)
    return bf.latticesample(as_lattice(mm, c.lat), c.V, c.K if K is None else K, c.seed if seed is None else seed, c.lens, c.extra, **kw)


def _decide(res, c, ref=None, what=None):
    """The decision rule on rec; path = i(rec); logz to the parity bar; -1 and -inf where the restatement has them."""
    ref = ref or reference_of(c, K=res.rec.shape[1])
    what = what or c.name
    nopen = ls.check(res.rec, ref, what)
    assert res.rec.dtype == np.int64 and res.path.dtype == np.int32 and res.logprob.dtype == np.float32 and res.logz.dtype == np.float32
    for b, f in enumerate(c.fs):
        on = res.rec[b] >= 0
        assert np.array_equal(res.path[b][on], lr.system(f).i[c.arc[res.rec[b][on]]]) and (res.path[b][~on] == -1).all(), (what, b)
    assert np.array_equal(np.isneginf(res.logz), np.isneginf(ref.logz)), (what, res.logz, ref.logz)
    zf = np.isfinite(ref.logz)
    assert (np.abs(res.logz[zf] - ref.logz[zf]) <= 1e-4 * np.maximum(1, np.abs(ref.logz[zf]))).all(), (what, res.logz, ref.logz)
    assert np.isneginf(res.logprob[~zf]).all() and not np.isnan(res.logprob).any(), what
    closed = ~ref.open & zf[:, None]
    tol = 1e-4 * np.maximum(1, np.abs(ref.logz))[:, None] + 1e-6 * np.abs(ref.logprob)
    assert (np.abs(res.logprob[closed] - ref.logprob[closed]) <= tol[closed]).all(), (what, np.abs(res.logprob[closed] - ref.logprob[closed]).max())
    print(f"{what}: {res.rec.shape[0] * res.rec.shape[1]} chains, {nopen} open")
    return ref


def _raw(mm, torch, bf, Vt, lt, offsets, arc, nrec, extra, K, seed, fwd, rec, path, logprob, logz):
    B, N, P = Vt.shape
    ptr = lambda t: t.data_ptr() if t is not None else None
    return _lib(mm).lib.mm_latticesample_f32(bf._h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), ptr(lt), N, offsets.data_ptr(), arc.data_ptr(), nrec, ptr(extra), K,
                                             seed, ptr(fwd), ptr(rec), rec.stride(0) if rec is not None else 0, rec.stride(1) if rec is not None else 0, ptr(path),
                                             path.stride(0) if path is not None else 0, path.stride(1) if path is not None else 0, ptr(logprob),
                                             logprob.stride(0) if logprob is not None else 0, ptr(logz), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def rand40(mm, wl):
    c = rand40_case(mm, wl)
    return c, _batch(mm, c.fs, c.gs)


def test_exact_distribution_on_tiny_lattices(mm, wl, torch):
    """1. K = 65 536 record sequences of every tiny case against the enumeration of every lattice path: bernstein_ratio <= 1, no sample
    outside the enumeration; the parallel records of the last case -- the same source and destination in one cell -- appear each with
    its own frequency, because a sample is a RECORD sequence."""
    for c in tiny_cases(mm, wl):
        f, g = c.fs[0], c.gs[0]
        N, L = c.V.shape[1], int(c.lens[0])
        paths, logp, logz = ls.enumerate_paths(f, g.state2pdf, g.P, c.V[0], L, N, lp.cells(c.offsets, c.arc.size, 0, N), c.arc, c.extra)
        res = _draw(mm, c)
        assert res.rec.shape == (1, c.K, N) and (res.rec[0, :, L:] == -1).all() and (res.path[0, :, L:] == -1).all()
        freq, outside = ls.path_frequencies(paths, res.rec[0, :, :L])
        ratio = bernstein_ratio(freq, np.exp(logp), c.K)
        print(f"{c.name}: {paths.shape[0]} paths, Bernstein ratio {ratio:.3f}")
        assert outside == 0 and ratio <= 1, (c.name, outside, ratio)
        assert abs(res.logz[0] - logz) <= 1e-4 * max(1, abs(logz))
        index = {tuple(p): q for q, p in enumerate(paths.tolist())}
        want = logp[[index[tuple(r)] for r in res.rec[0, :, :L].tolist()]]
        assert (np.abs(res.logprob[0] - want) <= 1e-4 * max(1, abs(logz)) + 1e-6 * np.abs(want)).all(), c.name
    # (c: the case with parallel entries)
    sy = lr.system(f)
    post = lp.reference(c.fs, c.gs, c.V, c.lens, c.offsets, c.arc, c.extra).post
    seen = 0
    for lo, hi in lp.cells(c.offsets, c.arc.size, 0, N)[:L]:
        pairs = {}
        for r in range(lo, hi):
            if post[r] > -np.inf:
                pairs.setdefault((sy.i[c.arc[r]], sy.j[c.arc[r]]), []).append(r)
        for rs in pairs.values():
            if len(rs) > 1 and np.ptp(post[rs]) > 0.1:
                seen += 1
                cnt = np.array([(res.rec[0, :, :L] == r).sum() for r in rs]) / c.K
                assert bernstein_ratio(cnt, np.exp(post[rs]), c.K, M=c.arc.size) <= 1, rs
    assert seen > 0


def test_decision_rule_on_small_graphs(mm, wl, torch):
    """2. The two small graphs, B = 3, lens (N, N - 3, 0), N = 12, beam 6, extra NULL and given, K = 8; want_path / want_logprob off."""
    for c in decision_cases(mm, wl)[:4]:
        res = _draw(mm, c)
        _decide(res, c)
        assert (res.rec[2] == -1).all() and np.isneginf(res.logz[2]) and (res.rec[1, :, 9:] == -1).all() and (res.rec[1, :, :9] >= 0).all()
        bare = _draw(mm, c, want_path=False, want_logprob=False)
        assert bare.path is None and bare.logprob is None and _bits(bare.rec, res.rec) and _bits(bare.logz, res.logz)


@pytest.mark.parametrize("n", CELL_COUNTS)
def test_cell_sizes_around_the_workgroup(mm, wl, torch, n):
    """3. Cells of exactly n records on ONE destination state (the wave, workgroup and second-turn edges): the decision rule with
    different weights; with equal weights at n = 65 and K = 16 384 the places of every cell are uniform by the Bernstein rule."""
    c = cell_case(mm, n)
    assert (c.lat.counts[0, :3] == n).all()
    _decide(_draw(mm, c), c)
    if n == 65:
        e = cell_case(mm, n, K=16384, equal=True)
        res = _draw(mm, e)
        for b, L in enumerate(e.lens):
            for t in range(int(L) - 1):
                place = res.rec[b, :, t] - e.offsets[b * 4 + t]
                assert place.min() >= 0 and place.max() < n
                assert bernstein_ratio(np.bincount(place, minlength=n) / e.K, np.full(n, 1.0 / n), e.K) <= 1, (b, t)


def test_thread_counts(mm, wl, torch):
    """4. The three instances (MM_LATPOST_NT under MM_DEBUG), each in a fresh batch, on cells of 257 and 1025 records and K = 70 (two
    chunks): identical bits in rec, path, logprob and logz, the decision rule once, and kernels() names the instance."""
    for n in (257, 1025):
        c = cell_case(mm, n, K=70)
        got = {}
        for nt in (256, 512, 1024):
            bf = _with_env({"MM_DEBUG": "1", "MM_LATPOST_NT": str(nt)}, lambda: _batch(mm, c.fs, c.gs))
            k = bf.kernels("latticesample")
            assert f"mm_latsample_fwd_kernel<{nt}>" in k and f"mm_latsample_kernel<{nt}>" in k and "exceed" not in k, k
            got[nt] = _draw(mm, c, bf)
        _decide(got[1024], c)
        for nt in (256, 512):
            assert all(_bits(getattr(got[nt], key), getattr(got[1024], key)) for key in FIELDS), (n, nt)


def test_rng_contract(mm, wl, torch, rand40):
    """5. K = 3, 64, 65 and 130 agree on their common prefixes (across the 64-sample chunk); a repeated call is bit-identical;
    another seed gives other samples; two identical utterances at different positions differ; utterance b's samples do not change
    when another utterance's V does."""
    c, bf = rand40
    got = {K: _draw(mm, c, bf, K=K) for K in (3, 64, 65, 130)}
    for K in (3, 64, 65):
        for key in ("rec", "path", "logprob"):
            assert _bits(getattr(got[K], key), np.ascontiguousarray(getattr(got[130], key)[:, :K])), (K, key)
        assert _bits(got[K].logz, got[130].logz)
    again = _draw(mm, c, bf, K=130)
    assert all(_bits(getattr(again, key), getattr(got[130], key)) for key in FIELDS)
    other = _draw(mm, c, bf, K=130, seed=c.seed + 1)
    assert (other.rec != got[130].rec).any(axis=2).mean() > 0.5 and _bits(other.logz, got[130].logz)
    _decide(other, c, reference_of(rand40_case(mm, wl, 130, c.seed + 1)), "another seed")
    # utterances 0 and 1 of a batch of three copies of ONE utterance
    V1 = np.repeat(c.V[:1], 3, axis=0)
    lat = as_lattice(mm, lr.batch_reference(c.fs, c.gs, V1, None, INF))
    same = bf.latticesample(lat, V1, 64, c.seed)
    assert _bits(same.logz[0], same.logz[1]) and (same.rec[0] - lat.offsets[0] != same.rec[1] - lat.offsets[6]).any()
    # another utterance's V
    V2 = c.V.copy()
    V2[1] += 1.0
    moved = _draw(mm, SimpleNamespace(**{**vars(c), "V": V2}), bf, K=64)
    for key in ("rec", "path", "logprob"):
        assert _bits(getattr(moved, key)[[0, 2]], getattr(got[64], key)[[0, 2]]), key
    assert not _bits(moved.logz[1], got[64].logz[1])


def test_validity_logprob_and_record_frequencies(mm, wl, torch, rand40):
    """6. The 40-state lattice, K = 64: every sample is connected (j(r_t) = i(r_{t+1})), ends in f and lies inside its cells;
    path = i(rec); |logprob - (W64 - logz_ref)| <= 1e-4 max(1, |logz_ref|) + 1e-6 |logprob| with W64 the float64 weight of the
    DEVICE's record sequence; logz is latticeposteriors', bit for bit; the decision rule.  Then the record frequencies at K = 4096
    against exp(post) of latpost_reference by the Bernstein rule, M the number of records."""
    c, bf = rand40
    B, N = c.V.shape[0], c.V.shape[1]
    res = _draw(mm, c, bf)
    ref = _decide(res, c)
    sy = lr.system(c.fs[0])
    f = sy.S1 - 1
    for b in range(B):
        ut = ref.uts[b]
        wz = {int(r): float(w) for st in ut.steps for r, w in zip(st.r, st.wz)}
        for k in range(c.K):
            r = res.rec[b, k]
            e = c.arc[r]
            assert all(c.offsets[b * N + t] <= r[t] < c.offsets[b * N + t + 1] for t in range(N)), (b, k)
            assert np.array_equal(sy.j[e[:-1]], sy.i[e[1:]]) and sy.j[e[-1]] == f and np.array_equal(res.path[b, k], sy.i[e])
            W64 = ut.a0[sy.i[e[0]]] + sum(wz[int(x)] for x in r)
            assert abs(res.logprob[b, k] - (W64 - ref.logz[b])) <= 1e-4 * max(1, abs(ref.logz[b])) + 1e-6 * abs(res.logprob[b, k]), (b, k)
    post = bf.latticeposteriors(as_lattice(mm, c.lat), c.V, None, c.extra, want_gamma=False)
    assert _bits(res.logz, post.logz)
    K = 4096
    big = _draw(mm, c, bf, K=K)
    pref = lp.reference(c.fs, c.gs, c.V, None, c.offsets, c.arc, c.extra).post
    freq = np.bincount(big.rec.reshape(-1), minlength=c.arc.size) / K
    ratio = bernstein_ratio(freq, np.exp(pref), K, M=c.arc.size)
    print(f"record frequencies, K = {K}: Bernstein ratio {ratio:.3f}")
    assert ratio <= 1 and (freq[np.isneginf(pref)] == 0).all()


def test_exact_edges(mm, wl, torch):
    """7. A beam-0 lattice with a unique best path on grid inputs: every sample's rec is latticebest's and logprob == 0 exactly.  A
    record with extra = -inf is never drawn.  A no-path utterance and a len = 0 utterance: -1 in rec / path, -inf in logprob / logz.
    The chain of 3000 states."""
    g, f = small_graphs(mm, wl)[1]
    gx = on_grid(g)
    fx = wl.to_fsm(mm, gx, semiring="tropical")
    B, N = 3, 6
    lens = np.array([6, 4, 6], dtype=np.int32)
    seed, Vu = unique_best_seed(mm, wl, gx, fx, B, N, lens)
    bx = _batch(mm, [fx] * B, [gx] * B)
    l0 = as_lattice(mm, lr.batch_reference([fx] * B, [gx] * B, Vu, lens, 0.0))
    assert np.array_equal(l0.counts, (np.arange(N)[None] < lens[:, None]).astype(np.int32))
    best = bx.latticebest(l0, Vu, lens)
    res = bx.latticesample(l0, Vu, 70, 1, lens)
    assert (res.rec == best.rec[:, None, :]).all() and (res.path == best.path[:, None, :]).all()
    assert (res.logprob == 0).all() and _bits(res.logz, best.best)
    # extra = -inf on a record of the beam-3 lattice: never drawn, the others still are
    l3 = as_lattice(mm, lr.batch_reference([fx] * B, [gx] * B, Vu, lens, 3.0))
    # (the third record of utterance 0's best path: test_latticebest.test_gpu_case_conditions -- the lattice holds a way round it)
    base = bx.latticesample(l3, Vu, 256, 2, lens)
    gone = int(bx.latticebest(l3, Vu, lens).rec[0, 2])
    ex = np.zeros(l3.arc.size, dtype=np.float32)
    ex[gone] = -np.inf
    cut = bx.latticesample(l3, Vu, 256, 2, lens, ex)
    assert (base.rec == gone).any() and not (cut.rec == gone).any() and (cut.rec[0] >= 0).all() and np.isfinite(cut.logz[0]) and cut.logz[0] < base.logz[0]
    assert _bits(cut.rec[1:], base.rec[1:]) and _bits(cut.logprob[1:], base.logprob[1:])
    # no path, and len = 0
    gs, fs, V, ln = distinct_case(mm, wl)
    ln = ln.copy()
    ln[3] = 0
    bd = _batch(mm, fs, gs)
    ld = as_lattice(mm, lr.batch_reference(fs, gs, V, ln, 2.0))
    rd = bd.latticesample(ld, V, 5, 3, ln)
    for b in (1, 3):
        assert (rd.rec[b] == -1).all() and (rd.path[b] == -1).all() and np.isneginf(rd.logprob[b]).all() and np.isneginf(rd.logz[b])
    for b in (0, 2):
        assert (rd.rec[b, :, : ln[b]] >= 0).all() and (rd.rec[b, :, ln[b] :] == -1).all() and np.isfinite(rd.logprob[b]).all()
    c = chain_case(mm, wl)
    _decide(_draw(mm, c), c)


def test_doctored_input(mm, wl, torch):
    """8. Through the raw entry: entry indices out of range, decreasing offsets, offsets beyond nrec and a lattice cut by cap -- the
    result is the decision rule's on the clamped lattice; fwd holds -inf on the dead records and keeps its sentinel behind nrec; rec
    and path with strides of their own, whose padding stays untouched."""
    for c in doctored_cases(mm, wl):
        B, N = c.V.shape[0], c.V.shape[1]
        bf = _batch(mm, c.fs, c.gs)
        n = c.arc.size if c.nrec is None else c.nrec
        Vt = torch.from_numpy(c.V).cuda()
        fwd = torch.full((c.arc.size,), 7.0, device="cuda")
        rec = torch.full((B, c.K + 1, N + 3), 7, dtype=torch.int64, device="cuda")
        path = torch.full((B, c.K, N + 1), 7, dtype=torch.int32, device="cuda")
        logprob = torch.full((B, c.K + 2), 7.0, device="cuda")
        logz = torch.empty(B, device="cuda")
        rc = _raw(mm, torch, bf, Vt, None, torch.from_numpy(c.offsets).cuda(), torch.from_numpy(c.arc).cuda(), n, torch.from_numpy(c.extra).cuda(), c.K, c.seed,
                  fwd, rec, path, logprob, logz)
        assert rc == 0, _lib(mm).lib.mm_last_error()
        torch.cuda.synchronize()
        got = SimpleNamespace(rec=rec[:, : c.K, :N].cpu().numpy(), path=path[:, :, :N].cpu().numpy(), logprob=logprob[:, : c.K].cpu().numpy(), logz=logz.cpu().numpy())
        ref = _decide(got, c)
        assert (rec[:, c.K :] == 7).all() and (rec[:, :, N:] == 7).all() and (path[:, :, N:] == 7).all() and (logprob[:, c.K :] == 7).all()
        fw = fwd.cpu().numpy()
        assert (fw[n:] == 7.0).all() and not np.isnan(fw[:n]).any()
        dead = (c.arc[:n] < 0) | (c.arc[:n] >= c.fs[0].nnz)
        assert np.isneginf(fw[:n][dead]).all()
        if c.nrec is not None:
            assert np.isneginf(ref.logz[1:]).all() and np.isfinite(ref.logz[0])


def test_limits_and_refusals(mm, wl, torch, rand40):
    """9. The error codes with a live batch, the state cap with the limit in the message (the largest chain that fits runs), log
    batches, kernels(), the binding's checks and the module-level call."""
    c, bf = rand40
    B, N = c.V.shape[0], c.V.shape[1]
    lat = as_lattice(mm, c.lat)
    k = bf.kernels("latticesample")
    assert "mm_latsample_fwd_kernel<1024>" in k and "mm_latsample_kernel<1024>" in k and "exceed" not in k, k
    cap = int(re.search(r"state cap (\d+)", k).group(1))
    assert 10000 < cap and 64 + 16 * cap <= 160 * 1024 < 64 + 16 * (cap + 4)
    Vc, lens = emissions(3, 2, 3, 4), np.array([3, 2], dtype=np.int32)
    for S, fits in ((cap - 4, True), (cap, False)):  # (the padded count is S + 2 rounded up to a multiple of 4)
        gc = chain_graph(wl, S)
        fc = wl.to_fsm(mm, gc, semiring="tropical")
        bc = _batch(mm, [fc, fc], [gc, gc])
        latc = bc.lattice(Vc, 1.0, lens)
        assert ("exceed" in bc.kernels("latticesample")) == (not fits)
        if fits:
            res = bc.latticesample(latc, Vc, 4, 1, lens)
            assert np.isfinite(res.logz).all() and (res.rec[0, :, :3] >= 0).all() and (res.rec[1, :, 2:] == -1).all()
        else:
            with pytest.raises(mm.MarkovModelsAMDError) as ei:
                bc.latticesample(latc, Vc, 4, 1, lens)
            assert ei.value.code == -4 and str(cap) in str(ei.value), str(ei.value)
    for K, code in ((0, -1), (-3, -1)):
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            bf.latticesample(lat, c.V, K)
        assert ei.value.code == code and "nsamples" in str(ei.value)
    Vt = torch.from_numpy(c.V).cuda()
    offs, arc = torch.from_numpy(c.offsets).cuda(), torch.from_numpy(c.arc).cuda()
    fwd, logz = torch.empty(c.arc.size, device="cuda"), torch.empty(B, device="cuda")
    rec = torch.empty((B, 4, N), dtype=torch.int64, device="cuda")
    lib = _lib(mm).lib
    assert _raw(mm, torch, bf, Vt, None, offs, arc, c.arc.size, None, 4, 0, fwd, None, None, None, logz) == -1 and b"both NULL" in lib.mm_last_error()
    assert _raw(mm, torch, bf, Vt, None, offs, arc, c.arc.size, None, 5, 0, fwd, rec, None, None, logz) == -2 and b"rec_stride_b" in lib.mm_last_error()
    assert _raw(mm, torch, bf, Vt, None, offs, arc, c.arc.size, None, 4, 0, fwd, torch.empty((B, 4, N - 1), dtype=torch.int64, device="cuda"), None, None, logz) == -2 and b"rec_stride_k" in lib.mm_last_error()
    assert _raw(mm, torch, bf, Vt, None, offs, arc, c.arc.size, None, 4, 0, fwd, rec, None, torch.empty((B, 3), device="cuda"), logz) == -2
    lg = mm.batch(*([mm.compile(wl.to_fsm(mm, c.gs[0]), mm.statemap(c.gs[0].state2pdf, c.gs[0].P))] * B))
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        lg.latticesample(lat, c.V, 4)
    assert ei.value.code == -4 and "tropical" in str(ei.value)
    with pytest.raises(mm.MarkovModelsAMDError):
        lg.kernels("latticesample")
    with pytest.raises(TypeError):
        mm.latticesample(lg, lat, [np.zeros((c.gs[0].P + 1, N + 1), dtype=np.float32)] * B, 4)
    with pytest.raises(ValueError):
        bf.latticesample(mm.Lattice(lat.counts, lat.offsets, lat.arc[:-3], lat.score[:-3], lat.best), c.V, 4)
    with pytest.raises(mm.DimensionMismatch):
        bf.latticesample(lat, c.V, 4, extra=np.zeros(c.arc.size - 1, dtype=np.float32))
    with pytest.raises(mm.DimensionMismatch):
        bf.latticesample(mm.Lattice(lat.counts, lat.offsets[:-1], lat.arc, lat.score, lat.best), c.V, 4)
    res = mm.latticesample(bf, lat, [mm.expand(c.V[b].T, N, "tropical") for b in range(B)], c.K, c.seed, extra=c.extra)
    base = _draw(mm, c, bf)
    assert all(_bits(getattr(res, key), getattr(base, key)) for key in FIELDS)


def test_graph_capture(mm, wl, torch, rand40):
    """10. A capture after a first call replays, and follows V and extra overwritten in place."""
    c, _ = rand40
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in as_lattice(mm, c.lat)))
    Vt = torch.from_numpy(c.V).cuda()
    et = torch.zeros(c.arc.size, device="cuda")
    fresh = _batch(mm, c.fs, c.gs)
    first = fresh.latticesample(tl, Vt, c.K, c.seed, None, et)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fresh.latticesample(tl, Vt, c.K, c.seed, None, et)
    for cn in capture_cases(mm, wl):
        Vn, en = cn.V, cn.extra
        Vt.copy_(torch.from_numpy(Vn).cuda())
        et.copy_(torch.from_numpy(en).cuda())
        out.rec.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = SimpleNamespace(**{key: getattr(out, key).cpu().numpy() for key in FIELDS})
        live = fresh.latticesample(tl, Vt, c.K, c.seed, None, et)
        assert all(_bits(getattr(got, key), getattr(live, key).cpu().numpy()) for key in FIELDS), cn.name
        _decide(got, cn, what=cn.name)
    assert np.isfinite(first.logz.cpu().numpy()).all()


def test_lattice_sampled_risk_on_the_device(mm, wl, torch):
    """11. lattices.lattice_sampled_risk with non-additive costs, the edit distance of a sample's state sequence to a fixed one
    (in [0, C], C the length): backward equals the formula on the device's samples; and with K = 16 384 on a tiny lattice the
    estimate lies within K / (K - 1) C (3 e + e^2) + 1e-4 of the exact Cov(cost, indicator) of the enumeration for each of the M
    coordinates of V and extra, e = sqrt(ln(6 M / 1e-6) / (2 K)): Hoeffding on the three sample means the estimator is made of.
    (A union bound at the worst-case cost: 0.45 here, where the exact covariances reach 0.31 and the restatement's own samples miss
    them by 0.007.  The equality with the formula is the sharp half of this test.)"""
    c = tiny_cases(mm, wl)[3]  # (random_fsm(5, seed 4) with an extra: 137 paths)
    f, g = c.fs[0], c.gs[0]
    N, L, P = c.V.shape[1], int(c.lens[0]), g.P
    K = 16384
    bf = _batch(mm, c.fs, c.gs)
    tl = mm.Lattice(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in as_lattice(mm, c.lat)))
    Vt = torch.from_numpy(c.V).cuda().requires_grad_(True)
    et = torch.from_numpy(c.extra).cuda().requires_grad_(True)
    lt = torch.from_numpy(c.lens).cuda()
    smp = bf.latticesample(tl, Vt.detach(), K, c.seed, lt, et.detach())
    rec, path = smp.rec.cpu().numpy(), smp.path.cpu().numpy()
    sy = lr.system(f)
    target = [0, 1, 2, 3, 4, 0][:L]
    paths, logp, _ = ls.enumerate_paths(f, g.state2pdf, P, c.V[0], L, N, lp.cells(c.offsets, c.arc.size, 0, N), c.arc, c.extra)
    cost_of = {tuple(p): float(edit_distance(sy.i[c.arc[p]].tolist(), target)) for p in paths}
    costs = np.array([[cost_of[tuple(r)] for r in rec[0, :, :L].tolist()]], dtype=np.float32)
    Cmax = float(L)
    assert 0 <= costs.min() and costs.max() <= Cmax and np.ptp(costs) >= 2
    risk = mm.lattices.lattice_sampled_risk(bf, tl, Vt, smp, torch.from_numpy(costs).cuda(), et)
    assert abs(float(risk.detach()[0]) - costs.mean()) <= 1e-5 * Cmax
    risk.backward(torch.ones(1, device="cuda"))
    gV, gE, w = sampled_risk_gradients(costs, rec, path, [np.asarray(g.state2pdf)], np.ones(1), c.V.shape, c.arc.size)
    assert abs(w.sum()) <= 1e-9
    dV, dE = Vt.grad.cpu().numpy(), et.grad.cpu().numpy()
    assert np.abs(dV - gV).max() <= 1e-4 and np.abs(dE - gE).max() <= 1e-4  # (float32 sums of K terms of size <= C / K)
    # the exact gradient: Cov(cost, indicator) over the enumeration
    p = np.exp(logp)
    cp = np.array([cost_of[tuple(q)] for q in paths])
    indE = np.zeros((paths.shape[0], c.arc.size))
    indV = np.zeros((paths.shape[0], N, P))
    for q, pr in enumerate(paths):
        indE[q, pr] = 1
        indV[q, np.arange(L), np.asarray(g.state2pdf)[sy.i[c.arc[pr]]]] = 1
    covE = (p * cp) @ indE - (p @ cp) * (p @ indE)
    covV = np.tensordot(p * cp, indV, 1) - (p @ cp) * np.tensordot(p, indV, 1)
    M = c.arc.size + N * P
    e = np.sqrt(np.log(6 * M / 1e-6) / (2 * K))
    bound = K / (K - 1) * Cmax * (3 * e + e * e) + 1e-4
    worst = max(np.abs(dE - covE).max(), np.abs(dV[0] - covV).max())
    print(f"sampled gradient against the exact covariance: worst {worst:.4g}, bound {bound:.4g}, largest |Cov| {max(np.abs(covE).max(), np.abs(covV).max()):.4g}")
    assert worst <= bound
