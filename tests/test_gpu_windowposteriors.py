"""Fixed-lag smoothing posteriors (mm_windowposteriors_f32) on the MI355X against the float64 reference of tests/window_reference.py,
and the consequences the header states: (a) closed from the FSM's own start = pdfposteriors, (b) open = the filter's last frame,
increments and state, (c) exact re-windowing with the carried state in place, (d) the level of a frame, (g) bit-identical repeats
and the outputs that may be NULL; the kernel instances, more pdfs than threads, output strides, error codes, and
streaming.FixedLagSmoother over irregular chunks with one utterance finished early.

The bars are the project's own (tests/test_windowposteriors.py check_against_reference): gamma has check_gamma of
tests/test_gpu_parity.py, ttl and lcommit np.allclose(rtol=1e-5, atol=1e-4), state_out the bar of
test_filterposteriors.check_against_reference.  Every utterance of every test is compared; windows without mass, empty ones and dead
prefixes by their exact conventions.  The reference's float32 mode stays below 0.005 of each bar on these inputs
(test_float32_mode_within_the_bars)."""
import copy
import ctypes as C

import numpy as np
import pytest

import filter_reference as fr
import window_reference as wr
from test_gpu_parity import _with_env, check_gamma
from test_windowposteriors import case_den600, case_distinct, case_random40, check_against_reference, references

pytestmark = pytest.mark.gpu
STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
BIGV = {"MM_DEBUG": "1", "MM_BIGV": "1"}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib").lib


def _batch(mm, wl, gs):
    cache = {}
    for g in gs:
        if id(g) not in cache:
            cache[id(g)] = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    return mm.batch(*[cache[id(g)] for g in gs])


def _seg(bf, so, b):
    return so[int(bf.state_offsets[b]) : int(bf.state_offsets[b + 1])]


def _check(bf, out, refs, lens, what=""):
    """Every utterance against its reference; prints and returns the worst error over each bar."""
    gamma, ttl, lcommit, so = out
    worst = np.zeros(3)
    for b, ref in enumerate(refs):
        worst = np.maximum(worst, check_against_reference(gamma[b], ttl[b], lcommit[b], _seg(bf, so, b), ref, int(lens[b])))
    print(f"{what}: worst error over its bar: gamma {worst[0]:.3g}, ttl / lcommit {worst[1]:.3g}, state_out {worst[2]:.3g}")
    return worst


def _run(bf, case, **kw):
    gs, V, lens, closed, commit = case
    return bf.windowposteriors(V, lens, closed=closed, commit=commit, want_state=True, **kw)


@pytest.fixture(scope="module")
def random40(wl):
    case = case_random40(wl)
    return case, references(case)


def test_random_graph_lengths_end_modes_and_commits(mm, wl, torch, random40):
    case, refs = random40
    gs, V, lens, closed, commit = case
    bf = _batch(mm, wl, gs)
    assert "mm_window_fwd_kernel<8,lds>" in bf.kernels("window") and "mm_window_bwd_kernel<8,lds>" in bf.kernels("window"), bf.kernels("window")
    out = _run(bf, case)
    _check(bf, out, refs, lens, "random40")
    gamma, ttl, lcommit, so = out
    # utterance 4 dies at frame 14, behind its commit frame 9: no gamma, no ttl, the prefix's state_out and lcommit
    assert (gamma[4] == 0).all() and np.isneginf(ttl[4]) and np.isfinite(lcommit[4]) and np.isfinite(_seg(bf, so, 4)).any()
    # utterance 3: len = 0 -- the start vector passes through; utterance 0: c = 0 with len > 0 likewise
    start = fr.start_vector(gs[0]).astype(np.float32)
    assert (gamma[3] == 0).all() and np.isneginf(ttl[3]) and lcommit[3] == 0 and np.array_equal(_seg(bf, so, 3), start)
    assert lcommit[0] == 0 and np.array_equal(_seg(bf, so, 0), start) and np.isfinite(ttl[0])
    assert np.isfinite(ttl[[0, 1, 2, 5]]).all()
    # ... and the same with the death ahead of the commit frame: state_out and lcommit are -inf
    commit2 = commit.copy()
    commit2[4] = 20
    case2 = (gs, V, lens, closed, commit2)
    out = _run(bf, case2)
    _check(bf, out, references(case2), lens, "random40, the death ahead of the commit")
    assert np.isneginf(out[2][4]) and np.isneginf(_seg(bf, out[3], 4)).all()


def test_distinct_graphs(mm, wl, torch):
    case = case_distinct(wl)
    bf = _batch(mm, wl, case[0])
    out = _run(bf, case)
    assert np.isfinite(out[1]).all()
    _check(bf, out, references(case), case[2], "distinct graphs")


def test_denominator_graph(mm, wl, torch):
    case = case_den600(wl)
    bf = _batch(mm, wl, case[0])
    out = _run(bf, case)
    assert np.isfinite(out[1]).all()
    _check(bf, out, references(case), case[2], "denominator graph, 600 states")


def test_streamed_and_global_vector_instances(mm, wl, torch, random40):
    case, refs = random40
    bf = _with_env(STREAMED, lambda: _batch(mm, wl, case[0]))
    assert "mm_window_fwd_kernel<0,global>" in bf.kernels("window"), bf.kernels("window")
    _check(bf, _run(bf, case), refs, case[2], "streamed instance")
    bf = _with_env(BIGV, lambda: _batch(mm, wl, case[0]))
    assert "mm_window_bwd_kernel<8,global>" in bf.kernels("window"), bf.kernels("window")
    _check(bf, _run(bf, case), refs, case[2], "vectors in global memory")


def test_vectors_global_by_the_plan(mm, wl, torch):
    """12 500 states: four vectors of 4 bytes per state exceed the 160 KB of a compute unit, the plan itself puts them in global
    memory (as the arc entry's, whose LDS size this entry's is)."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    V = np.random.default_rng(4).standard_normal((2, 12, g.P)).astype(np.float32)
    case = ([g, g], V, np.array([12, 7], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([5, 7], dtype=np.int32))
    bf = _batch(mm, wl, case[0])
    assert "mm_window_fwd_kernel<8,global>" in bf.kernels("window") and "global" in bf.kernels("arcs"), bf.kernels("window")
    _check(bf, _run(bf, case), references(case), case[2], "12500 states")


def test_more_pdfs_than_threads(mm, wl, torch):
    """600 pdfs against at most 512 threads: both kernels stage a frame's emissions in two parts."""
    g = wl.random_fsm(700, 600, 3.0, seed=9)
    V = np.random.default_rng(10).standard_normal((3, 14, g.P)).astype(np.float32)
    case = ([g] * 3, V, np.array([14, 9, 2], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32), np.array([7, 9, 1], dtype=np.int32))
    bf = _batch(mm, wl, case[0])
    _check(bf, _run(bf, case), references(case), case[2], "700 states, 600 pdfs")


def test_closed_is_pdfposteriors_and_open_ends_as_the_filter(mm, wl, torch, random40):
    """(a) and (b), against the entries themselves."""
    (gs, V, lens, _, _), _ = random40
    bf = _batch(mm, wl, gs)
    B = len(gs)
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    gamma, ttl, lcommit = bf.windowposteriors(V, lens, closed=np.ones(B, dtype=np.int32))
    ok = np.isfinite(t_pdf)
    assert (np.isfinite(ttl) == ok).all() and np.allclose(ttl[ok], t_pdf[ok], rtol=1e-5, atol=1e-4), (ttl, t_pdf)
    for b in range(B):
        if ok[b]:
            check_gamma(gamma[b][None], g_pdf[b].astype(np.float64)[None], [int(lens[b])])
        else:
            assert (gamma[b] == 0).all()
    filt, incr, t_f, so_f = bf.filterposteriors(V, lens, want_state=True)
    gamma, ttl, lcommit, so = bf.windowposteriors(V, lens, want_state=True)
    alive = np.isfinite(incr).all(-1) & (lens > 0)
    assert alive.sum() == 4 and (np.isfinite(ttl) == alive).all()
    assert np.allclose(ttl[alive], incr.sum(-1, dtype=np.float64)[alive], rtol=1e-5, atol=1e-4)
    assert np.allclose(lcommit[alive], ttl[alive], rtol=1e-5, atol=1e-4)
    for b in np.flatnonzero(alive):
        L = int(lens[b])
        check_gamma(gamma[b, L - 1][None, None], filt[b, L - 1].astype(np.float64)[None, None], [1])
        check_against_reference(gamma[b], ttl[b], lcommit[b], _seg(bf, so, b), (gamma[b].astype(np.float64), float(ttl[b]), float(lcommit[b]), _seg(bf, so_f, b).astype(np.float64)), L)


def test_rewindowing_on_the_device_with_the_state_in_place(mm, wl, torch):
    """(c): the second window runs from the first one's state_out, read and written in one buffer; each side against the float64
    reference of ITS definition (the second: the whole window's gamma behind c, ttl - lcommit), not against the other side."""
    gs, V, lens, closed, _ = case_den600(wl)
    B, M, P = V.shape
    c = np.array([60, 1, 119, 20], dtype=np.int32)
    case1 = (gs, V, lens, closed, c)
    refs1 = references(case1)
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    g1, t1, l1, state = bf.windowposteriors(Vt, lt, closed=closed, commit=c, want_state=True)
    _check(bf, [t.cpu().numpy() for t in (g1, t1, l1, state)], refs1, lens, "first window")
    # the frames behind c, per utterance, moved to the front
    V2 = np.zeros_like(V)
    for b in range(B):
        V2[b, : M - c[b]] = V[b, c[b] :]
    lens2 = lens - c
    g2, t2, l2, s2 = bf.windowposteriors(torch.from_numpy(V2).cuda(), torch.from_numpy(lens2).cuda(), state=state, closed=closed, want_state=state)
    torch.cuda.synchronize()
    assert s2 is state
    whole = references((gs, V, lens, closed, None))  # commit = len: state_out and lcommit behind the last frame
    refs2 = []
    for b in range(B):
        gam = np.zeros((M, P))
        gam[: M - c[b]] = whole[b][0][c[b] :]
        refs2.append((gam, whole[b][1] - refs1[b][2], whole[b][2] - refs1[b][2], whole[b][3]))
    _check(bf, [t.cpu().numpy() for t in (g2, t2, l2, s2)], refs2, lens2, "second window, state in place")


def test_the_level_of_a_frame(mm, wl, torch, random40):
    """(d): +100 and -150 nats on one frame: gamma against the UNSHIFTED reference, ttl (and lcommit behind the frame) moved by it."""
    case, refs = random40
    gs, V, lens, closed, commit = case
    bf = _batch(mm, wl, gs)
    n = 5
    for shift in (100.0, -150.0):
        Vs = V.copy()
        Vs[:, n] += np.float32(shift)
        refs_s = []
        for b, r in enumerate(refs):
            c = min(max(int(commit[b]), 0), int(lens[b]))
            refs_s.append((r[0], r[1] + shift * (lens[b] > n), r[2] + shift * (c > n), r[3]))
        _check(bf, _run(bf, (gs, Vs, lens, closed, commit)), refs_s, lens, f"frame {n} {shift:+g}")


def test_bit_identical_repeats_and_null_outputs(mm, wl, torch):
    """(g): no atomics; gamma does not depend on which of the other outputs are asked for, nor on the frames behind len."""
    lib = _lib(mm)
    gs, V, lens, closed, commit = case_den600(wl)
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    ct, mt = torch.from_numpy(closed).cuda(), torch.from_numpy(commit).cuda()
    out0 = bf.windowposteriors(Vt, lt, closed=ct, commit=mt, want_state=True)
    out1 = bf.windowposteriors(Vt, lt, closed=ct, commit=mt, want_state=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    # (f): what lies behind len is not read
    V2 = V.copy()
    for b in range(B):
        V2[b, lens[b] :] = 3.0
    out2 = bf.windowposteriors(torch.from_numpy(V2).cuda(), lt, closed=ct, commit=mt, want_state=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out2))
    gamma = torch.full((B, N, P), 7.0, device="cuda")
    rc = lib.mm_windowposteriors_f32(bf._h, Vt.data_ptr(), N * P, P, lt.data_ptr(), N, None, ct.data_ptr(), mt.data_ptr(), None, None,
                                     gamma.data_ptr(), N * P, P, 1, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gamma, out0[0])


def test_column_major_output_strides(mm, wl, torch):
    """The reference's B x P x N column-major layout: g_stride_b = 1, g_stride_p = B, g_stride_n = B * P; and the module-level
    call in pdfposteriors' shape."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 50, g.P
    bf = _batch(mm, wl, [g] * B)
    V = torch.from_numpy(np.random.default_rng(8).standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([50, 41, 50, 13], dtype=torch.int32, device="cuda")
    closed = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device="cuda")
    gamma0, ttl0, _ = bf.windowposteriors(V, lens, closed=closed)
    gamma = torch.full((N, P, B), 7.0, device="cuda")  # element (b, n, p) at b + p * B + n * B * P
    ttl = torch.empty(B, device="cuda")
    rc = lib.mm_windowposteriors_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, None, closed.data_ptr(), None, None, None,
                                     gamma.data_ptr(), 1, B * P, B, ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gamma.permute(2, 0, 1), gamma0) and torch.equal(ttl, ttl0)
    Vn, ln = V.cpu().numpy(), lens.cpu().numpy()
    Vh = [mm.expand(Vn[b].T, int(ln[b])) for b in range(B)]
    g_mod, t_mod = mm.windowposteriors(bf, Vh, closed=closed)
    assert g_mod.shape == (B, P, N) and np.array_equal(g_mod, gamma0.cpu().numpy().transpose(0, 2, 1)) and np.array_equal(t_mod, ttl0.cpu().numpy())
    g_dev, t_dev = mm.windowposteriors(bf, torch.from_numpy(np.stack(Vh)).cuda(), seqlengths=ln, closed=closed)
    assert torch.equal(g_dev, gamma0.transpose(1, 2)) and torch.equal(t_dev, ttl0)


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    gamma = torch.zeros((B, N, P), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, gamma_ptr=gamma.data_ptr(), gsn=P):
        return lib.mm_windowposteriors_f32(h, V.data_ptr(), N * P, P, None, N, None, None, None, None, None, gamma_ptr, N * P, gsn, 1, None, st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(tb._h) == -4
    assert b"log" in lib.mm_last_error()
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h) == -4
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h, gamma_ptr=None) == -1
    assert call(lb._h, gsn=P - 1) == -2
    assert call(lb._h) == 0
    torch.cuda.synchronize()
    for b in (tb, pb):
        with pytest.raises(mm.MarkovModelsAMDError):
            b.kernels("window")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.windowposteriors(V, None)


def test_fixed_lag_smoother(mm, wl, torch):
    """Irregular chunks (1, 37, 50, 62), lag 20, ragged lengths, utterance 3 finished early while the others go on: every emitted
    frame against the reference of the whole prefix pushed by then, the frames of finish against the smoothing posteriors of the
    whole audio, loglik + the closed ttl against pdfposteriors' log Z."""
    g = wl.lfmmi_denominator(600, 40, seed=5)
    B, N, lag = 4, 150, 20
    gs = [g] * B
    lens = np.array([150, 120, 150, 33], dtype=np.int32)
    V = np.random.default_rng(1).standard_normal((B, N, g.P)).astype(np.float32)
    bf = _batch(mm, wl, gs)
    _, z_pdf = bf.pdfposteriors(V, lens)
    closed_refs = references((gs, V, lens, np.ones(B, dtype=np.int32), None))
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    sm = mm.FixedLagSmoother(bf, lag)
    emitted = np.zeros(B, dtype=np.int64)
    done = np.zeros(B, dtype=bool)
    worst = 0.0

    def finish(mask):
        nonlocal worst
        gam, cnt, logz = sm.finish(mask, as_numpy=True)
        for b in np.flatnonzero(mask):
            assert emitted[b] + cnt[b] == lens[b]
            ref = np.zeros((lag, g.P))
            ref[: cnt[b]] = closed_refs[b][0][emitted[b] : lens[b]]
            out = np.zeros((lag, g.P))
            out[: cnt[b]] = gam[b, : cnt[b]]
            worst = max(worst, check_gamma(out[None], ref[None], [int(cnt[b])]))
            assert np.isclose(logz[b], closed_refs[b][1], rtol=1e-5, atol=1e-4) and np.isclose(logz[b], z_pdf[b], rtol=1e-5, atol=1e-4), (b, logz[b], z_pdf[b])
            emitted[b] += cnt[b]
            done[b] = True
        assert (cnt[~np.asarray(mask)] == 0).all()

    n0 = 0
    for ch in (1, 37, 50, 62):
        cl = torch.clamp(lt - n0, 0, ch).to(torch.int32)
        gam, cnt = sm.push(Vt[:, n0 : n0 + ch], cl)
        n0 += ch
        gam, cnt = gam.cpu().numpy(), cnt.cpu().numpy()
        pushed = np.minimum(lens, n0)
        for b in range(B):
            if done[b]:
                assert cnt[b] == 0
                continue
            assert cnt[b] == max(0, pushed[b] - lag) - emitted[b] and (gam[b, cnt[b] :] == 0).all()
            if cnt[b]:
                prefix = wr.reference(g, V[b].astype(np.float64), int(pushed[b]), int(pushed[b]))
                out = np.zeros((ch, g.P))
                out[: cnt[b]] = gam[b, : cnt[b]]
                ref = np.zeros((ch, g.P))
                ref[: cnt[b]] = prefix[0][emitted[b] : emitted[b] + cnt[b]]
                worst = max(worst, check_gamma(out[None], ref[None], [int(cnt[b])]))
                emitted[b] += cnt[b]
        if n0 == 38:  # utterance 3 (33 frames) has ended: finished alone, the others go on
            finish(np.array([False, False, False, True]))
    finish(~done)
    torch.cuda.synchronize()
    assert (emitted == lens).all() and float(sm.loglik.abs().sum()) == 0 and int(sm.npending.sum()) == 0
    print(f"fixed-lag smoother: worst gamma error over its bar {worst:.3g}")
