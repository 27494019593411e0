"""Segment posteriors (mm_segmentposteriors_f32) on the MI355X against the float64 reference of tests/segment_reference.py, and the
consequences the header states: (a) without an end vector = windowposteriors, (b) exact chaining with the end vector fed back in
place, (c) the level of a frame, (d) the level of the end vector, (g) bit-identical repeats and the outputs that may be NULL; the
kernel instances, more pdfs than threads, output strides, hipGraph capture, error codes; BatchedFSM.chunkedposteriors against the
whole closed reference and pdfposteriors' log Z with no call beyond `chunk` frames, and longform.chunked_loglik's gradient.

The bars are the project's own (tests/test_segmentposteriors.py check_against_reference): gamma has check_gamma of
tests/test_gpu_parity.py, ttl and lend np.isclose(rtol=1e-5, atol=1e-4), end_out the state_out bar of
test_windowposteriors.check_against_reference with -inf exactly where the reference has it.  Every output of every utterance of
every test is compared; segments without mass or without a frame by their exact conventions.  The reference's float32 mode stays
below 0.01 of each bar on these inputs (test_segmentposteriors.test_float32_mode_within_the_bars)."""
import copy
import ctypes as C

import numpy as np
import pytest

import filter_reference as fr
import segment_reference as sr
import window_reference as wr
from test_gpu_parity import _with_env, check_gamma
from test_segmentposteriors import (CHUNK_LENS, case_big, case_den, case_distinct, case_many_pdfs, case_random40, case_random40_other_ends,
                                    check_against_reference, references)
from test_windowposteriors import case_den600

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


def _seg(bf, v, b):
    return v[int(bf.state_offsets[b]) : int(bf.state_offsets[b + 1])]


def _flat(gs, rows):
    """Per-utterance vectors as the entry's one buffer [total_states]; a None row: ln alpha_hat (what a NULL state_in stands for)."""
    return np.concatenate([fr.start_vector(g).astype(np.float32) if r is None else np.asarray(r, dtype=np.float32) for g, r in zip(gs, rows)])


def _run(bf, case, **kw):
    gs, V, lens, modes, states, end = case
    state = None if all(s is None for s in states) else _flat(gs, states)
    return bf.segmentposteriors(V, lens, state=state, end_mode=modes, end=_flat(gs, list(end)), want_end=True, **kw)


def _check(bf, out, refs, lens, what=""):
    """Every utterance against its reference; prints and returns the worst error over each bar."""
    gamma, ttl, lend, eo = out
    worst = np.zeros(3)
    for b, ref in enumerate(refs):
        worst = np.maximum(worst, check_against_reference(gamma[b], ttl[b], lend[b], _seg(bf, eo, b), ref, int(lens[b])))
    print(f"{what}: worst error over its bar: gamma {worst[0]:.3g}, ttl / lend {worst[1]:.3g}, end_out {worst[2]:.3g}")
    return worst


@pytest.fixture(scope="module")
def random40(wl):
    case = case_random40(wl)
    return case, references(case)


@pytest.fixture(scope="module")
def den(wl):
    case = case_den(wl)
    return case, references(case)


def test_random_graph_lengths_and_end_modes(mm, wl, torch, random40):
    case, refs = random40
    gs, V, lens, modes, states, end = case
    bf = _batch(mm, wl, gs)
    assert "mm_window_fwd_kernel<8,lds>" in bf.kernels("segment") and "mm_segment_bwd_kernel<8,lds>" in bf.kernels("segment"), bf.kernels("segment")
    out = _run(bf, case)
    _check(bf, out, refs, lens, "random40")
    gamma, ttl, lend, eo = out

    def dead(b):
        return (gamma[b] == 0).all() and np.isneginf(ttl[b]) and np.isneginf(lend[b]) and np.isneginf(_seg(bf, eo, b)).all()

    # utterance 4 dies at frame 14; utterance 2's end vector has no live state: nothing to hand back either
    assert dead(4) and dead(2)
    # utterance 3: len = 0 -- the carried end vector passes through as given, its final entry included
    assert (gamma[3] == 0).all() and np.isneginf(ttl[3]) and lend[3] == 0 and np.array_equal(_seg(bf, eo, 3), end[3])
    assert np.isfinite(ttl[[0, 1, 5]]).all() and np.isfinite(lend[[0, 1, 5]]).all()
    for b in (0, 1, 5):
        assert _seg(bf, eo, b).max() == 0 and np.isneginf(_seg(bf, eo, b)[-1])
    # ... utterance 2 alive on a live end vector, utterance 5 without mass
    case2 = case_random40_other_ends(wl)
    out = _run(bf, case2)
    _check(bf, out, references(case2), lens, "random40, the other ends")
    assert np.isfinite(out[1][2]) and np.isneginf(out[1][5]) and np.isneginf(_seg(bf, out[3], 5)).all()
    # ... and no frame with an open end and with the final weights
    lens0 = np.zeros(6, dtype=np.int32)
    case3 = (gs, V, lens0, modes, states, end)
    _check(bf, _run(bf, case3), references(case3), lens0, "random40, no frame")


def test_streamed_and_global_vector_instances(mm, wl, torch, random40):
    case, refs = random40
    bf = _with_env(STREAMED, lambda: _batch(mm, wl, case[0]))
    assert "mm_segment_bwd_kernel<0,global>" in bf.kernels("segment"), bf.kernels("segment")
    _check(bf, _run(bf, case), refs, case[2], "streamed instance")
    bf = _with_env(BIGV, lambda: _batch(mm, wl, case[0]))
    assert "mm_segment_bwd_kernel<8,global>" in bf.kernels("segment"), bf.kernels("segment")
    _check(bf, _run(bf, case), refs, case[2], "vectors in global memory")


def test_vectors_global_by_the_plan(mm, wl, torch):
    """12 500 states: the plan itself puts the vectors in global memory (the window entry's LDS size)."""
    case = case_big(wl)
    bf = _batch(mm, wl, case[0])
    assert "mm_segment_bwd_kernel<8,global>" in bf.kernels("segment"), bf.kernels("segment")
    _check(bf, _run(bf, case), references(case), case[2], "12500 states")


def test_distinct_graphs(mm, wl, torch):
    case = case_distinct(wl)
    bf = _batch(mm, wl, case[0])
    out = _run(bf, case)
    assert np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
    _check(bf, out, references(case), case[2], "distinct graphs")


def test_more_pdfs_than_threads(mm, wl, torch):
    """600 pdfs against at most 512 threads: both kernels stage a frame's emissions in two parts."""
    case = case_many_pdfs(wl)
    bf = _batch(mm, wl, case[0])
    _check(bf, _run(bf, case), references(case), case[2], "700 states, 600 pdfs")


def test_denominator_graph(mm, wl, torch, den):
    case, refs = den
    bf = _batch(mm, wl, case[0])
    out = _run(bf, case)
    assert np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
    _check(bf, out, refs, case[2], "denominator graph, 600 states")


def test_without_an_end_vector_it_is_the_window(mm, wl, torch, random40):
    """(a): end_in NULL against windowposteriors with closed = end_mode on the same inputs, within the bars."""
    (gs, V, lens, modes, states, _), _ = random40
    bf = _batch(mm, wl, gs)
    state = _flat(gs, states)
    g_w, t_w, _ = bf.windowposteriors(V, lens, state=state, closed=modes)
    g_s, t_s, l_s = bf.segmentposteriors(V, lens, state=state, end_mode=modes)
    ok = np.isfinite(t_w)
    assert ok.sum() == 4 and (np.isfinite(t_s) == ok).all() and np.allclose(t_s[ok], t_w[ok], rtol=1e-5, atol=1e-4), (t_s, t_w)
    for b in range(len(gs)):
        if ok[b]:
            check_gamma(g_s[b][None], g_w[b].astype(np.float64)[None], [int(lens[b])])
        else:
            assert (g_s[b] == 0).all()
    print(f"end_in NULL against windowposteriors: gamma bits equal {np.array_equal(g_s, g_w)}, ttl bits equal {np.array_equal(t_s, t_w)}")


def test_chaining_on_the_device_with_the_end_vector_in_place(mm, wl, torch, den):
    """(b): segment B runs from the filter's state behind A's frames, A ends on B's end_out, read and written in one buffer; each
    side's gamma against the float64 reference of the ONE call over all frames with B's end, A's other outputs against what follows
    from it, B's against the reference of B itself from the float64 filter state."""
    (gs, V, lens, modes, _, end), _ = den
    B, M, P = V.shape
    L1 = np.array([60, 1, 119, 20], dtype=np.int32)
    one = references((gs, V, lens, modes, [None] * B, end))
    bf = _batch(mm, wl, gs)
    Vt = torch.from_numpy(V).cuda()
    _, _, _, state = bf.filterposteriors(Vt, torch.from_numpy(L1).cuda(), want_state=True, want_filt=False)
    V2 = np.zeros_like(V)
    for b in range(B):
        V2[b, : M - L1[b]] = V[b, L1[b] :]
    endv = torch.from_numpy(_flat(gs, list(end))).cuda()
    gB, tB, lB, eB = bf.segmentposteriors(torch.from_numpy(V2).cuda(), torch.from_numpy(lens - L1).cuda(), state=state,
                                          end_mode=torch.from_numpy(modes).cuda(), end=endv, want_end=endv)
    assert eB is endv
    eB = eB.clone()
    gA, tA, lA, eA = bf.segmentposteriors(Vt, torch.from_numpy(L1).cuda(), end_mode=torch.full((B,), 2, dtype=torch.int32, device="cuda"),
                                          end=endv, want_end=endv)
    torch.cuda.synchronize()
    assert eA is endv
    gA, tA, lA, eA, gB, tB, lB, eB = (t.cpu().numpy() for t in (gA, tA, lA, eA, gB, tB, lB, eB))
    refsA, refsB = [], []
    for b in range(B):
        g1, t1, l1, e1 = one[b]
        gam = np.zeros((M, P))
        gam[: L1[b]] = g1[: L1[b]]
        refsA.append((gam, t1 - float(lB[b]), l1 - float(lB[b]), e1))
        gam = np.zeros((M, P))
        gam[: M - L1[b]] = g1[L1[b] :]
        own = sr.reference(gs[b], V2[b].astype(np.float64), int(lens[b] - L1[b]), M, fr.reference(gs[b], V[b].astype(np.float64), int(L1[b]), M)[3],
                           int(modes[b]), end[b])
        assert np.abs(own[0] - gam).max() <= 1e-9
        refsB.append((gam, own[1], own[2], own[3]))
    _check(bf, (gA, tA, lA, eA), refsA, L1, "segment A on B's end vector, in place")
    _check(bf, (gB, tB, lB, eB), refsB, lens - L1, "segment B from the filter's state")
    for b in range(B):
        assert np.isclose(float(tA[b]) + float(lB[b]), one[b][1], rtol=1e-5, atol=1e-4) and np.isclose(float(lA[b]) + float(lB[b]), one[b][2], rtol=1e-5, atol=1e-4)


def test_the_level_of_a_frame_and_of_the_end_vector(mm, wl, torch, random40):
    """(c): +100 and -150 nats on one frame: gamma and end_out against the UNSHIFTED reference, ttl and lend moved by it.  (d): +50 on
    end_in: ttl and lend of the carried utterances moved by it, nothing else."""
    case, refs = random40
    gs, V, lens, modes, states, end = case
    bf = _batch(mm, wl, gs)
    n = 5
    for shift in (100.0, -150.0):
        Vs = V.copy()
        Vs[:, n] += np.float32(shift)
        refs_s = [(r[0], r[1] + shift * (lens[b] > n), r[2] + shift * (lens[b] > n), r[3]) for b, r in enumerate(refs)]
        _check(bf, _run(bf, (gs, Vs, lens, modes, states, end)), refs_s, lens, f"frame {n} {shift:+g}")
    carried = (modes == 2) & (lens > 0)
    refs_e = [(r[0], r[1] + 50.0 * carried[b], r[2] + 50.0 * carried[b], r[3] + 50.0 * ((modes[b] == 2) and lens[b] == 0)) for b, r in enumerate(refs)]
    _check(bf, _run(bf, (gs, V, lens, modes, states, end + np.float32(50.0))), refs_e, lens, "end_in +50")


def test_bit_identical_repeats_null_outputs_strides_and_capture(mm, wl, torch, den):
    """(g): no atomics; gamma does not depend on which of the other outputs are asked for; the reference's column-major layout; one
    hipGraph capture behind a first call."""
    lib = _lib(mm)
    (gs, V, lens, modes, states, end), _ = den
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt, lt, mt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(modes).cuda()
    st, et = torch.from_numpy(_flat(gs, states)).cuda(), torch.from_numpy(_flat(gs, list(end))).cuda()

    def run():
        return bf.segmentposteriors(Vt, lt, state=st, end_mode=mt, end=et, want_end=True)

    out0, out1 = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gamma = torch.full((B, N, P), 7.0, device="cuda")
    rc = lib.mm_segmentposteriors_f32(bf._h, Vt.data_ptr(), N * P, P, lt.data_ptr(), N, st.data_ptr(), mt.data_ptr(), et.data_ptr(), None, None,
                                      gamma.data_ptr(), N * P, P, 1, None, stream)
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gamma, out0[0])
    gcm = torch.full((N, P, B), 7.0, device="cuda")  # element (b, n, p) at b + p * B + n * B * P
    ttl, lend, eo = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(et)
    rc = lib.mm_segmentposteriors_f32(bf._h, Vt.data_ptr(), N * P, P, lt.data_ptr(), N, st.data_ptr(), mt.data_ptr(), et.data_ptr(), eo.data_ptr(),
                                      lend.data_ptr(), gcm.data_ptr(), 1, B * P, B, ttl.data_ptr(), stream)
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gcm.permute(2, 0, 1), out0[0]) and torch.equal(ttl, out0[1]) and torch.equal(lend, out0[2]) and torch.equal(eo, out0[3])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = run()
    for _ in range(2):
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out0, out2))


def test_capture_before_a_first_call_is_refused(mm, wl, torch):
    """The item forms are never put on the device during a capture.  (A batch of the wave kernel is created without them.)"""
    g = wl.lexicon_fsm(300, 20, seed=2, hubs=1)
    fresh = _batch(mm, wl, [g] * 5)
    assert "mm_wave_kernel" in fresh.kernels("log"), fresh.kernels("log")
    N = 40
    Vn = np.random.default_rng(9).standard_normal((5, N, g.P)).astype(np.float32)
    ln = np.array([40, 31, 40, 12, 25], dtype=np.int32)
    V, lens = torch.from_numpy(Vn).cuda(), torch.from_numpy(ln).cuda()
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.segmentposteriors(V, lens)
    assert ei.value.code == -1 and "not on the device yet" in str(ei.value)
    # ... and the batch works afterwards
    modes = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    out = fresh.segmentposteriors(V, lens, end_mode=modes, want_end=True)
    torch.cuda.synchronize()
    case = ([g] * 5, Vn, ln, modes, [None] * 5, None)
    _check(fresh, [t.cpu().numpy() for t in out], references(case), ln, "wave-kernel batch")


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    gamma = torch.zeros((B, N, P), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, gamma_ptr=gamma.data_ptr(), gsn=P):
        return lib.mm_segmentposteriors_f32(h, V.data_ptr(), N * P, P, None, N, None, None, None, None, None, gamma_ptr, N * P, gsn, 1, None, st)

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
            b.kernels("segment")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.segmentposteriors(V, None)


@pytest.fixture(scope="module")
def chunk_case(wl):
    gs, V, _, _, _ = case_den600(wl)
    N = V.shape[1]
    whole = [wr.reference(gs[b], V[b].astype(np.float64), int(CHUNK_LENS[b]), N, None, True) for b in range(len(gs))]
    return gs, V, CHUNK_LENS, whole


def _limited(bf, chunk, seen):
    """The two entries of the driver wrapped: no call may see more than `chunk` frames."""
    fil, seg = bf.filterposteriors, bf.segmentposteriors

    def filterposteriors(V, *a, **kw):
        seen.append(("filter", V.shape[1]))
        assert V.shape[1] <= chunk
        return fil(V, *a, **kw)

    def segmentposteriors(V, *a, **kw):
        seen.append(("segment", V.shape[1]))
        assert V.shape[1] <= chunk
        return seg(V, *a, **kw)

    bf.filterposteriors, bf.segmentposteriors = filterposteriors, segmentposteriors


@pytest.mark.parametrize("chunk", [37, 40])
def test_chunkedposteriors(mm, wl, torch, chunk_case, chunk):
    """Chunk 40: utterance 1 (120 frames) ends exactly on a boundary, utterance 3 (33 frames) lies wholly inside chunk 0."""
    gs, V, lens, whole = chunk_case
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    _, z_pdf = bf.pdfposteriors(V, lens)
    seen = []
    _limited(bf, chunk, seen)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    out = torch.full((B, N, P), 7.0, device="cuda")
    gamma, ttl = bf.chunkedposteriors(Vt, lt, chunk=chunk, out=out)
    torch.cuda.synchronize()
    K = -(-N // chunk)
    assert gamma is out and seen == [("filter", min(chunk, N - k * chunk)) for k in range(K)] + [("segment", min(chunk, N - k * chunk)) for k in range(K - 1, -1, -1)]
    gamma, ttl = gamma.cpu().numpy(), ttl.cpu().numpy()
    worst = np.zeros(2)
    for b in range(B):
        worst[0] = max(worst[0], check_gamma(gamma[b][None], whole[b][0][None], [int(lens[b])]))
        assert np.isclose(ttl[b], whole[b][1], rtol=1e-5, atol=1e-4) and np.isclose(ttl[b], z_pdf[b], rtol=1e-5, atol=1e-4), (b, ttl[b], whole[b][1], z_pdf[b])
        worst[1] = max(worst[1], abs(ttl[b] - whole[b][1]) / (1e-4 + 1e-5 * abs(whole[b][1])))
    print(f"chunkedposteriors, chunk {chunk}: worst error over its bar: gamma {worst[0]:.3g}, ttl {worst[1]:.3g}")


def test_chunkedposteriors_one_chunk_and_a_dead_utterance(mm, wl, torch, chunk_case):
    gs, V, lens, whole = chunk_case
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    # chunk >= N is one segment call
    for chunk in (N, N + 50):
        g1, t1 = bf.chunkedposteriors(Vt, lt, chunk=chunk)
        g2, t2, _ = bf.segmentposteriors(Vt, lt, end_mode=torch.ones(B, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(t1, t2)
    # utterance 2 dies at frame 70, in the second of four chunks: gamma = 0 in every chunk, before and behind
    Vd = V.copy()
    Vd[2, 70, :] = -np.inf
    gamma, ttl = bf.chunkedposteriors(Vd, lens, chunk=40)
    assert (gamma[2] == 0).all() and np.isneginf(ttl[2]) and not np.isnan(gamma).any()
    for b in (0, 1, 3):
        check_gamma(gamma[b][None], whole[b][0][None], [int(lens[b])])
        assert np.isclose(ttl[b], whole[b][1], rtol=1e-5, atol=1e-4)
    # the module-level call in pdfposteriors' shape
    Vh = [mm.expand(V[b].T, int(lens[b])) for b in range(B)]
    g_mod, t_mod = mm.chunkedposteriors(bf, Vh, chunk=40)
    g_ref, t_ref = bf.chunkedposteriors(V, lens, chunk=40)
    assert g_mod.shape == (B, P, N) and np.array_equal(g_mod, g_ref.transpose(0, 2, 1)) and np.array_equal(t_mod, t_ref)


def test_chunked_loglik_gradient(mm, wl, torch, chunk_case):
    """d (sum_b w_b log Z_b) / d V = w_b gamma_b: the reference gamma times the upstream gradient."""
    gs, V, lens, whole = chunk_case
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt = torch.from_numpy(V).cuda().requires_grad_(True)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], device="cuda")
    logz = mm.longform.chunked_loglik(Vt, bf, torch.from_numpy(lens).cuda(), 40)
    assert logz.shape == (B,)
    (logz * w).sum().backward()
    torch.cuda.synchronize()
    grad, wn = Vt.grad.cpu().numpy(), w.cpu().numpy()
    for b in range(B):
        assert np.isclose(float(logz[b].detach()), whole[b][1], rtol=1e-5, atol=1e-4)
        check_gamma((grad[b] / wn[b])[None], whole[b][0][None], [int(lens[b])])
