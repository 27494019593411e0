"""Forward filtering posteriors with a carried state (mm_filterposteriors_f32) on the MI355X against the float64 reference of
tests/filter_reference.py, and the properties of the entry: causality bit for bit, exact chunking through streaming.ForwardFilter,
the carried state in place, the level of V, the kernel instances, agreement with pdfposteriors, the likelihood-only call,
bit-identical repeats, hipGraph capture, error codes, output strides.

The bars are the project's own (tests/test_filterposteriors.py check_against_reference): filt has check_gamma of
tests/test_gpu_parity.py, incr per frame and ttl np.allclose(rtol=1e-5, atol=1e-4), state_out 1e-4 relative on the log where the
reference exceeds ln 1e-30 and -inf where the reference is -inf.  Every utterance of every test is compared; dead and empty
utterances by their exact conventions.  The reference's float32 mode stays below 0.004 of each bar on the small inputs
(test_float32_mode_within_the_bars), so no bar had to be measured."""
import copy
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import filter_reference as fr
from test_filterposteriors import check_against_reference
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}


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


def _log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def _refs(gs, V, lens):
    """The float64 references of a batch, computed once and shared: a list of (filt, incr, ttl, state_out)."""
    return [fr.reference(gs[b], V[b].astype(np.float64), int(lens[b]), V.shape[1]) for b in range(len(gs))]


def _seg(bf, so, b):
    return so[int(bf.state_offsets[b]) : int(bf.state_offsets[b + 1])]


def _check(bf, out, refs, lens, what=""):
    """Every utterance against its reference; prints and returns the worst error over each bar."""
    filt, incr, ttl, so = out
    worst = np.zeros(3)
    for b, ref in enumerate(refs):
        w = check_against_reference(filt[b], incr[b], ttl[b], _seg(bf, so, b), ref, int(lens[b]))
        worst = np.maximum(worst, w)
    print(f"{what}: worst error over its bar: filt {worst[0]:.3g}, incr / ttl {worst[1]:.3g}, state_out {worst[2]:.3g}")
    return worst


def _run(bf, V, lens, **kw):
    return bf.filterposteriors(V, lens, want_state=True, **kw)


def case_random40(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([30, 25, 1, 0, 28, 30], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((6, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf  # a frame with -inf entries
    V[4, 4, :] = -np.inf   # utterance 4 dies at frame 4
    V[5, :15] = V[0, :15]  # utterance 5 is utterance 0 up to frame 14
    return [g] * 6, V, lens


def test_random_graph_lengths_dead_frames_and_causality(mm, wl, torch):
    gs, V, lens = case_random40(wl)
    bf = _batch(mm, wl, gs)
    out = _run(bf, V, lens)
    refs = _refs(gs, V, lens)
    _check(bf, out, refs, lens, "random40")
    filt, incr, ttl, so = out
    # utterance 4: alive up to frame 3 (checked above against the reference), the conventions from frame 4 on
    assert (filt[4, :4].sum(-1) > 0.99).all() and np.isfinite(incr[4, :4]).all()
    assert (filt[4, 4:] == 0).all() and np.isneginf(incr[4, 4:28]).all() and (incr[4, 28:] == 0).all()
    assert np.isneginf(ttl[4]) and np.isneginf(_seg(bf, so, 4)).all()
    # utterance 3: len = 0 -- the reset vector
    assert (filt[3] == 0).all() and (incr[3] == 0).all() and np.isneginf(ttl[3])
    assert np.isfinite(ttl[[0, 1, 2, 5]]).all()
    # causality, bit for bit
    assert np.array_equal(filt[5, :15], filt[0, :15]) and np.array_equal(incr[5, :15], incr[0, :15])
    assert not np.array_equal(filt[5, 15:], filt[0, 15:])


def _distinct(wl):
    return [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]


def test_distinct_graphs(mm, wl, torch):
    gs = _distinct(wl)
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    bf = _batch(mm, wl, gs)
    out = _run(bf, V, lens)
    assert np.isfinite(out[2]).all()
    _check(bf, out, _refs(gs, V, lens), lens, "distinct graphs")


def _push_all(ff, Vt, lt, chunks, torch):
    fs, incs, n0 = [], [], 0
    for c in chunks:
        f, i = ff.push(Vt[:, n0 : n0 + c], torch.clamp(lt - n0, 0, c).to(torch.int32))
        fs.append(f)
        incs.append(i)
        n0 += c
    return torch.cat(fs, 1), torch.cat(incs, 1)


def test_chunking_through_forward_filter(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    B, N = 4, 150
    gs = [g] * B
    lens = np.array([150, 120, 150, 33], dtype=np.int32)
    V = np.random.default_rng(1).standard_normal((B, N, g.P)).astype(np.float32)
    refs = _refs(gs, V, lens)
    z_ref = np.array([r[2] for r in refs])
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    whole = _run(bf, Vt, lt)
    _check(bf, [t.cpu().numpy() for t in whole], refs, lens, "one call")
    ff = mm.ForwardFilter(bf)
    first = None
    for chunks in ((50, 50, 50), (1, 148, 1)):
        ff.reset()
        filt, incr = _push_all(ff, Vt, lt, chunks, torch)
        torch.cuda.synchronize()
        z = ff.logz().cpu().numpy()
        ttl = (ff.loglik + ff.state[ff._final].double()).float().cpu().numpy()
        _check(bf, (filt.cpu().numpy(), incr.cpu().numpy(), ttl, ff.state.cpu().numpy()), refs, lens, f"chunks {chunks}")
        assert np.allclose(z, z_ref, rtol=1e-5, atol=1e-4), (chunks, z, z_ref)
        assert np.allclose(ff.loglik.cpu().numpy(), [r[1].sum() for r in refs], rtol=1e-5, atol=1e-4)
        if first is None:
            first = (filt.clone(), incr.clone())
    # the carried state in place: the same bits as separate buffers
    s0 = whole[3]
    a = bf.filterposteriors(Vt, lt, state=s0, want_state=True)
    s1 = s0.clone()
    b = bf.filterposteriors(Vt, lt, state=s1, want_state=s1)
    torch.cuda.synchronize()
    assert b[3] is s1 and all(torch.equal(x, y) for x, y in zip(a, b))
    # reset(mask) of one utterance reproduces a fresh start; the others stand still on lens = 0
    ff.reset()
    ff.push(Vt[:, :50], torch.clamp(lt, 0, 50).to(torch.int32))
    lk1 = ff.loglik.clone()
    ff.push(Vt[:, 50:], torch.clamp(lt - 50, 0, 100).to(torch.int32))
    state_before, lk_before = ff.state.clone(), ff.loglik.clone()
    ff.reset([False, True, False, False])
    f, i = ff.push(Vt[:, :50], torch.tensor([0, 50, 0, 0], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(f[1], first[0][1, :50]) and torch.equal(i[1], first[1][1, :50])
    assert float(ff.loglik[1]) == float(lk1[1])
    o = bf.state_offsets
    for b_ in (0, 2, 3):
        assert torch.equal(ff.state[int(o[b_]) : int(o[b_ + 1])], state_before[int(o[b_]) : int(o[b_ + 1])])
        assert (f[b_] == 0).all() and (i[b_] == 0).all() and float(ff.loglik[b_]) == float(lk_before[b_])


SHIFTS = (100.0, -150.0)


def case_config3(wl, sharp):
    """config 3's graph, B = 4, N = 300: randn emissions, or (sharp) log_softmax(10 randn).  (Module-level: the floor tool
    tools/measure_filter_floor.py runs the reference's float32 mode on the very same inputs and their shifted copies.)"""
    g = wl.lfmmi_denominator()
    B, N = 4, 300
    x = np.random.default_rng(3).standard_normal((B, N, g.P))
    V = (_log_softmax(10.0 * x) if sharp else x).astype(np.float32)
    return [g] * B, V, np.array([300, 263, 226, 189], dtype=np.int32)


def shifted(V, shift):
    return (V + np.float32(shift)).astype(np.float32)


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph_and_the_level_of_v(mm, wl, torch, sharp):
    gs, V, lens = case_config3(wl, sharp)
    N = V.shape[1]
    refs = _refs(gs, V, lens)
    bf = _batch(mm, wl, gs)
    out = _run(bf, V, lens)
    assert np.isfinite(out[2]).all()
    _check(bf, out, refs, lens, f"config 3 graph, sharp = {sharp}")
    for shift in SHIFTS:
        Vs = shifted(V, shift)
        outs = _run(bf, Vs, lens)
        # filt against the UNSHIFTED reference, incr moved by the constant
        refs_s = [(r[0], r[1] + shift * (np.arange(N) < L), r[2] + shift * L, r[3]) for r, L in zip(refs, lens)]
        _check(bf, outs, refs_s, lens, f"config 3 graph, sharp = {sharp}, V {shift:+g}")


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, torch, name):
    g = wl.load_npz_graph(os.path.join(HERE, "golden", name + ".npz"))
    B, N = 3, 200
    V = np.random.default_rng(11).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([200, 171, 130], dtype=np.int32)
    bf = _batch(mm, wl, [g] * B)
    out = _run(bf, V, lens)
    # (the numerator graph has no accepting path of 130 frames: utterance 2 is alive in every frame -- filt, incr and the real
    # entries of state_out are finite -- while the final weights accept none of its mass: state_out(final) = ttl = -inf)
    assert (np.isfinite(out[2]) == ([True] * 3 if name.startswith("den") else [True, True, False])).all(), out[2]
    assert np.isfinite(out[1]).all() and np.allclose(out[0].sum(-1), np.arange(N)[None] < lens[:, None], atol=1e-5)
    _check(bf, out, _refs([g] * B, V, lens), lens, name)


def test_vectors_in_global_memory(mm, wl, torch):
    """12 500 states (the size of the item-form tests).  This entry keeps two vectors where the item kernel keeps four, so its own
    plan still has them in LDS at that size: the <8,global> instance runs there by MM_BIGV, and by its own plan from 20 000 states
    on (2 x 4 x 20 000 bytes = the 160 KB of a compute unit)."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    N = 40
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([40, 29], dtype=np.int32)
    refs = _refs([g, g], V, lens)
    bf = _with_env({"MM_DEBUG": "1", "MM_BIGV": "1"}, lambda: _batch(mm, wl, [g, g]))
    assert "mm_filter_kernel<8,global>" in bf.kernels("filter"), bf.kernels("filter")
    _check(bf, _run(bf, V, lens), refs, lens, "12500 states, vectors in global memory")
    bf = _batch(mm, wl, [g, g])
    assert "mm_filter_kernel<8,lds>" in bf.kernels("filter") and "global" in bf.kernels("arcs"), bf.kernels("filter")
    _check(bf, _run(bf, V, lens), refs, lens, "12500 states, vectors in LDS")
    g = wl.random_fsm(20600, 40, 3.0, seed=3)
    N = 12
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([12, 7], dtype=np.int32)
    bf = _batch(mm, wl, [g, g])
    assert "mm_filter_kernel<8,global>" in bf.kernels("filter"), bf.kernels("filter")
    _check(bf, _run(bf, V, lens), _refs([g, g], V, lens), lens, "20600 states")


def test_streamed_instance(mm, wl, torch):
    gs, V, lens = case_random40(wl)
    bf = _with_env(STREAMED, lambda: _batch(mm, wl, gs))
    assert "mm_filter_kernel<0,global>" in bf.kernels("filter"), bf.kernels("filter")
    _check(bf, _run(bf, V, lens), _refs(gs, V, lens), lens, "streamed instance")


def test_lds_plan_is_no_larger_than_the_item_kernels(mm, wl, torch):
    """The entry's LDS plan is the export modes' (two vectors, no stage rows): wherever the item kernel keeps its vectors in LDS,
    so does this entry -- there is no graph between two plans to test."""
    g = wl.random_fsm(9000, 40, 3.0, seed=5)
    bf = _batch(mm, wl, [g, g])
    assert "global" not in bf.kernels("export") and "mm_filter_kernel<8,lds>" in bf.kernels("filter"), bf.kernels("filter")
    N = 20
    V = np.random.default_rng(12).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([20, 13], dtype=np.int32)
    _check(bf, _run(bf, V, lens), _refs([g, g], V, lens), lens, "9000 states")


def test_agrees_with_pdfposteriors(mm, wl, torch):
    gs, V, lens = case_random40(wl)
    bf = _batch(mm, wl, gs)
    filt, incr, ttl = bf.filterposteriors(V, lens)
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    ok = np.isfinite(t_pdf)
    assert (np.isfinite(ttl) == ok).all() and np.allclose(ttl[ok], t_pdf[ok], rtol=1e-5, atol=1e-4), (ttl, t_pdf)
    # final weights equal on every real state: filt of the last frame is the smoothing posterior
    g = gs[0]
    gu = dataclasses.replace(g, name=g.name + "_uf", final_idx=np.arange(g.S), final_w=np.full(g.S, -1.25))
    bu = _batch(mm, wl, [gu] * 6)
    filt, incr, ttl = bu.filterposteriors(V, lens)
    g_pdf, t_pdf = bu.pdfposteriors(V, lens)
    assert np.allclose(ttl[ok], t_pdf[ok], rtol=1e-5, atol=1e-4)
    for b in np.flatnonzero(ok):
        L = int(lens[b])
        check_gamma(filt[b, L - 1][None, None], g_pdf[b, L - 1].astype(np.float64)[None, None], [1])
    assert np.abs(filt[0, :29] - g_pdf[0, :29]).max() > 1e-3


def _property_inputs(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    bf = _batch(mm, wl, [g] * 6)
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    return g, bf, V, lens


def test_capture_before_a_first_call_is_refused(mm, wl, torch):
    """The item forms are never put on the device during a capture.  (A batch of the wave kernel is created without them.)"""
    g = wl.lexicon_fsm(300, 20, seed=2, hubs=1)
    fresh = _batch(mm, wl, [g] * 5)
    assert "mm_wave_kernel" in fresh.kernels("log"), fresh.kernels("log")
    N = 40
    V = torch.from_numpy(np.random.default_rng(9).standard_normal((5, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([40, 31, 40, 12, 25], dtype=torch.int32, device="cuda")
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.filterposteriors(V, lens)
    assert ei.value.code == -1 and "not on the device yet" in str(ei.value)
    # ... and the batch works afterwards
    out = _run(fresh, V, lens)
    torch.cuda.synchronize()
    Vn, ln = V.cpu().numpy(), lens.cpu().numpy()
    _check(fresh, [t.cpu().numpy() for t in out], _refs([g] * 5, Vn, ln), ln, "wave-kernel batch")


def test_bit_identical_likelihood_only_and_graph_capture(mm, wl, torch):
    g, bf, V, lens = _property_inputs(mm, wl, torch)
    out0 = _run(bf, V, lens)
    out1 = _run(bf, V, lens)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    # filt = NULL: the same incr, ttl and state_out bits
    lik = _run(bf, V, lens, want_filt=False)
    torch.cuda.synchronize()
    assert lik[0] is None and all(torch.equal(x, y) for x, y in zip(out0[1:], lik[1:]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = _run(bf, V, lens)
    for _ in range(2):
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out0, out2))
    gs = [g] * 6
    Vn, ln = V.cpu().numpy(), lens.cpu().numpy()
    _check(bf, [t.cpu().numpy() for t in out0], _refs(gs, Vn, ln), ln, "property inputs")


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    filt = torch.zeros((B, N, P), device="cuda")
    incr = torch.zeros((B, N), device="cuda")
    ttl = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, filt_ptr=filt.data_ptr(), fsn=P, incr_ptr=incr.data_ptr(), isb=N, ttl_ptr=ttl.data_ptr()):
        return lib.mm_filterposteriors_f32(h, V.data_ptr(), N * P, P, None, N, None, None, filt_ptr, N * P, fsn, 1, incr_ptr, isb, ttl_ptr, st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(tb._h) == -4
    assert b"log" in lib.mm_last_error()
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h) == -4
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h, filt_ptr=None, incr_ptr=None, ttl_ptr=None) == -1
    assert call(lb._h, fsn=P - 1) == -2
    assert call(lb._h, isb=N - 1) == -2
    assert call(lb._h) == 0 and call(lb._h, filt_ptr=None, incr_ptr=None) == 0
    torch.cuda.synchronize()
    assert "mm_filter_kernel<8,lds>" in lb.kernels("filter")
    for b in (tb, pb):
        with pytest.raises(mm.MarkovModelsAMDError):
            b.kernels("filter")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.filterposteriors(V, None)


def test_column_major_output_strides(mm, wl, torch):
    """The reference's B x P x N column-major layout: f_stride_b = 1, f_stride_p = B, f_stride_n = B * P."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 50, g.P
    bf = _batch(mm, wl, [g] * B)
    V = torch.from_numpy(np.random.default_rng(8).standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([50, 41, 50, 13], dtype=torch.int32, device="cuda")
    filt0, incr0, ttl0 = bf.filterposteriors(V, lens)
    filt = torch.full((N, P, B), 7.0, device="cuda")   # element (b, n, p) at b + p * B + n * B * P
    incr = torch.full((B, N + 3), 7.0, device="cuda")  # rows of N + 3: the three elements behind a row are not touched
    ttl = torch.empty(B, device="cuda")
    rc = lib.mm_filterposteriors_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, None, None, filt.data_ptr(), 1, B * P, B,
                                     incr.data_ptr(), N + 3, ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(filt.permute(2, 0, 1), filt0) and torch.equal(ttl, ttl0)
    assert torch.equal(incr[:, :N], incr0) and (incr[:, N:] == 7.0).all()
    # the module-level call in pdfposteriors' shape: filt [B, P, N] from expanded V_hats
    Vn, ln = V.cpu().numpy(), lens.cpu().numpy()
    Vh = [mm.expand(Vn[b].T, int(ln[b])) for b in range(B)]
    f_mod, i_mod, t_mod = mm.filterposteriors(bf, Vh)
    assert f_mod.shape == (B, P, N) and np.array_equal(f_mod, filt0.cpu().numpy().transpose(0, 2, 1))
    assert np.array_equal(i_mod, incr0.cpu().numpy()) and np.array_equal(t_mod, ttl0.cpu().numpy())
    f_dev, i_dev, t_dev = mm.filterposteriors(bf, torch.from_numpy(np.stack(Vh)).cuda(), seqlengths=ln)
    assert torch.equal(f_dev, filt0.transpose(1, 2)) and torch.equal(i_dev, incr0) and torch.equal(t_dev, ttl0)
