"""Leaky-HMM pdf posteriors (mm_leakyposteriors_f32) on the MI355X against the float64 reference of tests/leaky_reference.py, and
the properties of the entry: the no-path conventions, agreement with pdfposteriors at a zero leak, the restart case, bit-identical
repeats, hipGraph capture, error codes, output strides, the LF-MMI loss with a leaky denominator.

The bars are the project's own: gamma has check_gamma of tests/test_gpu_parity.py (2e-5 absolute, 1e-4 relative on log gamma where
gamma_ref > 1e-30, exact zeros beyond the length, rows summing to 1 within 1e-5), ttl np.allclose(rtol=1e-5, atol=1e-4) as the arc
tests use."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import leaky_reference as lr
from test_gpu_parity import _with_env, check_gamma
from test_leakyposteriors import restart_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


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


def _check(gamma, ttl, gs, V, lens, eps, idx=None):
    """Every utterance of `idx` (None: all) against the float64 reference; returns the worst log-posterior error over its bar."""
    N = V.shape[1]
    worst = 0.0
    for b in (range(len(gs)) if idx is None else idx):
        L = int(lens[b])
        g_ref, z_ref = lr.reference(gs[b], V[b].astype(np.float64), L, N, eps)
        if not np.isfinite(z_ref):
            assert np.isneginf(ttl[b]) and (gamma[b] == 0).all(), (b, ttl[b])
            print(f"utterance {b}: len {L}, no path: gamma = 0, ttl = -inf")
            continue
        assert np.allclose(ttl[b], z_ref, rtol=1e-5, atol=1e-4), (b, ttl[b], z_ref)
        e = check_gamma(gamma[b][None], g_ref[None], [L])
        print(f"utterance {b}: len {L}, ttl {ttl[b]:.6f} (ref {z_ref:.6f}), worst log-posterior error over its bar {e:.3g}")
        worst = max(worst, e)
    return worst


def case_random40(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((5, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf   # a frame with -inf entries
    V[4, 4, :] = -np.inf    # no path, leak or not
    return [g] * 5, V, lens


@pytest.mark.parametrize("eps", [1e-5, 0.1])
def test_random_graph_lengths_and_no_path(mm, wl, torch, eps):
    gs, V, lens = case_random40(wl)
    bf = _batch(mm, wl, gs)
    gamma, ttl = bf.leakyposteriors(V, lens, leak=eps)
    _check(gamma, ttl, gs, V, lens, eps)
    for b in (3, 4):  # len = 0; a frame whose emissions are all -inf
        assert np.isneginf(ttl[b]) and (gamma[b] == 0).all()
    assert np.isfinite(ttl[[0, 1, 2]]).all()


def test_streamed_instance(mm, wl, torch):
    """No item in registers (MM_NITEMS=0): every item streamed, the vectors in global memory -- the instance FSMs of more than 65534
    states run, on the graph of test_random_graph_lengths_and_no_path and with its bars."""
    gs, V, lens = case_random40(wl)
    bf = _with_env({"MM_DEBUG": "1", "MM_NITEMS": "0"}, lambda: _batch(mm, wl, gs))
    k = bf.kernels("leaky")
    assert "mm_leaky_fwd_kernel<0,global>" in k and "mm_leaky_bwd_kernel<0,global>" in k, k
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.1)
    _check(gamma, ttl, gs, V, lens, 0.1)
    for b in (3, 4):  # len = 0; a frame whose emissions are all -inf
        assert np.isneginf(ttl[b]) and (gamma[b] == 0).all()
    assert np.isfinite(ttl[[0, 1, 2]]).all()


def test_zero_leak_agrees_with_pdfposteriors(mm, wl, torch):
    gs, V, lens = case_random40(wl)
    bf = _batch(mm, wl, gs)
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.0)
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    ok = np.isfinite(t_pdf)
    assert (np.isfinite(ttl) == ok).all()
    assert np.allclose(ttl[ok], t_pdf[ok], rtol=1e-5, atol=1e-4)
    check_gamma(gamma[ok], g_pdf[ok].astype(np.float64), lens[ok])
    assert (gamma[~ok] == 0).all() and (g_pdf[~ok] == 0).all()
    _check(gamma, ttl, gs, V, lens, 0.0)
    # a larger graph, the kernels mm_pdfposteriors_f32 picks for it being others than the item kernel
    g = wl.lfmmi_denominator(600, 40, seed=5)
    bf = _batch(mm, wl, [g] * 4)
    lens = np.array([150, 120, 150, 33], dtype=np.int32)
    V = np.random.default_rng(1).standard_normal((4, 150, g.P)).astype(np.float32)
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.0)
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    assert np.isfinite(ttl).all() and np.allclose(ttl, t_pdf, rtol=1e-5, atol=1e-4)
    check_gamma(gamma, g_pdf.astype(np.float64), lens)


def test_restart_case(mm, wl, torch):
    g, V = restart_case(wl)
    V = V.astype(np.float32)[None]
    lens = np.array([5], dtype=np.int32)
    bf = _batch(mm, wl, [g])
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    assert np.isneginf(t_pdf[0]) and (g_pdf == 0).all()
    gamma, ttl = bf.leakyposteriors(V, lens, leak=1e-5)
    assert np.isfinite(ttl[0]) and abs(float(ttl[0]) - (-14.97864)) <= 1e-4 + 1e-5 * 14.97864
    _check(gamma, ttl, [g], V, lens, 1e-5)


@pytest.mark.parametrize("shift", [100.0, -150.0])
def test_a_constant_added_to_v_changes_no_posterior(mm, wl, torch, shift):
    """pdfposteriors does not depend on the level of V, and neither may the leak: emissions near +100 nats (2^(v + 32) of an
    un-normalised value would overflow) and near -150 nats (it would flush to zero and the leak would be dropped without a word)."""
    gs, V, lens = case_random40(wl)
    bf = _batch(mm, wl, gs)
    Vs = (V + np.float32(shift)).astype(np.float32)
    for eps in (1e-5, 0.1):
        g0, t0 = bf.leakyposteriors(V, lens, leak=eps)
        g1, t1 = bf.leakyposteriors(Vs, lens, leak=eps)
        assert np.isfinite(g1).all() and (np.isfinite(t1) == np.isfinite(t0)).all()
        _check(g1, t1, gs, Vs, lens, eps)
        ok = np.isfinite(t0)
        check_gamma(g1[ok], g0[ok].astype(np.float64), lens[ok])
    # the restart case lives on the leak alone: dropped, its log Z would be -inf
    g, Vr = restart_case(wl)
    Vr = (Vr + shift).astype(np.float32)[None]
    gamma, ttl = _batch(mm, wl, [g]).leakyposteriors(Vr, np.array([5], dtype=np.int32), leak=1e-5)
    assert np.isclose(ttl[0], -14.97864 + 5 * shift, rtol=1e-5, atol=1e-4), ttl
    _check(gamma, ttl, [g], Vr, np.array([5], dtype=np.int32), 1e-5)
    # ... and a zero leak stays pdfposteriors at that level
    g0, t0 = bf.leakyposteriors(Vs, lens, leak=0.0)
    _check(g0, t0, gs, Vs, lens, 0.0)


def test_graph_between_the_two_lds_plans(mm, wl, torch):
    """9000 states: the item kernel's vectors fit the LDS, this entry's (one row of constants more) do not -- the batch gets its
    global vectors with the entry's first call."""
    g = wl.random_fsm(9000, 40, 3.0, seed=5)
    N = 30
    V = np.random.default_rng(12).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([30, 21], dtype=np.int32)
    bf = _batch(mm, wl, [g, g])
    assert "<8,global>" in bf.kernels("leaky") and "global" not in bf.kernels("export"), (bf.kernels("leaky"), bf.kernels("export"))
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.1)
    _check(gamma, ttl, [g, g], V, lens, 0.1)


def case_config3(wl, sharp):
    g = wl.lfmmi_denominator()
    B, N = (8, 1500) if not sharp else (4, 500)
    x = np.random.default_rng(3).standard_normal((B, N, g.P))
    V = (_log_softmax(10.0 * x) if sharp else x).astype(np.float32)
    lens = np.array([N] + [N - 37 * k for k in range(1, B)], dtype=np.int32)
    return [g] * B, V, lens, [0, 1, B - 1]


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph(mm, wl, torch, sharp):
    gs, V, lens, idx = case_config3(wl, sharp)
    bf = _batch(mm, wl, gs)
    gamma, ttl = bf.leakyposteriors(V, lens, leak=1e-5)
    assert np.isfinite(ttl).all()
    worst = _check(gamma, ttl, gs, V, lens, 1e-5, idx)
    print(f"config 3 graph, sharp = {sharp}: worst log-posterior error over its bar {worst:.3g}")


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, torch, name):
    g = wl.load_npz_graph(os.path.join(HERE, "golden", name + ".npz"))
    B, N = 3, 700
    V = np.random.default_rng(11).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([N, 611, 430], dtype=np.int32) if name.startswith("den") else np.array([N, 650, 500], dtype=np.int32)
    bf = _batch(mm, wl, [g] * B)
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.1)
    assert np.isfinite(ttl).all()
    worst = _check(gamma, ttl, [g] * B, V, lens, 0.1)
    print(f"{name}: worst log-posterior error over its bar {worst:.3g}")


def test_distinct_graphs(mm, wl, torch):
    """Four graphs in one batch, each with its own initial distribution (its own pi and rho)."""
    gs = [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    bf = _batch(mm, wl, gs)
    for eps in (1e-5, 0.1):
        gamma, ttl = bf.leakyposteriors(V, lens, leak=eps)
        assert np.isfinite(ttl).all()
        _check(gamma, ttl, gs, V, lens, eps)


def test_graph_beyond_the_lds(mm, wl, torch):
    """12 500 states (the size of the item-form tests): the state vectors do not fit the LDS."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    N = 40
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([40, 29], dtype=np.int32)
    bf = _batch(mm, wl, [g, g])
    k = bf.kernels("leaky")
    assert "mm_leaky_fwd_kernel<8,global>" in k and "mm_leaky_bwd_kernel<8,global>" in k, k
    gamma, ttl = bf.leakyposteriors(V, lens, leak=0.1)
    _check(gamma, ttl, [g, g], V, lens, 0.1)


def _property_inputs(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    bf = _batch(mm, wl, [g] * 6)
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    return g, bf, V, lens


def test_capture_before_a_first_call_is_refused(mm, wl, torch):
    """The item forms and the leak rows are never put on the device during a capture."""
    g, fresh, V, lens = _property_inputs(mm, wl, torch)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.leakyposteriors(V, lens, leak=1e-5)
    assert ei.value.code == -1 and "not on the device yet" in str(ei.value)
    # ... and the batch works afterwards
    out = fresh.leakyposteriors(V, lens, leak=1e-5)
    torch.cuda.synchronize()
    assert torch.isfinite(out[1]).all()


def test_bit_identical_and_graph_capture(mm, wl, torch):
    g, bf, V, lens = _property_inputs(mm, wl, torch)
    out0 = bf.leakyposteriors(V, lens, leak=1e-5)
    out1 = bf.leakyposteriors(V, lens, leak=1e-5)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = bf.leakyposteriors(V, lens, leak=1e-5)
    for _ in range(2):
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out0, out2))
    gs = [g] * 6
    _check(out0[0].cpu().numpy(), out0[1].cpu().numpy(), gs, V.cpu().numpy(), lens.cpu().numpy(), 1e-5, [0, 4])


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    gamma = torch.zeros((B, N, P), device="cuda")
    ttl = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, leak, gamma_ptr=gamma.data_ptr(), gsn=P):
        return lib.mm_leakyposteriors_f32(h, V.data_ptr(), N * P, P, None, N, C.c_float(leak), gamma_ptr, N * P, gsn, 1, ttl.data_ptr(), st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(tb._h, 0.1) == -4
    assert b"log" in lib.mm_last_error()
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h, 0.1) == -4
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(lb._h, bad) == -1, bad
    assert call(lb._h, 0.1, gamma_ptr=None) == -1
    assert call(lb._h, 0.1, gsn=P - 1) == -2
    assert call(lb._h, 0.0) == 0 and call(lb._h, 0.1) == 0
    torch.cuda.synchronize()
    assert "mm_leaky_fwd_kernel" in lb.kernels("leaky") and "mm_leaky_bwd_kernel" in lb.kernels("leaky")
    for b in (tb, pb):
        with pytest.raises(mm.MarkovModelsAMDError):
            b.kernels("leaky")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.leakyposteriors(V, None, leak=0.1)


def test_column_major_output_strides(mm, wl, torch):
    """The reference's B x P x N column-major layout: g_stride_b = 1, g_stride_p = B, g_stride_n = B * P."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 50, g.P
    bf = _batch(mm, wl, [g] * B)
    V = torch.from_numpy(np.random.default_rng(8).standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([50, 41, 50, 13], dtype=torch.int32, device="cuda")
    gamma0, ttl0 = bf.leakyposteriors(V, lens, leak=0.1)
    gamma = torch.full((N, P, B), 7.0, device="cuda")   # element (b, n, p) at b + p * B + n * B * P
    ttl = torch.empty(B, device="cuda")
    rc = lib.mm_leakyposteriors_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, C.c_float(0.1), gamma.data_ptr(), 1, B * P, B,
                                    ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gamma.permute(2, 0, 1), gamma0) and torch.equal(ttl, ttl0)
    # the module-level call in pdfposteriors' shape: gamma [B, P, N] from expanded V_hats
    Vn, ln = V.cpu().numpy(), lens.cpu().numpy()
    Vh = [mm.expand(Vn[b].T, int(ln[b])) for b in range(B)]
    g_mod, t_mod = mm.leakyposteriors(bf, Vh, leak=0.1)
    assert g_mod.shape == (B, P, N) and np.array_equal(g_mod, gamma0.cpu().numpy().transpose(0, 2, 1)) and np.array_equal(t_mod, ttl0.cpu().numpy())
    g_dev, t_dev = mm.leakyposteriors(bf, torch.from_numpy(np.stack(Vh)).cuda(), leak=0.1, seqlengths=ln)
    assert torch.equal(g_dev, gamma0.transpose(1, 2)) and torch.equal(t_dev, ttl0)


def test_lfmmi_loss_with_a_leaky_denominator(mm, wl, torch):
    """loss = -(ttl_num - ttl_den_leaky), V.grad = gamma_den_leaky - gamma_num, from the references; leak=None is today's path."""
    P, N = 6, 15
    den = wl.random_fsm(30, P, 3.0, seed=21)
    nums = [wl.random_fsm(S, P, 2.0, seed=30 + S) for S in (8, 11, 9)]
    lens = np.array([15, 12, 9], dtype=np.int32)
    V = np.random.default_rng(7).standard_normal((3, N, P)).astype(np.float32)
    cden = mm.compile(wl.to_fsm(mm, den), mm.statemap(den.state2pdf, P))
    bden = mm.batch(cden, cden, cden)
    bnum = mm.batch(*[mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, P)) for g in nums])
    lt = torch.from_numpy(lens).cuda()
    l_ref, g_ref = 0.0, np.zeros((3, N, P))
    for b in range(3):
        gd, zd = lr.reference(den, V[b].astype(np.float64), int(lens[b]), N, 0.1)
        gn, zn = lr.reference(nums[b], V[b].astype(np.float64), int(lens[b]), N, 0.0)
        l_ref -= zn - zd
        g_ref[b] = gd - gn
    for mode in ("auto", "serial", "concurrent"):
        Vt = torch.from_numpy(V).cuda().requires_grad_(True)
        loss, tn, td = mm.lfmmi_loss(Vt, bnum, bden, lt, mode=mode, leak=0.1)
        loss.backward()
        assert np.isclose(float(loss.detach()), l_ref, rtol=1e-5, atol=1e-4), (mode, float(loss.detach()), l_ref)
        assert np.allclose(Vt.grad.cpu().numpy(), g_ref, atol=2e-5), (mode, np.abs(Vt.grad.cpu().numpy() - g_ref).max())
    # leak=None: the same bits as the call without the argument
    outs = []
    for kw in ({}, {"leak": None}):
        Vt = torch.from_numpy(V).cuda().requires_grad_(True)
        loss, tn, td = mm.lfmmi_loss(Vt, bnum, bden, lt, **kw)
        loss.backward()
        outs.append((loss.detach(), tn, td, Vt.grad))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*outs))
