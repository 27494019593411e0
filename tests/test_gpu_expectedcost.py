"""Expected path cost and its gradient (mm_expectedcost_f32) on the MI355X against the float64 reference of
tests/cost_reference.py, and the properties of the entry: the identities of the definition on the device's own outputs, costs
beyond the length never read, output strides, bit-identical repeats, hipGraph capture, error codes, the autograd functions.

The input builders (`case_*`) are module-level so that tools/measure_cost_floor.py can run the reference's float32 mode on the
very same inputs: the absolute part of the gradient's bar (cost_reference.GRAD_ABS_A) comes from there, not from the kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import cost_reference as cr
from test_gpu_parity import check_gamma

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
    fs, cache = [], {}
    for g in gs:
        if id(g) not in cache:
            f = wl.to_fsm(mm, g)
            cache[id(g)] = (f, mm.compile(f, mm.statemap(g.state2pdf, g.P)))
        fs.append(cache[id(g)][0])
    return fs, mm.batch(*[cache[id(g)][1] for g in gs])


def _log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def _smbr_cost(wl, g, B, N, seed):
    """-onehot of the pdfs along a path of the graph: the sMBR cost of a reference alignment."""
    pdf = np.asarray(g.state2pdf)[wl.sample_paths(g, B, N, seed)]
    cost = np.zeros((B, N, g.P), dtype=np.float32)
    np.put_along_axis(cost, pdf[:, :, None], -1.0, 2)
    return cost, pdf


# ---- the inputs: (graphs, V, cost, lens, utterances checked against the reference)
def case_random40(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((5, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf   # a frame with -inf entries
    V[4, 4, :] = -np.inf    # no accepting path
    cost = np.random.default_rng(10).standard_normal((5, N, g.P)).astype(np.float32)
    return [g] * 5, V, cost, lens, None


def case_config3(wl, sharp):
    g = wl.lfmmi_denominator()
    B, N = (8, 1500) if not sharp else (4, 500)
    x = np.random.default_rng(3).standard_normal((B, N, g.P))
    V = (_log_softmax(10.0 * x) if sharp else x).astype(np.float32)
    lens = np.array([N] + [N - 37 * k for k in range(1, B)], dtype=np.int32)
    cost, _ = _smbr_cost(wl, g, B, N, seed=13)
    return [g] * B, V, cost, lens, [0, 1, B - 1]


def case_wsj(wl, name):
    g = wl.load_npz_graph(os.path.join(HERE, "golden", name + ".npz"))
    B, N = 3, 700
    V = np.random.default_rng(11).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([N, 611, 430], dtype=np.int32) if name.startswith("den") else np.array([N, 650, 500], dtype=np.int32)
    cost = np.random.default_rng(17).standard_normal((B, N, g.P)).astype(np.float32)
    return [g] * B, V, cost, lens, None


def case_distinct(wl):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    cost = np.random.default_rng(15).standard_normal((len(gs), N, 5)).astype(np.float32)
    return gs, V, cost, np.array([40, 33, 20, 38], dtype=np.int32), None


def case_bigv(wl):
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    N = 40
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    cost = np.random.default_rng(14).standard_normal((2, N, g.P)).astype(np.float32)
    return [g, g], V, cost, np.array([40, 29], dtype=np.int32), None


def _check_batch(mm, wl, oracle, case):
    o, oc = oracle
    gs, V, cost, lens, check_idx = case
    fs, bf = _batch(mm, wl, gs)
    N = V.shape[1]
    risk, grad, ttl, gamma = bf.expectedcost(V, cost, lens, want_gamma=True)
    for b in (range(len(gs)) if check_idx is None else check_idx):
        L = int(lens[b])
        ref = cr.reference(o, oc, gs[b], fs[b], V[b].astype(np.float64), cost[b].astype(np.float64), L, N)
        rr, ge = cr.check(risk[b], grad[b], ttl[b], ref, cost[b], L)
        print(f"utterance {b}: len {L}, risk {risk[b]:.6g} (ref {ref[0]:.6g}, error / bar {rr:.3g}), max |grad error| / G {ge:.3g} "
              f"(a = {cr.GRAD_ABS_A:.3g})")
        if np.isfinite(ref[3]):
            check_gamma(gamma[b][None], ref[2][None], [L])
        else:
            assert (gamma[b] == 0).all()
    return bf, risk, grad, ttl, gamma


def test_random_graph_lengths_and_no_path(mm, wl, oracle, torch):
    case = case_random40(wl)
    bf, risk, grad, ttl, gamma = _check_batch(mm, wl, oracle, case)
    for b in (3, 4):
        assert np.isneginf(ttl[b]) and risk[b] == 0 and (grad[b] == 0).all() and (gamma[b] == 0).all()
    # ttl is pdfposteriors' log Z
    _, t2 = bf.pdfposteriors(case[1], case[3])
    ok = np.isfinite(t2)
    assert np.allclose(ttl[ok], t2[ok], rtol=1e-5, atol=1e-4) and (np.isfinite(ttl) == ok).all()


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph_smbr_cost(mm, wl, oracle, torch, sharp):
    _check_batch(mm, wl, oracle, case_config3(wl, sharp))


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, oracle, torch, name):
    _check_batch(mm, wl, oracle, case_wsj(wl, name))


def test_distinct_graphs(mm, wl, oracle, torch):
    _check_batch(mm, wl, oracle, case_distinct(wl))


def test_bigv_graph(mm, wl, oracle, torch):
    case = case_bigv(wl)
    _, bf = _batch(mm, wl, case[0])
    k = bf.kernels("cost")
    assert "mm_cost_fwd_kernel<8,global>" in k and "mm_cost_bwd_kernel<8,global>" in k
    _check_batch(mm, wl, oracle, case)


def test_identities_on_the_device_outputs(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    _, bf = _batch(mm, wl, [g] * 6)
    N = 200
    rng = np.random.default_rng(6)
    V = rng.standard_normal((6, N, g.P)).astype(np.float32)
    cost = rng.standard_normal((6, N, g.P)).astype(np.float32)
    lens = np.array([200, 180, 90, 200, 7, 64], dtype=np.int32)
    risk, grad, ttl, gamma = bf.expectedcost(V, cost, lens, want_gamma=True)
    assert np.isfinite(risk).all() and np.isfinite(grad).all() and np.isfinite(ttl).all()
    g_pdf, t_pdf = bf.pdfposteriors(V, lens)
    check_gamma(gamma, g_pdf.astype(np.float64), lens)
    assert np.allclose(ttl, t_pdf, rtol=1e-5, atol=1e-4)
    a = cr.GRAD_ABS_A
    for b, L in enumerate(lens):
        c = cost[b, :L].astype(np.float64)
        G = np.abs(grad[b]).max()
        # sum_p grad = 0: P terms, each within the gradient's bar (its relative part on |grad|, its absolute part on G)
        s = np.abs(grad[b].astype(np.float64).sum(axis=1))
        assert (s <= 1e-4 * np.abs(grad[b]).sum(axis=1) + g.P * a * G).all(), (b, s.max(), G)
        # risk = sum gamma cost, the risk's own bar (twice: both sides are the device's)
        dot = float(np.sum(gamma[b, :L].astype(np.float64) * c))
        bar = 1e-4 * float(np.sum(gamma[b, :L] * np.abs(c))) + 1e-6 * L * float(np.abs(c).max())
        assert abs(float(risk[b]) - dot) <= 2 * bar, (b, risk[b], dot, bar)
    # a cost that does not depend on the pdf: risk = sum c_n, grad = 0 (the bar's scale is the cost's: the reference's gradient is 0)
    cn = rng.standard_normal((6, N)).astype(np.float32)
    flat = np.repeat(cn[:, :, None], g.P, axis=2)
    risk, grad, ttl = bf.expectedcost(V, flat, lens)
    for b, L in enumerate(lens):
        tot = float(cn[b, :L].astype(np.float64).sum())
        assert abs(float(risk[b]) - tot) <= 1e-4 * float(np.abs(cn[b, :L]).sum()) + 1e-6 * L * float(np.abs(cn[b, :L]).max()), (b, risk[b], tot)
        assert np.abs(grad[b]).max() <= a * float(np.abs(cn[b, :L]).max()), (b, np.abs(grad[b]).max())


def test_costs_beyond_the_length_are_not_read(mm, wl, torch):
    gs, V, cost, lens, _ = case_random40(wl)
    _, bf = _batch(mm, wl, gs)
    clean = bf.expectedcost(V, cost, lens, want_gamma=True)
    dirty = cost.copy()
    for b, L in enumerate(lens):
        dirty[b, L:] = np.nan
    out = bf.expectedcost(V, dirty, lens, want_gamma=True)
    for x, y in zip(clean, out):
        assert x.tobytes() == y.tobytes()


def test_column_major_output_strides(mm, wl, torch):
    """The reference's B x P x N column-major layout: g_stride_b = 1, g_stride_p = B, g_stride_n = B * P."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 50, g.P
    _, bf = _batch(mm, wl, [g] * B)
    rng = np.random.default_rng(8)
    V = torch.from_numpy(rng.standard_normal((B, N, P)).astype(np.float32)).cuda()
    cost = torch.from_numpy(rng.standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([50, 41, 50, 13], dtype=torch.int32, device="cuda")
    risk0, grad0, ttl0, gamma0 = bf.expectedcost(V, cost, lens, want_gamma=True)
    grad = torch.full((N, P, B), 7.0, device="cuda")   # element (b, n, p) at b + p * B + n * B * P
    gamma = torch.full((N, P, B), 7.0, device="cuda")
    risk, ttl = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    rc = lib.mm_expectedcost_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, cost.data_ptr(), N * P, P, risk.data_ptr(),
                                 grad.data_ptr(), gamma.data_ptr(), 1, B * P, B, ttl.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(grad.permute(2, 0, 1), grad0) and torch.equal(gamma.permute(2, 0, 1), gamma0)
    assert torch.equal(risk, risk0) and torch.equal(ttl, ttl0)


def test_bit_identical_and_graph_capture(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    _, bf = _batch(mm, wl, [g] * 6)
    N = 120
    rng = np.random.default_rng(6)
    V = torch.from_numpy(rng.standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    cost = torch.from_numpy(rng.standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    out0 = bf.expectedcost(V, cost, lens, want_gamma=True)
    out1 = bf.expectedcost(V, cost, lens, want_gamma=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = bf.expectedcost(V, cost, lens, want_gamma=True)
    for _ in range(2):
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out0, out2))


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    cost = torch.zeros((B, N, P), device="cuda")
    grad = torch.zeros((B, N, P), device="cuda")
    risk = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, grad_ptr, gsn, csn=P):
        return lib.mm_expectedcost_f32(h, V.data_ptr(), N * P, P, None, N, cost.data_ptr(), N * P, csn, risk.data_ptr(), grad_ptr, None,
                                       N * P, gsn, 1, None, st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(tb._h, grad.data_ptr(), P) == -4
    assert b"log" in lib.mm_last_error()
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h, None, P) == -1
    assert call(lb._h, grad.data_ptr(), P - 1) == -2
    assert call(lb._h, grad.data_ptr(), P, csn=P - 1) == -2
    assert call(lb._h, grad.data_ptr(), P) == 0
    torch.cuda.synchronize()
    assert "mm_cost_fwd_kernel" in lb.kernels("cost") and "mm_cost_bwd_kernel" in lb.kernels("cost")
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("cost")


def test_autograd_expected_cost(mm, wl, torch):
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 3, 60, g.P
    _, bf = _batch(mm, wl, [g] * B)
    rng = np.random.default_rng(9)
    V = torch.from_numpy(rng.standard_normal((B, N, P)).astype(np.float32)).cuda().requires_grad_(True)
    cost = torch.from_numpy(rng.standard_normal((B, N, P)).astype(np.float32)).cuda().requires_grad_(True)
    lens = torch.tensor([60, 44, 31], dtype=torch.int32, device="cuda")
    risk0, grad0, ttl0, gamma0 = bf.expectedcost(V.detach(), cost.detach(), lens, want_gamma=True)
    loss, risk, ttl = mm.expected_cost(V, cost, bf, lens)
    assert torch.equal(risk, risk0) and torch.equal(ttl, ttl0)
    assert torch.isclose(loss, risk0.double().sum().float(), rtol=1e-6)
    (2.5 * loss).backward()
    assert torch.equal(V.grad, grad0 * 2.5) and torch.equal(cost.grad, gamma0 * 2.5)
    # without a gradient for the cost the posteriors are not asked for
    V2 = V.detach().clone().requires_grad_(True)
    loss2, _, _ = mm.expected_cost(V2, cost.detach(), bf, lens)
    loss2.backward()
    assert torch.equal(V2.grad, grad0)


def test_smbr_loss_on_the_reference_path(mm, wl, torch):
    """Emissions that put all their mass on the reference alignment: every frame is correct."""
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N = 3, 80
    _, bf = _batch(mm, wl, [g] * B)
    lens = np.array([80, 66, 52], dtype=np.int32)
    pdf = np.zeros((B, N), dtype=np.int64)
    for b, L in enumerate(lens):  # a path of exactly len_b frames per utterance
        pdf[b, :L] = np.asarray(g.state2pdf)[wl.sample_paths(g, 1, int(L), seed=30 + b)[0]]
    x = np.full((B, N, g.P), -60.0, dtype=np.float32)
    np.put_along_axis(x, pdf[:, :, None], 0.0, 2)
    V = torch.from_numpy(x).cuda().requires_grad_(True)
    loss, acc, ttl = mm.smbr_loss(V, torch.from_numpy(pdf).cuda(), bf, torch.from_numpy(lens).cuda())
    assert torch.isfinite(ttl).all()
    assert np.abs(acc.detach().cpu().numpy() - lens).max() <= 1e-4
    assert abs(float(loss.detach()) + float(lens.sum())) <= 1e-3
    loss.backward()
    assert torch.isfinite(V.grad).all()
