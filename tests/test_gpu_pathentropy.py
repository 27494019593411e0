"""Posterior path entropy and its gradient (mm_pathentropy_f32) on the MI355X against the float64 reference of
tests/entropy_reference.py, and the properties of the entry: the identities of the definition on the device's own outputs, the
value-only call, emissions beyond the length never read, output strides, bit-identical repeats, hipGraph capture, error codes, the
autograd functions.

The input builders (`case_*`) are module-level so that tools/measure_entropy_floor.py can run the reference's float32 mode on the
very same inputs: the absolute parts of the bars (entropy_reference.H_ABS_PER_FRAME, GRAD_ABS_A) come from there, not from the
kernel.  They are the builders of tests/test_gpu_expectedcost.py without the cost."""
import copy
import ctypes as C

import numpy as np
import pytest

import entropy_reference as er
import test_gpu_expectedcost as tc
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu

STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
ITEM = {"MM_DEBUG": "1", "MM_KERNEL": "item"}  # pdfposteriors on the item kernel: its workspace is the alpha~ store and the offsets


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_lib, _batch = tc._lib, tc._batch


# ---- the inputs: (graphs, V, lens, utterances checked against the reference)
def _drop_cost(case):
    gs, V, _, lens, idx = case
    return gs, V, lens, idx


def case_random40(wl):
    """lens [30, 25, 1, 0, 28]; utterance 0 has a frame with three -inf entries, utterance 4 a frame of all -inf: no path."""
    return _drop_cost(tc.case_random40(wl))


def case_distinct(wl):
    return _drop_cost(tc.case_distinct(wl))


def case_config3(wl, sharp):
    """config 3's graph: sharp, B = 4, T = 500, log_softmax(10 x), three utterances checked; else B = 2, T = 1500, randn, one
    utterance checked -- the smallest case in which the centring of Hf and Hb matters."""
    g = wl.lfmmi_denominator()
    B, N = (4, 500) if sharp else (2, 1500)
    x = np.random.default_rng(3).standard_normal((B, N, g.P))
    V = (tc._log_softmax(10.0 * x) if sharp else x).astype(np.float32)
    lens = np.array([N] + [N - 37 * k for k in range(1, B)], dtype=np.int32)
    return [g] * B, V, lens, ([0, 1, B - 1] if sharp else [0])


def case_wsj(wl, name):
    return _drop_cost(tc.case_wsj(wl, name))


def case_bigv(wl):
    return _drop_cost(tc.case_bigv(wl))


def case_single_path(wl, B=2, N=12):
    """A chain: a left-to-right HMM of as many states as frames, emissions that forbid the self-loops -- one path of positive
    weight."""
    g = wl.l2r_hmm(N)
    V = np.full((B, N, g.P), -np.inf, dtype=np.float32)
    pdf = np.asarray(g.state2pdf)
    for n in range(N):
        V[:, n, pdf[n]] = np.random.default_rng(n).standard_normal(B)
    return [g] * B, V, np.full(B, N, dtype=np.int32), None


_REFS = {}


def _reference(oracle, key, g, f, V, L, N):
    """The float64 reference of one utterance, computed once per module run and shared (never modified)."""
    if key not in _REFS:
        o, oc = oracle
        _REFS[key] = er.reference(o, oc, g, f, V.astype(np.float64), L, N)
    return _REFS[key]


def _check_batch(mm, wl, oracle, case, name, bf_fs=None):
    gs, V, lens, check_idx = case
    fs, bf = bf_fs if bf_fs is not None else _batch(mm, wl, gs)
    N = V.shape[1]
    H, grad, ttl, gamma = bf.pathentropy(V, lens, want_gamma=True)
    for b in (range(len(gs)) if check_idx is None else check_idx):
        L = int(lens[b])
        ref = _reference(oracle, (name, b), gs[b], fs[b], V[b], L, N)
        er.check(H[b], grad[b], ttl[b], ref, L, label=f"{name} utterance {b}")
        if np.isfinite(ref[3]):
            check_gamma(gamma[b][None], ref[2][None], [L])
        else:
            assert (gamma[b] == 0).all()
    return bf, H, grad, ttl, gamma


def test_random_graph_lengths_and_no_path(mm, wl, oracle, torch):
    case = case_random40(wl)
    bf, H, grad, ttl, gamma = _check_batch(mm, wl, oracle, case, "rand40")
    assert "mm_entropy_fwd_kernel<8,lds>" in bf.kernels("entropy") and "mm_entropy_bwd_kernel<8,lds>" in bf.kernels("entropy")
    for b in (3, 4):
        assert np.isneginf(ttl[b]) and H[b] == 0 and (grad[b] == 0).all() and (gamma[b] == 0).all()
    # ttl is pdfposteriors' log Z
    _, t2 = bf.pdfposteriors(case[1], case[2])
    ok = np.isfinite(t2)
    assert np.allclose(ttl[ok], t2[ok], rtol=1e-5, atol=1e-4) and (np.isfinite(ttl) == ok).all()


def test_random_graph_streamed_instances(mm, wl, oracle, torch):
    case = case_random40(wl)
    bf_fs = _with_env(STREAMED, lambda: _batch(mm, wl, case[0]))
    k = bf_fs[1].kernels("entropy")
    assert "mm_entropy_fwd_kernel<0,global>" in k and "mm_entropy_bwd_kernel<0,global>" in k, k
    bf, H, grad, ttl, gamma = _check_batch(mm, wl, oracle, case, "rand40", bf_fs)
    for b in (3, 4):
        assert np.isneginf(ttl[b]) and H[b] == 0 and (grad[b] == 0).all() and (gamma[b] == 0).all()


def test_distinct_graphs(mm, wl, oracle, torch):
    _check_batch(mm, wl, oracle, case_distinct(wl), "distinct")


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph(mm, wl, oracle, torch, sharp):
    _check_batch(mm, wl, oracle, case_config3(wl, sharp), "config3 sharp" if sharp else "config3 randn")


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, oracle, torch, name):
    _check_batch(mm, wl, oracle, case_wsj(wl, name), name)


def test_bigv_graph(mm, wl, oracle, torch):
    case = case_bigv(wl)
    bf_fs = _batch(mm, wl, case[0])
    k = bf_fs[1].kernels("entropy")
    assert "mm_entropy_fwd_kernel<8,global>" in k and "mm_entropy_bwd_kernel<8,global>" in k, k
    _check_batch(mm, wl, oracle, case, "12500 states", bf_fs)


def test_identities_on_the_device_outputs(mm, wl, oracle, torch):
    gs, V, lens, _ = case_random40(wl)
    fs, bf = _batch(mm, wl, gs)
    N = V.shape[1]
    H, grad, ttl, gamma = bf.pathentropy(V, lens, want_gamma=True)
    assert np.isfinite(H).all() and (H >= 0).all() and np.isfinite(grad).all()
    for b, L in enumerate(lens):
        # sum_p grad = 0 to the rounding of the line that takes the frame's mean out: P products of |grad| <= gamma * |bracket|,
        # each rounded to float32, and the float32 sum of P such terms
        s = np.abs(grad[b].astype(np.float64).sum(axis=1))
        bound = 8 * np.finfo(np.float32).eps * (np.abs(grad[b]).sum(axis=1) + float(np.abs(grad[b]).max()))
        print(f"utterance {b}: max |sum_p grad| {s.max():.3g}, its bound {bound.max():.3g}")
        assert (s <= bound).all(), (b, s.max())
    # a constant added to the emissions of every frame changes neither H nor grad: each shifted call within the bars, against the
    # reference of the float32 emissions the device was given (the shift rounds them to 8e-6 nats), whose H stays the unshifted one
    for shift in (100.0, -150.0):
        Vs = (V + np.float32(shift)).astype(np.float32)
        H2, grad2, ttl2 = bf.pathentropy(Vs, lens)
        for b in (0, 1, 2):
            L = int(lens[b])
            ref = _reference(oracle, ("rand40", b), gs[b], fs[b], V[b], L, N)
            ref_s = _reference(oracle, ("rand40", shift, b), gs[b], fs[b], Vs[b], L, N)
            assert abs(ref_s[0] - ref[0]) <= 1e-4 * ref[0], (ref_s[0], ref[0])
            er.check(H2[b], grad2[b], ttl2[b], ref_s, L, label=f"rand40 shifted by {shift:+g} nats per frame, utterance {b}")


def test_single_path_has_exactly_no_entropy(mm, wl, torch):
    gs, V, lens, _ = case_single_path(wl)
    _, bf = _batch(mm, wl, gs)
    H, grad, ttl = bf.pathentropy(V, lens)
    assert np.isfinite(ttl).all()
    assert (H == 0).all(), H
    # grad = (g - q * mean) / q with one live state per frame, g = q * bracket: what is left is the rounding of that line, 2 eps
    # |bracket|, and the bracket here is the float32 error of ln q = 0, far below 1e-2 nats over 12 frames
    print("single path: max |grad|", np.abs(grad).max())
    assert np.abs(grad).max() <= 2 * np.finfo(np.float32).eps * 1e-2


def test_value_only_call(mm, wl, torch):
    """grad = gamma = NULL: the forward kernel alone, the same bits, and no Hf store -- a full call captured right after a
    value-only call of the same shape finds the workspace too small, one captured after a full call does not."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 300, g.P
    _, bf = _with_env(ITEM, lambda: _batch(mm, wl, [g] * B))  # (so that no other entry's workspace is larger than the full call's)
    rng = np.random.default_rng(8)
    V = torch.from_numpy(rng.standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([300, 241, 1, 113], dtype=torch.int32, device="cuda")
    H1, none, ttl1 = bf.pathentropy(V, lens, want_grad=False)
    assert none is None
    torch.cuda.synchronize()
    grad = torch.zeros((B, N, P), device="cuda")
    H = torch.zeros(B, device="cuda")
    dummy = torch.zeros(4, device="cuda")

    def captured_full_call():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            dummy.add_(1.0)
            rc = lib.mm_pathentropy_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, H.data_ptr(), grad.data_ptr(), None, N * P, P, 1,
                                        None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, graph

    rc, _ = captured_full_call()
    assert rc == -1 and b"grow" in lib.mm_last_error(), (rc, lib.mm_last_error())
    H0, grad0, ttl0 = bf.pathentropy(V, lens)
    torch.cuda.synchronize()
    assert torch.equal(H0, H1) and torch.equal(ttl0, ttl1)
    assert (H0[:2] > 1).all()
    rc, graph = captured_full_call()
    assert rc == 0, lib.mm_last_error()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(H, H0) and torch.equal(grad, grad0)
    # and the value-only call after the full one: still the same bits
    H2, _, ttl2 = bf.pathentropy(V, lens, want_grad=False)
    assert torch.equal(H2, H0) and torch.equal(ttl2, ttl0)


def test_emissions_beyond_the_length_are_not_read(mm, wl, torch):
    gs, V, lens, _ = case_random40(wl)
    _, bf = _batch(mm, wl, gs)
    clean = bf.pathentropy(V, lens, want_gamma=True)
    dirty = V.copy()
    for b, L in enumerate(lens):
        dirty[b, L:] = np.nan
    out = bf.pathentropy(dirty, lens, want_gamma=True)
    for x, y in zip(clean, out):
        assert x.tobytes() == y.tobytes()


def test_column_major_output_strides(mm, wl, torch):
    """The reference's B x P x N column-major layout: g_stride_b = 1, g_stride_p = B, g_stride_n = B * P."""
    lib = _lib(mm)
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 4, 50, g.P
    _, bf = _batch(mm, wl, [g] * B)
    V = torch.from_numpy(np.random.default_rng(8).standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([50, 41, 50, 13], dtype=torch.int32, device="cuda")
    H0, grad0, ttl0, gamma0 = bf.pathentropy(V, lens, want_gamma=True)
    grad = torch.full((N, P, B), 7.0, device="cuda")   # element (b, n, p) at b + p * B + n * B * P
    gamma = torch.full((N, P, B), 7.0, device="cuda")
    H, ttl = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    rc = lib.mm_pathentropy_f32(bf._h, V.data_ptr(), N * P, P, lens.data_ptr(), N, H.data_ptr(), grad.data_ptr(), gamma.data_ptr(), 1, B * P, B,
                                ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(grad.permute(2, 0, 1), grad0) and torch.equal(gamma.permute(2, 0, 1), gamma0)
    assert torch.equal(H, H0) and torch.equal(ttl, ttl0)


def test_bit_identical_and_graph_capture(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    _, bf = _batch(mm, wl, [g] * 6)
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    out0 = bf.pathentropy(V, lens, want_gamma=True)
    out1 = bf.pathentropy(V, lens, want_gamma=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = bf.pathentropy(V, lens, want_gamma=True)
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
    grad = torch.zeros((B, N, P), device="cuda")
    H = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, H_ptr, grad_ptr, gsn, Vt=V):
        return lib.mm_pathentropy_f32(h, Vt.data_ptr(), N * P, P, None, N, H_ptr, grad_ptr, None, N * P, gsn, 1, None, st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(tb._h, H.data_ptr(), grad.data_ptr(), P) == -4
    assert b"log" in lib.mm_last_error()
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h, H.data_ptr(), grad.data_ptr(), P, Vt=torch.ones((B, N, P), device="cuda")) == -4
    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h, None, grad.data_ptr(), P) == -1
    assert call(lb._h, H.data_ptr(), grad.data_ptr(), P - 1) == -2
    assert call(lb._h, H.data_ptr(), None, P - 1) == 0  # (no output with strides: they are not looked at)
    assert call(lb._h, H.data_ptr(), grad.data_ptr(), P) == 0
    torch.cuda.synchronize()
    assert "mm_entropy_fwd_kernel" in lb.kernels("entropy") and "mm_entropy_bwd_kernel" in lb.kernels("entropy")
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("entropy")


def test_autograd_path_entropy(mm, wl, torch):
    g = wl.lfmmi_denominator(300, 20, seed=3)
    B, N, P = 3, 60, g.P
    _, bf = _batch(mm, wl, [g] * B)
    V = torch.from_numpy(np.random.default_rng(9).standard_normal((B, N, P)).astype(np.float32)).cuda().requires_grad_(True)
    lens = torch.tensor([60, 44, 31], dtype=torch.int32, device="cuda")
    H0, grad0, ttl0 = bf.pathentropy(V.detach(), lens)
    total, H, ttl = mm.path_entropy(V, bf, lens)
    assert torch.equal(H, H0) and torch.equal(ttl, ttl0)
    assert torch.isclose(total, H0.double().sum().float(), rtol=1e-6)
    (2.5 * total).backward()
    assert torch.equal(V.grad, grad0 * 2.5)
    # per-utterance weights reach the gradient through the second output
    V2 = V.detach().clone().requires_grad_(True)
    w = torch.tensor([1.0, 0.0, -2.0], device="cuda")
    (mm.path_entropy(V2, bf, lens)[1] * w).sum().backward()
    assert torch.equal(V2.grad, grad0 * w[:, None, None])
    # the semi-supervised objective is the sum; without a gradient to compute, the value alone
    loss, H3, _ = mm.conditional_entropy_loss(V.detach(), bf, lens)
    assert torch.equal(H3, H0) and torch.isclose(loss, total.detach())
    # under no_grad a leaf that requires a gradient gets the value-only call: no gradient is asked of the engine
    asked = []
    orig = bf.pathentropy
    bf.pathentropy = lambda *a, **k: (asked.append(k.get("want_grad", True)), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            _, H4, _ = mm.path_entropy(V, bf, lens)
        mm.path_entropy(V, bf, lens)
    finally:
        del bf.pathentropy
    assert asked == [False, True] and torch.equal(H4, H0)
