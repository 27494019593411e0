"""Arc posteriors (mm_arcposteriors_f32) on the MI355X against the float64 reference of tests/arc_reference.py, and the
properties of the entry: bit-identical repeats, hipGraph capture, d log Z / d log w, EM, error codes."""
import ctypes as C
import os

import numpy as np
import pytest

import arc_reference as ar

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
    fs = [wl.to_fsm(mm, g) for g in gs]
    return fs, mm.batch(*[mm.compile(f, mm.statemap(g.state2pdf, g.P)) for f, g in zip(fs, gs)])


def _check_batch(mm, wl, oracle, gs, V, lens, check_idx=None, want_batch=False):
    o, oc = oracle
    fs, bf = _batch(mm, wl, gs)
    N = V.shape[1]
    c, ttl, init = bf.arcposteriors(V, lens, want_init=True)
    for b in (range(len(gs)) if check_idx is None else check_idx):
        f = fs[b]
        c_ref, i_ref, z_ref = ar.reference(o, oc, gs[b], f, V[b].astype(np.float64), int(lens[b]), N)
        worst = ar.check(c[b, : f.nnz], init[b, : len(f.alpha_idx)], ttl[b], c_ref, i_ref, z_ref, int(lens[b]), N)
        print(f"utterance {b}: len {int(lens[b])}, worst arc count error / bar {worst:.3g}")
        assert (c[b, f.nnz :] == 0).all()
    return (c, ttl, bf) if want_batch else (c, ttl)


def test_random_graph_lengths_and_no_path(mm, wl, oracle, torch):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((5, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf   # a frame with -inf entries
    V[4, 4, :] = -np.inf    # no accepting path
    c, ttl = _check_batch(mm, wl, oracle, [g] * 5, V, lens)
    assert np.isneginf(ttl[3]) and np.isneginf(ttl[4]) and (c[3] == 0).all() and (c[4] == 0).all()
    # ttl is pdfposteriors' log Z
    _, bf = _batch(mm, wl, [g] * 5)
    _, t2 = bf.pdfposteriors(V, lens)
    ok = np.isfinite(t2)
    assert np.allclose(ttl[ok], t2[ok], rtol=1e-5, atol=1e-4) and (np.isfinite(ttl) == ok).all()


@pytest.mark.parametrize("sharp", [False, True])
def test_config3_graph(mm, wl, oracle, torch, sharp):
    g = wl.lfmmi_denominator()
    B, N = (8, 1500) if not sharp else (4, 500)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, N, g.P))
    V = (torch.log_softmax(torch.from_numpy(10.0 * x), dim=-1).numpy() if sharp else x).astype(np.float32)
    lens = np.array([N] + [N - 37 * k for k in range(1, B)], dtype=np.int32)
    _check_batch(mm, wl, oracle, [g] * B, V, lens, check_idx=[0, 1, B - 1])


@pytest.mark.parametrize("name", ["den_fsm_wsj", "num_fsm_wsj"])
def test_wsj_graphs(mm, wl, oracle, torch, name):
    g = wl.load_npz_graph(os.path.join(HERE, "golden", name + ".npz"))
    B, N = 3, 700
    V = np.random.default_rng(11).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([N, 611, 430], dtype=np.int32) if name.startswith("den") else np.array([N, 650, 500], dtype=np.int32)
    _check_batch(mm, wl, oracle, [g] * B, V, lens)


def test_distinct_graphs_in_their_own_order(mm, wl, oracle, torch):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    _check_batch(mm, wl, oracle, gs, V, lens)


def test_csr_layout_with_scrambled_entries(mm, wl, oracle, torch):
    """An FSM handed over as CSR(T_hat) with the entries of every row in a scrambled order: the counts come back in that order."""
    _scrambled_csr_run(mm, wl, oracle, torch)


def _scrambled_csr_run(mm, wl, oracle, torch):
    """The case above; returns mm_batch_kernels' text for the arc entry of the batch it ran."""
    o, oc = oracle
    lib = _lib(mm)
    g = wl.random_fsm(50, 4, 3.0, seed=9)
    f = wl.to_fsm(mm, g)
    i, j, w = ar.fsm_entries(f)
    rng = np.random.default_rng(1)
    order = np.lexsort((rng.random(i.size), i))  # by source, scrambled inside a row
    S1 = f.colptr.size - 1
    ptr = np.zeros(S1 + 1, dtype=np.int64)
    np.add.at(ptr, i + 1, 1)
    ptr = np.cumsum(ptr)
    idx = np.ascontiguousarray(j[order], dtype=np.int64)
    val = np.ascontiguousarray(w[order], dtype=np.float32)
    aidx = np.ascontiguousarray(f.alpha_idx[::-1], dtype=np.int64)
    aval = np.ascontiguousarray(np.asarray(f.alpha_val)[::-1], dtype=np.float32)
    s2p = np.ascontiguousarray(list(g.state2pdf) + [g.P], dtype=np.int32)
    h = C.c_void_p()
    assert lib.mm_fsm_create(0, S1, i.size, 1, 8, 0, 4, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, aidx.size,
                             aidx.ctypes.data, aval.ctypes.data, s2p.ctypes.data, g.P + 1, C.byref(h)) == 0
    bh = C.c_void_p()
    arr = (C.c_void_p * 2)(h, h)
    assert lib.mm_batch_create(arr, 2, C.byref(bh)) == 0
    N = 25
    V = torch.from_numpy(np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([25, 19], dtype=torch.int32, device="cuda")
    K = i.size + 3
    counts = torch.full((2, K), -7.0, device="cuda")
    init = torch.zeros((2, aidx.size), device="cuda")
    ttl = torch.empty(2, device="cuda")
    rc = lib.mm_arcposteriors_f32(bh, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, counts.data_ptr(), K,
                                  init.data_ptr(), aidx.size, ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    c, ini, t = counts.cpu().numpy(), init.cpu().numpy(), ttl.cpu().numpy()
    for b, L in enumerate([25, 19]):
        c_ref, i_ref, z_ref = ar.reference(o, oc, g, f, V[b].cpu().numpy().astype(np.float64), L, N)
        ar.check(c[b, : i.size], ini[b], t[b], c_ref[order], i_ref[::-1], z_ref, L, N)
        assert (c[b, i.size :] == -7.0).all()  # slots beyond nnz are left alone
    buf = C.create_string_buffer(1024)
    assert lib.mm_batch_kernels(bh, 4, buf, 1024) == 0
    lib.mm_batch_destroy(bh)
    lib.mm_fsm_destroy(h)
    return buf.value.decode()


def test_bigv_graph(mm, wl, oracle, torch):
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    N = 40
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([40, 29], dtype=np.int32)
    _, bf = _batch(mm, wl, [g, g])
    assert "mm_arc_kernel<8>" in bf.kernels("arcs")
    _check_batch(mm, wl, oracle, [g, g], V, lens)


def test_bit_identical_and_graph_capture(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    _, bf = _batch(mm, wl, [g] * 6)
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    c0, t0, i0 = bf.arcposteriors(V, lens, want_init=True)
    c1, t1, i1 = bf.arcposteriors(V, lens, want_init=True)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and torch.equal(t0, t1) and torch.equal(i0, i1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c2, t2, i2 = bf.arcposteriors(V, lens, want_init=True)
    for _ in range(2):
        c2.zero_()
        t2.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c2, c0) and torch.equal(t2, t0) and torch.equal(i2, i0)


def test_gradient_of_log_z(mm, wl, torch):
    """c[k] = d log Z / d log w_k: central differences of ttl."""
    g = wl.random_fsm(8, 4, 2.5, seed=5)
    f = wl.to_fsm(mm, g)
    N, L = 12, 12
    V = np.random.default_rng(8).standard_normal((1, N, g.P)).astype(np.float32)
    sm = mm.statemap(g.state2pdf, g.P)
    c, ttl = mm.batch(mm.compile(f, sm)).arcposteriors(V, [L])
    eps = 1e-2
    for k in range(f.nnz):
        tt = []
        for s in (eps, -eps):
            f2 = wl.to_fsm(mm, g)
            f2.nzval = f2.nzval.copy()
            f2.nzval[k] += np.float32(s)
            tt.append(float(mm.batch(mm.compile(f2, sm)).arcposteriors(V, [L])[1][0]))
        assert abs((tt[0] - tt[1]) / (2 * eps) - c[0, k]) <= 1e-2, (k, tt, c[0, k])


def test_em_on_a_dense_ergodic_hmm(mm, wl, torch):
    """Five EM iterations re-estimating T and omega from the counts (the phony self-loop excluded): the total
    log-likelihood never decreases."""
    g = wl.dense_ergodic(64)
    B, N = 6, 80
    V = np.random.default_rng(9).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([80, 75, 60, 80, 33, 50], dtype=np.int32)
    f = wl.to_fsm(mm, g)
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    phony = (i == fs) & (j == fs)
    sm = mm.statemap(g.state2pdf, g.P)
    last = -np.inf
    for it in range(5):
        c, ttl = mm.batch(*([mm.compile(f, sm)] * B)).arcposteriors(V, lens)
        total = float(np.sum(ttl.astype(np.float64)))
        assert total >= last - 1e-3, (it, total, last)
        last = total
        cs = c[:, : f.nnz].astype(np.float64).sum(axis=0)
        tot = np.zeros(fs + 1)
        np.add.at(tot, i[~phony], cs[~phony])
        w = np.where(phony, 0.0, np.log(np.maximum(cs, 1e-30) / np.maximum(tot[i], 1e-30)))
        f = wl.to_fsm(mm, g)
        f.nzval = w.astype(np.float32)


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N = 10
    V = torch.zeros((2, N, g.P), device="cuda")
    c = torch.zeros((2, 1000), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * 2))
    assert lib.mm_arcposteriors_f32(tb._h, V.data_ptr(), N * g.P, g.P, None, N, c.data_ptr(), 1000, None, 0, None, st) == -4
    assert b"log" in lib.mm_last_error()
    f = wl.to_fsm(mm, g)
    lb = mm.batch(*([mm.compile(f, mm.statemap(g.state2pdf, g.P))] * 2))
    assert lib.mm_arcposteriors_f32(lb._h, V.data_ptr(), N * g.P, g.P, None, N, c.data_ptr(), f.nnz - 1, None, 0, None, st) == -2
    assert lib.mm_arcposteriors_f32(lb._h, V.data_ptr(), N * g.P, g.P, None, N, None, 1000, None, 0, None, st) == -1
    assert lib.mm_arcposteriors_f32(lb._h, V.data_ptr(), N * g.P, g.P, None, N, c.data_ptr(), f.nnz, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert np.isclose(float(c.view(-1)[: 2 * f.nnz].sum()), 2 * N, rtol=1e-4)  # (c_stride_b = nnz: the two utterances back to back)
    assert (c.view(-1)[2 * f.nnz :] == 0).all()
    assert "mm_arc_kernel" in lb.kernels("arcs")
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("arcs")
