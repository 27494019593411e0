"""Posteriors with call-time arc weights (mm_weightedposteriors_f32) on the GPU: every utterance and every entry against the float64
reference of tests/weighted_reference.py, gamma to check_gamma's bar (tests/test_gpu_parity.py), counts, init_counts and ttl to
arc_reference.check's.  Unless said otherwise the weights are the FSM's own plus N(0, 0.5) noise, per utterance."""
import ctypes as C

import numpy as np
import pytest

import arc_reference as ar
import weighted_reference as wr
from test_gpu_itemform import case_wide
from test_gpu_parity import _with_env, check_gamma

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
    """(FSMs, BatchedFSM): one compiled handle per distinct graph object."""
    cfs = {}
    fs = []
    for g in gs:
        if id(g) not in cfs:
            f = wl.to_fsm(mm, g)
            cfs[id(g)] = (f, mm.compile(f, mm.statemap(g.state2pdf, g.P)))
        fs.append(cfs[id(g)][0])
    return fs, mm.batch(*[cfs[id(g)][1] for g in gs])


def _noisy(rng, fs, sigma=0.5):
    """Per-utterance W [B, max nnz] and W_init [B, max n_init] in float32 (slack at 0)."""
    K, I = max(f.nnz for f in fs), max(len(f.alpha_idx) for f in fs)
    W, Wi = np.zeros((len(fs), K), dtype=np.float32), np.zeros((len(fs), I), dtype=np.float32)
    for b, f in enumerate(fs):
        W[b, : f.nnz] = np.asarray(f.nzval, dtype=np.float32) + (sigma * rng.standard_normal(f.nnz)).astype(np.float32)
        Wi[b, : len(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float32) + (sigma * rng.standard_normal(len(f.alpha_idx))).astype(np.float32)
    return W, Wi


def _refs(gs, fs, V, lens, W=None, Wi=None):
    """The float64 reference of every utterance: a list of (gamma, counts, init, log Z).  W / Wi: None, 1-D (shared) or per utterance."""
    N = V.shape[1]
    row = lambda w, b: None if w is None else (w if np.ndim(w) == 1 else w[b])  # noqa: E731
    return [wr.reference(f, g.state2pdf, g.P, V[b].astype(np.float64), int(lens[b]), N, row(W, b), row(Wi, b)) for b, (g, f) in enumerate(zip(gs, fs))]


def _check(out, refs, fs, lens, N, what=""):
    """Every utterance, every entry: gamma, counts, init, ttl (each may be None: not asked for)."""
    gamma, counts, ttl, init = (None if t is None else np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in out)
    if gamma is not None:
        assert np.isfinite(gamma).all(), what
        g_ref = np.stack([r[0] for r in refs])
        # (an utterance without a path has no frame that sums to 1: all its frames must be exact zeros)
        worst_g = check_gamma(gamma, g_ref, [int(L) if np.isfinite(r[3]) else 0 for L, r in zip(lens, refs)])
        print(f"[weighted] {what}: gamma worst error over its bar {worst_g:.4f}")
    worst_c = 0.0
    for b, (f, r) in enumerate(zip(fs, refs)):
        if counts is not None:
            assert np.isfinite(counts[b]).all(), (what, b)
            worst_c = max(worst_c, ar.check(counts[b, : f.nnz], None if init is None else init[b, : len(f.alpha_idx)], ttl[b], r[1], r[2], r[3], int(lens[b]), N))
        else:
            if np.isfinite(r[3]):
                assert np.isclose(ttl[b], r[3], rtol=1e-5, atol=1e-5 * max(1.0, abs(r[3])) + 1e-4), (what, b, ttl[b], r[3])
            else:
                assert np.isneginf(ttl[b]), (what, b)
    if counts is not None:
        print(f"[weighted] {what}: counts worst error over their bar {worst_c:.4f}")


def _base_case(wl):
    """random_fsm(40, 6, 3.0), B = 6, N = 30, lens (30, 25, 1, 0, 28, 30): a frame with -inf entries (utterance 0), an utterance killed
    by V (4: one whole frame at -inf), one killed by W (5: its final entries at -inf), a handful of single entries at -inf
    (utterances 0 and 1), W_init perturbed."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    B, N = 6, 30
    rng = np.random.default_rng(81)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    V[0, 7, [1, 4]] = -np.inf
    V[4, 11, :] = -np.inf
    lens = np.array([30, 25, 1, 0, 28, 30], dtype=np.int32)
    return g, B, N, V, lens, rng


def _base_weights(mm, wl, g, fs, rng):
    W, Wi = _noisy(rng, fs)
    i, j, _ = ar.fsm_entries(fs[0])
    fin = j == g.S
    W[5, np.flatnonzero(fin & (i != g.S))] = -np.inf
    real = np.flatnonzero(~fin)
    W[0, real[[2, 9, 33]]] = -np.inf
    W[1, real[[5, 50]]] = -np.inf
    W[:, np.flatnonzero(fin & (i == g.S))] = 77.0  # (garbage at the phony self-loop's index)
    return W, Wi


def _run_base(mm, wl, torch, env=None):
    g, B, N, V, lens, rng = _base_case(wl)
    fs, bf = _with_env(env or {}, lambda: _batch(mm, wl, [g] * B))
    W, Wi = _base_weights(mm, wl, g, fs, rng)
    out = bf.weightedposteriors(torch.from_numpy(V).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(Wi).cuda(), torch.from_numpy(lens).cuda(), want_init=True)
    torch.cuda.synchronize()
    return bf, out, _base_refs(wl), fs, lens, N, W


_BASE_REFS = []


def _base_refs(wl):
    """The base case's references, computed once and shared by the tests that run it on different instances."""
    if not _BASE_REFS:
        import __graft_entry__ as ge

        mm = ge.load_package()
        g, B, N, V, lens, rng = _base_case(wl)
        fs = [wl.to_fsm(mm, g)] * B
        W, Wi = _base_weights(mm, wl, g, fs, rng)
        _BASE_REFS.append(_refs([g] * B, fs, V, lens, W, Wi))
    return _BASE_REFS[0]


def test_base_case(mm, wl, torch):
    bf, out, refs, fs, lens, N, W = _run_base(mm, wl, torch)
    assert "mm_weighted_bwd_kernel<8,lds>" in bf.kernels("weighted") and "mm_weights_kernel" in bf.kernels("weighted")
    assert [bool(np.isfinite(r[3])) for r in refs][3:] == [False, False, False]  # (len 0, killed by V, killed by W)
    assert np.isfinite(refs[0][3]) and np.isfinite(refs[1][3])
    _check(out, refs, fs, lens, N, "base")
    assert np.isneginf(W[:2]).sum() == 5 and (out[1].cpu().numpy()[:2][np.isneginf(W[:2])] == 0).all()  # an entry at -inf has count 0


def test_distinct_graphs_with_a_sentinel_behind_their_entries(mm, wl, torch):
    """Four graphs of different nnz, c_stride_b and w_stride_b larger than every nnz: each utterance in its own entry order, what lies
    behind an FSM's own entries is untouched."""
    gs = [wl.random_fsm(40, 6, 3.0, seed=1), wl.random_fsm(55, 6, 2.5, seed=2), wl.random_fsm(30, 6, 4.0, seed=3), wl.random_fsm(48, 6, 2.0, seed=4, n_init=4)]
    fs, bf = _batch(mm, wl, gs)
    assert len({f.nnz for f in fs}) == 4
    B, N = 4, 22
    rng = np.random.default_rng(82)
    V = rng.standard_normal((B, N, 6)).astype(np.float32)
    lens = np.array([22, 15, 22, 9], dtype=np.int32)
    W, Wi = _noisy(rng, fs)
    K, I = W.shape[1] + 5, Wi.shape[1] + 3
    Wp, Wip = np.full((B, K), np.nan, dtype=np.float32), np.full((B, I), np.nan, dtype=np.float32)  # (NaN behind the entries: never read)
    for b, f in enumerate(fs):
        Wp[b, : f.nnz], Wip[b, : len(f.alpha_idx)] = W[b, : f.nnz], Wi[b, : len(f.alpha_idx)]
    Vt, lt, Wt, Wit = (torch.from_numpy(x).cuda() for x in (V, lens, Wp, Wip))
    gamma = torch.empty((B, N, 6), device="cuda")
    counts, init, ttl = torch.full((B, K), -7.0, device="cuda"), torch.full((B, I), -7.0, device="cuda"), torch.empty(B, device="cuda")
    rc = _lib(mm).mm_weightedposteriors_f32(bf._h, Vt.data_ptr(), N * 6, 6, lt.data_ptr(), N, Wt.data_ptr(), K, Wit.data_ptr(), I, gamma.data_ptr(), N * 6, 6, 1,
                                            counts.data_ptr(), K, init.data_ptr(), I, ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib(mm).mm_last_error()
    torch.cuda.synchronize()
    for b, f in enumerate(fs):
        assert (counts[b, f.nnz :] == -7.0).all() and (init[b, len(f.alpha_idx) :] == -7.0).all(), b
    _check((gamma, counts, ttl, init), _refs(gs, fs, V, lens, W, Wi), fs, lens, N, "distinct")


def test_shared_weights(mm, wl, torch):
    """One handle four times: a 1-D W (stride 0: one plane for the batch) against the same vector repeated per utterance, bit for
    bit in every output; against the reference; stride 0 on distinct handles is refused."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    fs, bf = _batch(mm, wl, [g] * 4)
    N = 26
    rng = np.random.default_rng(83)
    V = rng.standard_normal((4, N, g.P)).astype(np.float32)
    lens = np.array([26, 20, 26, 3], dtype=np.int32)
    W, Wi = _noisy(rng, fs[:1])
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    a = bf.weightedposteriors(Vt, torch.from_numpy(W[0]).cuda(), torch.from_numpy(Wi[0]).cuda(), lt, want_init=True)
    b = bf.weightedposteriors(Vt, torch.from_numpy(np.repeat(W, 4, 0)).cuda(), torch.from_numpy(np.repeat(Wi, 4, 0)).cuda(), lt, want_init=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _check(a, _refs([g] * 4, fs, V, lens, W[0], Wi[0]), fs, lens, N, "shared")
    g2 = wl.random_fsm(40, 6, 3.0, seed=1)  # (the same graph compiled twice: two handles)
    _, bd = _batch(mm, wl, [g, g2])
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        bd.weightedposteriors(Vt[:2], torch.from_numpy(W[0]).cuda(), None, lt[:2])
    assert ei.value.code == -1 and "same FSM" in str(ei.value)
    with pytest.raises(mm.MarkovModelsAMDError) as ei:
        bd.weightedposteriors(Vt[:2], None, torch.from_numpy(Wi[0]).cuda(), lt[:2])
    assert ei.value.code == -1


def _within_two_bars(c, c2, c_ref, L):
    return (np.abs(np.asarray(c, dtype=np.float64) - np.asarray(c2, dtype=np.float64)) <= 2 * (1e-4 * c_ref + 1e-6 * max(L, 1))).all()


def test_both_weight_arguments_null(mm, wl, torch):
    """The FSMs' own weights: against the reference, and against arcposteriors of the same batch within the sum of both bars."""
    g, B, N, V, lens, _ = _base_case(wl)
    fs, bf = _batch(mm, wl, [g] * B)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    out = bf.weightedposteriors(Vt, None, None, lt, want_init=True)
    c_a, t_a, i_a = bf.arcposteriors(Vt, lt, want_init=True)
    torch.cuda.synchronize()
    refs = _refs([g] * B, fs, V, lens)
    _check(out, refs, fs, lens, N, "own weights")
    c, ttl, init = out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()
    c_a, t_a, i_a = c_a.cpu().numpy(), t_a.cpu().numpy(), i_a.cpu().numpy()
    for b, r in enumerate(refs):
        if not np.isfinite(r[3]):
            assert np.isneginf(ttl[b]) and np.isneginf(t_a[b]) and (c[b] == 0).all() and (c_a[b] == 0).all()
            continue
        assert _within_two_bars(c[b], c_a[b], r[1], int(lens[b])), b
        assert (np.abs(init[b].astype(np.float64) - i_a[b]) <= 2 * (1e-4 * r[2] + 1e-6)).all(), b
        assert abs(float(ttl[b]) - float(t_a[b])) <= 2 * (1e-5 * abs(r[3]) + 1e-5 * max(1.0, abs(r[3])) + 1e-4), b


@pytest.mark.parametrize("env,inst", [(STREAMED, "<0,global>"), (BIGV, "<8,global>")], ids=["streamed", "bigv"])
def test_forced_instances(mm, wl, torch, env, inst):
    bf, out, refs, fs, lens, N, _ = _run_base(mm, wl, torch, env)
    assert "mm_weighted_bwd_kernel" + inst in bf.kernels("weighted"), bf.kernels("weighted")
    _check(out, refs, fs, lens, N, inst)


def _run_case(mm, wl, torch, gs, V, lens, seed, inst):
    fs, bf = _batch(mm, wl, gs)
    assert "mm_weighted_bwd_kernel" + inst in bf.kernels("weighted"), bf.kernels("weighted")
    W, Wi = _noisy(np.random.default_rng(seed), fs)
    out = bf.weightedposteriors(torch.from_numpy(V).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(Wi).cuda(), torch.from_numpy(lens).cuda(), want_init=True)
    torch.cuda.synchronize()
    _check(out, _refs(gs, fs, V, lens, W, Wi), fs, lens, V.shape[1], inst)


def test_vectors_global_by_the_plan(mm, wl, torch):
    """12 500 states: five vectors of 4 bytes per state exceed the 160 KB of a compute unit."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    V = np.random.default_rng(84).standard_normal((2, 40, g.P)).astype(np.float32)
    _run_case(mm, wl, torch, [g, g], V, np.array([40, 23], dtype=np.int32), 85, "<8,global>")


def test_beyond_16_bit_indices(mm, wl, torch):
    """70 000 states: every item streamed, 32-bit state indices."""
    g = wl.random_fsm(70000, 40, 3.0, seed=3)
    V = np.random.default_rng(86).standard_normal((1, 10, g.P)).astype(np.float32)
    _run_case(mm, wl, torch, [g], V, np.array([10], dtype=np.int32), 87, "<0,global>")


def test_more_pdfs_than_threads(mm, wl, torch):
    """600 pdfs against at most 512 threads: the emissions of a frame are staged in two parts, the per-pdf pass makes two rounds."""
    g = wl.random_fsm(700, 600, 3.0, seed=9)
    V = np.random.default_rng(88).standard_normal((2, 14, g.P)).astype(np.float32)
    _run_case(mm, wl, torch, [g, g], V, np.array([14, 9], dtype=np.int32), 89, "<8,lds>")


@pytest.mark.parametrize("name", ["wide", "ergodic300", "lexicon"])
def test_wide_rows(mm, wl, torch, name):
    """Rows of 140 to 650 arcs in both directions (the shapes of tests/test_gpu_itemform.py): streamed long rows, lane groups of 17 to 64."""
    gs, V, _, lens, _ = case_wide(wl, name)
    _run_case(mm, wl, torch, gs, V, lens, 90, "<8,lds>")


def _den_inputs(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40)
    fs, bf = _batch(mm, wl, [g] * 6)
    N = 120
    V = torch.from_numpy(np.random.default_rng(91).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    W, Wi = _noisy(np.random.default_rng(92), fs)
    W2, _ = _noisy(np.random.default_rng(93), fs)
    return g, fs, bf, N, V, lens, torch.from_numpy(W).cuda(), torch.from_numpy(Wi).cuda(), torch.from_numpy(W2).cuda()


def test_bit_identical_graph_capture_and_weights_overwritten_in_place(mm, wl, torch):
    g, fs, bf, N, V, lens, W, Wi, W2 = _den_inputs(mm, wl, torch)
    out0 = bf.weightedposteriors(V, W, Wi, lens, want_init=True)
    out1 = bf.weightedposteriors(V, W, Wi, lens, want_init=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    _check(out0, _refs([g] * 6, fs, V.cpu().numpy(), lens.cpu().numpy(), W.cpu().numpy(), Wi.cpu().numpy()), fs, lens.cpu().numpy(), N, "den600")
    Wc = W.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = bf.weightedposteriors(V, Wc, Wi, lens, want_init=True)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out2, out0))
    Wc.copy_(W2)  # in place: the graph reads the same buffer
    graph.replay()
    torch.cuda.synchronize()
    fresh = bf.weightedposteriors(V, W2, Wi, lens, want_init=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out2, fresh))
    assert not torch.equal(out2[2], out0[2]) and not torch.equal(out2[1], out0[1])


def test_capture_before_a_first_call_is_refused(mm, wl, torch):
    g, fs, fresh, N, V, lens, W, Wi, _ = _den_inputs(mm, wl, torch)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.weightedposteriors(V, W, Wi, lens)
    assert ei.value.code == -1 and "not on the device yet" in str(ei.value)
    out = fresh.weightedposteriors(V, W, Wi, lens)  # ... and the batch works afterwards
    torch.cuda.synchronize()
    assert torch.isfinite(out[2]).all()


def test_optional_outputs_and_column_major_gamma(mm, wl, torch):
    """counts only, gamma only and ttl only each equal the full call's values bit for bit; gamma through column-major strides (the
    reference's B x P x N layout)."""
    g, B, N, V, lens, rng = _base_case(wl)
    fs, bf = _batch(mm, wl, [g] * B)
    W, Wi = _base_weights(mm, wl, g, fs, rng)
    Vt, lt, Wt, Wit = (torch.from_numpy(x).cuda() for x in (V, lens, W, Wi))
    full = bf.weightedposteriors(Vt, Wt, Wit, lt, want_init=True)
    c_only = bf.weightedposteriors(Vt, Wt, Wit, lt, want_gamma=False)
    g_only = bf.weightedposteriors(Vt, Wt, Wit, lt, want_counts=False)
    lib, st = _lib(mm), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ttl = torch.empty(B, device="cuda")
    rc = lib.mm_weightedposteriors_f32(bf._h, Vt.data_ptr(), N * g.P, g.P, lt.data_ptr(), N, Wt.data_ptr(), W.shape[1], Wit.data_ptr(), Wi.shape[1],
                                       None, 0, 0, 0, None, 0, None, 0, ttl.data_ptr(), st)
    assert rc == 0, lib.mm_last_error()
    colmajor = torch.full((N, g.P, B), -3.0, device="cuda")  # element (b, n, p) at b + B * p + B * P * n
    out_cm = bf.weightedposteriors(Vt, Wt, Wit, lt, want_counts=False, out=colmajor.permute(2, 0, 1))
    torch.cuda.synchronize()
    assert c_only[0] is None and torch.equal(c_only[1], full[1]) and torch.equal(c_only[2], full[2])
    assert g_only[1] is None and torch.equal(g_only[0], full[0]) and torch.equal(g_only[2], full[2])
    assert torch.equal(ttl, full[2])
    assert out_cm[0].stride() == (1, B * g.P, B) and torch.equal(out_cm[0].contiguous(), full[0])


def test_against_compiled_weights(mm, wl, torch):
    """A second batch whose FSMs are compiled FROM the call's weights: its arcposteriors and pdfposteriors agree with the entry
    within the sum of the bars."""
    gs = [wl.random_fsm(40, 6, 3.0, seed=1), wl.random_fsm(55, 6, 2.5, seed=2), wl.lfmmi_denominator(200, 6, seed=3, n_init=9)]
    fs, bf = _batch(mm, wl, gs)
    B, N = 3, 28
    rng = np.random.default_rng(94)
    V = rng.standard_normal((B, N, 6)).astype(np.float32)
    lens = np.array([28, 19, 28], dtype=np.int32)
    W, Wi = _noisy(rng, fs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    out = bf.weightedposteriors(Vt, torch.from_numpy(W).cuda(), torch.from_numpy(Wi).cuda(), lt, want_init=True)
    g2s = [wr.rebuilt(g, f, W[b, : f.nnz], Wi[b, : len(f.alpha_idx)]) for b, (g, f) in enumerate(zip(gs, fs))]
    f2s, b2 = _batch(mm, wl, g2s)
    assert all(f2.nnz == f.nnz and (f2.rowval == f.rowval).all() for f, f2 in zip(fs, f2s))
    c_a, t_a, i_a = b2.arcposteriors(Vt, lt, want_init=True)
    g_p, t_p = b2.pdfposteriors(Vt, lt)
    torch.cuda.synchronize()
    refs = _refs(gs, fs, V, lens, W, Wi)
    gamma, c, ttl, init = (t.cpu().numpy().astype(np.float64) for t in out)
    c_a, t_a, i_a, g_p, t_p = (t.cpu().numpy().astype(np.float64) for t in (c_a, t_a, i_a, g_p, t_p))
    assert np.abs(gamma - g_p).max() <= 2 * 2e-5
    for b, (f, r) in enumerate(zip(fs, refs)):
        assert np.isfinite(r[3])
        assert _within_two_bars(c[b, : f.nnz], c_a[b, : f.nnz], r[1], int(lens[b])), b
        assert (np.abs(init[b, : len(f.alpha_idx)] - i_a[b, : len(f.alpha_idx)]) <= 2 * (1e-4 * r[2] + 1e-6)).all(), b
        bar = 2 * (1e-5 * abs(r[3]) + 1e-5 * max(1.0, abs(r[3])) + 1e-4)
        assert abs(ttl[b] - t_a[b]) <= bar and abs(ttl[b] - t_p[b]) <= bar, b


def test_graph_loglik_gradients(mm, wl, torch):
    """Gradients against V, shared W, per-utterance W and W_init against the reference's, within the entry's bars times |g_b|; an
    utterance without a path yields zeros."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    B, N = 4, 24
    fs, bf = _batch(mm, wl, [g] * B)
    rng = np.random.default_rng(95)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    V[3, 5, :] = -np.inf  # (no path)
    lens = np.array([24, 17, 24, 24], dtype=np.int32)
    W, Wi = _noisy(rng, fs)
    gb = np.array([1.0, -2.5, 0.5, 3.0])
    gt = torch.from_numpy(gb.astype(np.float32)).cuda()
    lt = torch.from_numpy(lens).cuda()
    for shared in (False, True):
        Wn, Win = (W[0], Wi[0]) if shared else (W, Wi)
        Vt = torch.from_numpy(V).cuda().requires_grad_(True)
        Wt = torch.from_numpy(Wn).cuda().requires_grad_(True)
        Wit = torch.from_numpy(Win).cuda().requires_grad_(True)
        ttl = mm.graph_loglik(Vt, bf, Wt, Wit, lt)
        assert np.isneginf(float(ttl.detach()[3]))
        (ttl[:3] * gt[:3]).sum().backward()  # (the loss leaves the dead utterance out, as lfmmi_loss's callers do)
        torch.cuda.synchronize()
        refs = _refs([g] * B, fs, V, lens, Wn, Win)
        gV, gW, gI = Vt.grad.cpu().numpy().astype(np.float64), Wt.grad.cpu().numpy().astype(np.float64), Wit.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(gV).all() and np.isfinite(gW).all() and np.isfinite(gI).all()
        assert (gV[3] == 0).all() and (shared or ((gW[3] == 0).all() and (gI[3] == 0).all()))
        want_W, want_I, bar_W, bar_I = np.zeros_like(gW), np.zeros_like(gI), np.zeros_like(gW), np.zeros_like(gI)
        for b in range(3):
            r, a = refs[b], abs(gb[b])
            assert np.abs(gV[b] - gb[b] * r[0]).max() <= 2e-5 * a, (shared, b)
            if shared:
                want_W += gb[b] * r[1]
                want_I += gb[b] * r[2]
                bar_W += a * (1e-4 * r[1] + 1e-6 * lens[b])
                bar_I += a * (1e-4 * r[2] + 1e-6)
            else:
                want_W[b], want_I[b] = gb[b] * r[1], gb[b] * r[2]
                bar_W[b], bar_I[b] = a * (1e-4 * r[1] + 1e-6 * lens[b]), a * (1e-4 * r[2] + 1e-6)
        assert (np.abs(gW - want_W) <= bar_W + 1e-7 * np.abs(want_W)).all(), shared  # (+ the float32 product and sum over b)
        assert (np.abs(gI - want_I) <= bar_I + 1e-7 * np.abs(want_I)).all(), shared
    # a gradient that arrives for the dead utterance -- even a NaN -- reaches nothing
    Vt = torch.from_numpy(V).cuda().requires_grad_(True)
    Wt = torch.from_numpy(W).cuda().requires_grad_(True)
    ttl = mm.graph_loglik(Vt, bf, Wt, None, lt)
    ttl.backward(torch.tensor([1.0, 1.0, 1.0, float("nan")], device="cuda"))
    assert torch.isfinite(Vt.grad).all() and torch.isfinite(Wt.grad).all() and (Vt.grad[3] == 0).all() and (Wt.grad[3] == 0).all()
    # without a gradient to compute, only ttl is
    with torch.no_grad():
        t2 = mm.graph_loglik(torch.from_numpy(V).cuda(), bf, torch.from_numpy(W).cuda(), None, lt)
    assert torch.equal(t2, ttl.detach())


def test_em_on_a_dense_ergodic_hmm_without_recompiling(mm, wl, torch):
    """Five EM iterations through weightedposteriors + reestimate on ONE batch: the total log-likelihood never drops by more than the
    existing test's 1e-3, and the final weights equal those of the loop that compiles a fresh FSM and batch per iteration."""
    g = wl.dense_ergodic(64)
    B, N = 6, 80
    V = np.random.default_rng(9).standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.array([80, 75, 60, 80, 33, 50], dtype=np.int32)
    f = wl.to_fsm(mm, g)
    sm = mm.statemap(g.state2pdf, g.P)
    bf = mm.batch(*([mm.compile(f, sm)] * B))
    handle = bf._h.value
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    W, last = None, -np.inf
    for it in range(5):
        _, c, ttl = bf.weightedposteriors(Vt, None if W is None else torch.from_numpy(W).cuda(), None, lt, want_gamma=False)
        total = float(ttl.double().sum())
        assert total >= last - 1e-3, (it, total, last)
        last = total
        W, _ = mm.reestimate(f, c.double().sum(0).cpu().numpy())
    assert bf._h.value == handle
    # the recompile loop of tests/test_gpu_arcposteriors.py::test_em_on_a_dense_ergodic_hmm
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    phony = (i == fs) & (j == fs)
    f2 = f
    for it in range(5):
        c, _ = mm.batch(*([mm.compile(f2, sm)] * B)).arcposteriors(V, lens)
        cs = c[:, : f.nnz].astype(np.float64).sum(axis=0)
        tot = np.zeros(fs + 1)
        np.add.at(tot, i[~phony], cs[~phony])
        w = np.where(phony, 0.0, np.log(np.maximum(cs, 1e-30) / np.maximum(tot[i], 1e-30)))
        f2 = wl.to_fsm(mm, g)
        f2.nzval = w.astype(np.float32)
    assert np.abs(W.astype(np.float64) - w).max() <= 1e-4, np.abs(W.astype(np.float64) - w).max()


def test_error_codes(mm, wl, torch):
    """On a device: a tropical batch (-4), strides below the largest FSM (-2), stride 0 on distinct handles (-1), all outputs NULL
    (-1), g strides that cannot hold the batch (-2); with everything in order 0."""
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N = 10
    f = wl.to_fsm(mm, g)
    sm = mm.statemap(g.state2pdf, g.P)
    V = torch.zeros((2, N, g.P), device="cuda")
    buf = torch.zeros((2, 4000), device="cuda")  # (weights: all 0)
    gam, outb, tt = torch.zeros((2, N, g.P), device="cuda"), torch.zeros((2, 4000), device="cuda"), torch.zeros(2, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_init = len(f.alpha_idx)

    def call(h, W=None, wsb=0, Wi=None, wisb=0, gamma=None, gs=(0, 0, 0), counts=None, csb=0, init=None, isb=0, ttl=None):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return lib.mm_weightedposteriors_f32(h, V.data_ptr(), N * g.P, g.P, None, N, p(W), wsb, p(Wi), wisb, p(gamma), gs[0], gs[1], gs[2], p(counts), csb, p(init), isb, p(ttl), st)

    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), sm)] * 2))
    assert call(tb._h, ttl=tt) == -4 and b"log" in lib.mm_last_error()
    lb = mm.batch(*([mm.compile(f, sm)] * 2))
    assert call(lb._h) == -1 and b"all NULL" in lib.mm_last_error()
    assert call(lb._h, W=buf, wsb=f.nnz - 1, ttl=tt) == -2 and b"w_stride_b" in lib.mm_last_error()
    assert call(lb._h, Wi=buf, wisb=n_init - 1, ttl=tt) == (-2 if n_init > 1 else 0)
    assert call(lb._h, counts=outb, csb=f.nnz - 1) == -2 and b"c_stride_b" in lib.mm_last_error()
    assert call(lb._h, init=outb, isb=n_init - 1) == -2 and b"i_stride_b" in lib.mm_last_error()
    assert call(lb._h, gamma=gam, gs=(N * g.P - 1, g.P, 1)) == -2 and b"g strides" in lib.mm_last_error()
    db = mm.batch(mm.compile(f, sm), mm.compile(wl.to_fsm(mm, g), sm))
    assert call(db._h, W=buf, wsb=0, ttl=tt) == -1 and b"same FSM" in lib.mm_last_error()
    assert call(db._h, W=buf, wsb=f.nnz, ttl=tt) == 0
    assert call(lb._h, W=buf, wsb=0, Wi=buf, wisb=0, gamma=gam, gs=(N * g.P, g.P, 1), counts=outb, csb=4000, ttl=tt) == 0
    torch.cuda.synchronize()
