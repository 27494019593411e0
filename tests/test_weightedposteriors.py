"""Posteriors with call-time arc weights (mm_weightedposteriors_f32) without a GPU: the bindings of the new entry, the argument checks
that need no device, and the float64 reference of tests/weighted_reference.py -- the header's definition -- against brute-force
enumeration, against the oracle and tests/arc_reference.py on a graph REBUILT with the substituted weights, against central
differences of log Z, and against the conventions the header states; `reestimate` and five EM iterations on the reference."""
import ctypes as C
import os
import re

import numpy as np

import arc_reference as ar
import graphs
import weighted_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds its 20 parameters, the host interface and the
    Julia wrapper are there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_weightedposteriors_f32" in mm.SYMBOLS
    assert lib.mm_weightedposteriors_f32.argtypes is not None and len(lib.mm_weightedposteriors_f32.argtypes) == 20
    assert callable(mm.weightedposteriors) and hasattr(mm.BatchedFSM, "weightedposteriors")
    assert callable(mm.graph_loglik) and callable(mm.reestimate)
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_weightedposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_weightedposteriors_f32, LIB\)", src) and re.search(r"function weightedposteriors\(", src)


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: all four outputs NULL (-1), a weight stride too small whatever
    the batch -- a negative one -- (-2), g strides that cannot even hold the N frames (-2); with those in order the NULL batch is
    what is refused (-1).  (A batch cannot be created without a device: the refusals that need the batch's own numbers -- a stride
    below max nnz, stride 0 on distinct handles, a tropical batch -- are in tests/test_gpu_weightedposteriors.py; they too come
    ahead of the first device call.)"""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(W=None, wsb=0, Wi=None, wisb=0, gamma=None, gs=(0, 0, 0), counts=None, init=None, ttl=None, N=8):
        return lib.mm_weightedposteriors_f32(None, p, 8, 1, None, N, W, wsb, Wi, wisb, gamma, gs[0], gs[1], gs[2], counts, 64, init, 64, ttl, None)

    assert call() == -1 and b"all NULL" in lib.mm_last_error()
    assert call(W=p, wsb=-1, ttl=p) == -2 and b"w_stride_b" in lib.mm_last_error()
    assert call(Wi=p, wisb=-3, ttl=p) == -2 and b"wi_stride_b" in lib.mm_last_error()
    assert call(gamma=p, gs=(64, 0, 1)) == -2 and b"g strides" in lib.mm_last_error()
    assert call(gamma=p, gs=(8, 1, 1)) == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(W=p, wsb=0, counts=p) == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(ttl=p) == -1 and b"NULL batch" in lib.mm_last_error()


def _tiny(wl):
    return [wl.l2r_hmm(3), wl.random_fsm(5, 3, mean_deg=2.0, seed=4), wl.random_fsm(4, 2, mean_deg=2.5, seed=9, n_init=3)]


def _noisy(rng, f, sigma=0.5):
    return np.asarray(f.nzval, dtype=np.float64) + sigma * rng.standard_normal(f.nnz), np.asarray(f.alpha_val, dtype=np.float64) + sigma * rng.standard_normal(len(f.alpha_idx))


def test_reference_against_path_enumeration(mm, wl):
    """Graphs of up to 5 states and up to 5 frames: gamma, counts, init and log Z, with the FSM's own and with substituted weights,
    an entry at -inf included."""
    rng = np.random.default_rng(71)
    for g in _tiny(wl):
        f = wl.to_fsm(mm, g)
        for N, L in ((5, 5), (4, 3), (3, 1)):
            V = rng.standard_normal((N, g.P))
            W, Wi = _noisy(rng, f)
            Wk = W.copy()
            Wk[0] = -np.inf
            for w, wi in ((None, None), (W, None), (W, Wi), (Wk, Wi)):
                got = wr.reference(f, g.state2pdf, g.P, V, L, N, w, wi)
                ref = wr.enumerate_paths(f, g.state2pdf, g.P, V, L, N, w, wi)
                what = (g.name, N, L, w is None, wi is None)
                assert np.isfinite(ref[3]) or w is Wk or L < 3, what  # (l2r3 needs three frames to reach its final state)
                for x, y in zip(got[:3], ref[:3]):
                    assert np.abs(x - y).max() <= 1e-10, what
                assert got[3] == ref[3] or abs(got[3] - ref[3]) <= 1e-10, what
                if np.isfinite(ref[3]):
                    assert np.allclose(got[0][:L].sum(-1), 1.0, atol=1e-12) and (got[0][L:] == 0).all()
                    assert abs(got[1].sum() - N) <= 1e-10 and abs(got[2].sum() - 1) <= 1e-10


def _cases(wl):
    return [(wl.l2r_hmm(3), 12, 9), (wl.random_fsm(40, 6, 3.0, seed=1), 30, 25), (wl.random_fsm(25, 4, 2.0, seed=3, n_init=4), 20, 20)]


def test_reference_against_the_oracle_on_a_rebuilt_graph(mm, wl, oracle):
    """gamma and log Z of the C oracle, counts and init of tests/arc_reference.py, all on the graph rebuilt with the call's weights."""
    o, oc = oracle
    rng = np.random.default_rng(72)
    for g, N, L in _cases(wl):
        f = wl.to_fsm(mm, g)
        V = rng.standard_normal((N, g.P))
        W, Wi = _noisy(rng, f)
        for w, wi in ((None, None), (W, Wi)):
            g2 = wr.rebuilt(g, f, w, wi)
            f2 = wl.to_fsm(mm, g2, dtype=np.float64)
            assert f2.nnz == f.nnz and (f2.rowval == f.rowval).all()
            gam, c, init, z = wr.reference(f, g.state2pdf, g.P, V, L, N, w, wi)
            g_o, t_o = oc.batch_shared(graphs.to_oracle(o, g2), g.state2pdf, g.P, V[None], np.array([L], dtype=np.int32), dtype=np.float64)
            assert np.abs(gam - g_o[0]).max() <= 1e-10 and abs(z - t_o[0]) <= 1e-10, (g.name, np.abs(gam - g_o[0]).max(), z, t_o[0])
            c_a, i_a, z_a = ar.reference(o, oc, g2, f2, V, L, N)
            assert np.abs(c - c_a).max() <= 1e-10 and np.abs(init - i_a).max() <= 1e-10 and abs(z - z_a) <= 1e-10, g.name


def test_gradient_by_central_differences(mm, wl):
    """counts = d log Z / d W, init = d log Z / d W_init: every entry, step 1e-5, agreement 1e-6."""
    rng = np.random.default_rng(73)
    h = 1e-5
    for g, N, L in _cases(wl)[:2]:
        f = wl.to_fsm(mm, g)
        V = rng.standard_normal((N, g.P))
        W, Wi = _noisy(rng, f)
        _, c, init, _ = wr.reference(f, g.state2pdf, g.P, V, L, N, W, Wi)
        i, j, _ = ar.fsm_entries(f)
        fs = f.colptr.size - 2
        for k in range(f.nnz):
            if i[k] == fs and j[k] == fs:
                continue  # (the phony self-loop is one(K) whatever W holds: no derivative to take)
            d = np.zeros(f.nnz)
            d[k] = h
            num = (wr.log_z(f, g.state2pdf, g.P, V, L, N, W + d, Wi) - wr.log_z(f, g.state2pdf, g.P, V, L, N, W - d, Wi)) / (2 * h)
            assert abs(num - c[k]) <= 1e-6, (g.name, k, num, c[k])
        for m in range(len(f.alpha_idx)):
            d = np.zeros(len(f.alpha_idx))
            d[m] = h
            num = (wr.log_z(f, g.state2pdf, g.P, V, L, N, W, Wi + d) - wr.log_z(f, g.state2pdf, g.P, V, L, N, W, Wi - d)) / (2 * h)
            assert abs(num - init[m]) <= 1e-6, (g.name, m, num, init[m])


def test_conventions(mm, wl):
    rng = np.random.default_rng(74)
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    f = wl.to_fsm(mm, g)
    N, L = 30, 25
    V = rng.standard_normal((N, g.P))
    i, j, w0 = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    own = wr.reference(f, g.state2pdf, g.P, V, L, N)
    # W = None is the FSM's own weights
    same = wr.reference(f, g.state2pdf, g.P, V, L, N, w0, np.asarray(f.alpha_val, dtype=np.float64))
    assert all(np.array_equal(x, y) for x, y in zip(own[:3], same[:3])) and own[3] == same[3]
    # -inf on an entry is the graph without it
    W, Wi = _noisy(rng, f)
    real = np.flatnonzero(j != fs)
    drop = real[[3, 17, 40]]
    Wk = W.copy()
    Wk[drop] = -np.inf
    got = wr.reference(f, g.state2pdf, g.P, V, L, N, Wk, Wi)
    g2 = wr.rebuilt(g, f, Wk, Wi)
    f2 = wl.to_fsm(mm, g2, dtype=np.float64)
    assert f2.nnz == f.nnz - 3
    ref = wr.reference(f2, g.state2pdf, g.P, V, L, N)
    keep = np.setdiff1d(np.arange(f.nnz), drop)
    assert (got[1][drop] == 0).all() and np.abs(got[1][keep] - ref[1]).max() <= 1e-10
    assert np.abs(got[0] - ref[0]).max() <= 1e-10 and np.abs(got[2] - ref[2]).max() <= 1e-10 and abs(got[3] - ref[3]) <= 1e-10
    # all final entries at -inf: everything 0, ttl = -inf
    Wd = W.copy()
    Wd[(j == fs) & (i != fs)] = -np.inf
    gam, c, init, z = wr.reference(f, g.state2pdf, g.P, V, L, N, Wd, Wi)
    assert np.isneginf(z) and (gam == 0).all() and (c == 0).all() and (init == 0).all()
    # a garbage value at the phony self-loop's index changes nothing
    Wg = W.copy()
    Wg[(i == fs) & (j == fs)] = 123.0
    a, b = wr.reference(f, g.state2pdf, g.P, V, L, N, W, Wi), wr.reference(f, g.state2pdf, g.P, V, L, N, Wg, Wi)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert abs(a[1][(i == fs) & (j == fs)][0] - (N - L)) <= 1e-10
    # len = 0: no path through the real states (every initial state is real)
    gam, c, init, z = wr.reference(f, g.state2pdf, g.P, V, 0, N, W, Wi)
    assert np.isneginf(z) and (gam == 0).all() and (c == 0).all() and (init == 0).all()
    # c on every final entry, or on every W_init entry: ttl + c, gamma and the counts unchanged
    for shift in (1.75, -0.4):
        Ws = W.copy()
        Ws[(j == fs) & (i != fs)] += shift
        for b in (wr.reference(f, g.state2pdf, g.P, V, L, N, Ws, Wi), wr.reference(f, g.state2pdf, g.P, V, L, N, W, Wi + shift)):
            assert abs(b[3] - a[3] - shift) <= 1e-10
            assert all(np.abs(x - y).max() <= 1e-10 for x, y in zip(a[:3], b[:3]))


def test_reestimate_and_em_on_the_reference(mm, wl):
    """Rows of exp(W) sum to 1 (the phony self-loop aside, which stays 0), exp(W_init) sums to 1; five EM iterations on the
    reference never lower the total log-likelihood."""
    rng = np.random.default_rng(75)
    g = wl.random_fsm(12, 4, 2.5, seed=5, n_init=3)
    f = wl.to_fsm(mm, g)
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    phony = (i == fs) & (j == fs)
    N = 14
    Vs = [rng.standard_normal((N, g.P)) for _ in range(4)]
    Ls = [14, 11, 7, 14]
    W, Wi = None, None
    last = -np.inf
    for it in range(5):
        res = [wr.reference(f, g.state2pdf, g.P, V, L, N, W, Wi) for V, L in zip(Vs, Ls)]
        total = sum(r[3] for r in res)
        assert np.isfinite(total) and total >= last - 1e-10, (it, total, last)
        last = total
        W, Wi = mm.reestimate(f, sum(r[1] for r in res), sum(r[2] for r in res))
        assert W.dtype == np.float32 and Wi.dtype == np.float32 and W[phony][0] == 0.0
        rows = np.bincount(i[~phony], weights=np.exp(W[~phony].astype(np.float64)), minlength=fs + 1)
        seen = np.bincount(i[~phony], minlength=fs + 1) > 0
        assert np.allclose(rows[seen], 1.0, atol=1e-5) and abs(np.exp(Wi.astype(np.float64)).sum() - 1) <= 1e-5
    W2, none = mm.reestimate(f, res[0][1])
    assert none is None and W2.shape == (f.nnz,)
