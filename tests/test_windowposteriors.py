"""Fixed-lag smoothing posteriors (mm_windowposteriors_f32) without a GPU: the bindings of the new entry, the argument checks that
need no device, and the float64 reference of tests/window_reference.py -- the header's definition -- against brute-force
enumeration, against the existing oracle (closed: its gamma and log Z; open: its alpha with beta restarted from ones), against the
consequences the header states -- (b) the filter's last frame, increments and state, (c) exact re-windowing, (d) the level shift --
and the dead, len = 0 and c = 0 conventions; the float32 mode of the reference against the bars the kernels are held to; and a
NumPy model of streaming.FixedLagSmoother's bookkeeping against whole-prefix references."""
import ctypes as C
import os
import re

import numpy as np

import arc_reference as ar
import filter_reference as fr
import leaky_reference as lr
import window_reference as wr
from test_filterposteriors import _graphs, _oracle
from test_gpu_parity import check_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there.
    (The header's signature has 17 parameters: batch, V and its two strides, lens, N, state_in, closed, commit, state_out, lcommit,
    gamma and its three strides, ttl, stream.)"""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_windowposteriors_f32" in mm.SYMBOLS
    assert lib.mm_windowposteriors_f32.argtypes is not None and len(lib.mm_windowposteriors_f32.argtypes) == 17
    assert callable(mm.windowposteriors) and hasattr(mm.BatchedFSM, "windowposteriors")
    assert hasattr(mm, "FixedLagSmoother") and all(hasattr(mm.FixedLagSmoother, k) for k in ("push", "finish", "reset"))
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_windowposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_windowposteriors_f32, LIB\)", src) and re.search(r"function windowposteriors\(", src)


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: gamma NULL (-1), g strides that cannot even hold the N frames
    (-2); with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(gamma=None, gs=(0, 0, 0), N=8):
        return lib.mm_windowposteriors_f32(None, p, 8, 1, None, N, None, None, None, None, None, gamma, gs[0], gs[1], gs[2], None, None)

    assert call() == -1 and b"gamma is NULL" in lib.mm_last_error()
    assert call(gamma=p, gs=(64, 0, 1)) == -2 and b"g strides" in lib.mm_last_error()
    assert call(gamma=p, gs=(8, 1, 1)) == -1 and b"NULL batch" in lib.mm_last_error()


def _same(so, so_ref, tol):
    m = np.isfinite(so_ref)
    return bool((np.isneginf(so) == ~m).all() and (not m.any() or np.abs(so[m] - so_ref[m]).max() <= tol))


def test_reference_against_path_enumeration(wl):
    rng = np.random.default_rng(51)
    for g, L in ((wl.l2r_hmm(3), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 4)):
        V = rng.standard_normal((6, g.P))
        for state_in in (None, np.log(rng.random(g.S + 1))):
            for closed in (False, True):
                for commit in (None, 0, 2, L + 3):
                    gam, ttl, lc, so = wr.reference(g, V, L, 6, state_in, closed, commit)
                    g_e, t_e, lc_e, so_e = wr.enumerate_paths(g, V, L, state_in, closed, commit)
                    what = (g.name, L, state_in is None, closed, commit)
                    assert np.isfinite(t_e), what
                    assert np.abs(gam[:L] - g_e).max() <= 1e-10 and (gam[L:] == 0).all(), what
                    assert abs(ttl - t_e) <= 1e-10 and abs(lc - lc_e) <= 1e-10, what
                    assert _same(so, so_e, 1e-10), what
                    assert np.allclose(gam[:L].sum(-1), 1.0, atol=1e-12)


def _dense_open_backward(g, V, L):
    """ln b_n [S, L] of the open window by the definition, on the dense T of the real states."""
    S = g.S
    i, j, w, _ = lr.entries(g)
    T = np.full((S + 1, S + 1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    T = T[:S, :S]
    s2p = np.asarray(g.state2pdf)
    b = np.zeros((S, L))
    with np.errstate(divide="ignore"):
        for n in range(L - 2, -1, -1):
            b[:, n] = ar._lse(T + (V[n + 1, s2p] + b[:, n + 1])[None, :], axis=1)
    return b


def test_reference_against_the_oracle(wl, oracle):
    """Closed, from the FSM's own start: the oracle's gamma and log Z.  Open: the oracle's alpha with beta restarted from ones."""
    o, oc = oracle
    rng = np.random.default_rng(52)
    for g in _graphs(wl):
        N, L = 25, 21
        V = rng.standard_normal((N, g.P))
        gam_o, z, A = _oracle(o, oc, g, V, L, N)
        gam, ttl, lc, so = wr.reference(g, V, L, N, closed=True)
        assert np.abs(gam - gam_o).max() <= 1e-10 and abs(ttl - z) <= 1e-10, (g.name, np.abs(gam - gam_o).max(), ttl, z)
        gam, ttl, lc, so = wr.reference(g, V, L, N)
        s2p = np.asarray(g.state2pdf)
        lg = A[: g.S, :L] + _dense_open_backward(g, V, L)
        tot = ar._lse(lg, axis=0)
        ref = np.zeros((N, g.P))
        for n in range(L):
            ref[n] = np.bincount(s2p, weights=np.exp(lg[:, n] - tot[n]), minlength=g.P)
        assert np.abs(gam - ref).max() <= 1e-10, (g.name, np.abs(gam - ref).max())
        assert abs(ttl - ar._lse(A[: g.S, L - 1])) <= 1e-10 and np.abs(tot - ttl).max() <= 1e-9, g.name
        assert abs(lc - ttl) <= 1e-12  # commit = None: l_len


def test_open_window_ends_as_the_filter(wl):
    """(b): gamma(len) = filt(len), ttl = the sum of incr, and with c = len state_out is the filter's."""
    rng = np.random.default_rng(53)
    for g in _graphs(wl):
        N, L = 25, 21
        V = rng.standard_normal((N, g.P))
        for state_in in (None, np.log(rng.random(g.S + 1))):
            gam, ttl, lc, so = wr.reference(g, V, L, N, state_in)
            filt, incr, _, so_f = fr.reference(g, V, L, N, state_in)
            assert np.abs(gam[L - 1] - filt[L - 1]).max() <= 1e-10 and np.abs(gam[: L - 1] - filt[: L - 1]).max() > 1e-6, g.name
            assert abs(ttl - incr.sum()) <= 1e-10 and abs(lc - ttl) <= 1e-12 and _same(so, so_f, 1e-10), g.name
            # ... and state_out and lcommit at c are the filter's after c frames, whatever lies behind c
            for c in (1, 9):
                _, _, lc, so = wr.reference(g, V, L, N, state_in, closed=True, commit=c)
                _, i_c, _, so_c = fr.reference(g, V, c, N, state_in)
                assert abs(lc - i_c.sum()) <= 1e-10 and _same(so, so_c, 1e-10), (g.name, c)


def test_rewindowing_is_exact(wl):
    """(c): a second window over the frames behind the commit frame, from the first window's state_out."""
    rng = np.random.default_rng(54)
    for g in _graphs(wl):
        M = 25
        V = rng.standard_normal((M, g.P))
        for closed in (False, True):
            for state_in in (None, np.log(rng.random(g.S + 1))):
                for c in (1, 10, 24):
                    g1, t1, lc1, so1 = wr.reference(g, V, M, M, state_in, closed, c)
                    g2, t2, lc2, so2 = wr.reference(g, V[c:], M - c, M - c, so1, closed)
                    assert np.abs(g2 - g1[c:]).max() <= 1e-10, (g.name, closed, c)
                    assert abs(t2 - (t1 - lc1)) <= 1e-10 * max(1.0, abs(t1)), (g.name, closed, c, t2, t1, lc1)


def test_level_shift(wl):
    """(d): a constant per frame moves ttl by the constants' sum, lcommit by the sum up to c, and nothing else."""
    rng = np.random.default_rng(55)
    for g in _graphs(wl):
        V = rng.standard_normal((20, g.P))
        k = rng.standard_normal(20) * 30
        for closed in (False, True):
            a, b = wr.reference(g, V, 17, 20, None, closed, 11), wr.reference(g, V + k[:, None], 17, 20, None, closed, 11)
            assert np.abs(a[0] - b[0]).max() <= 1e-12, g.name
            assert abs(b[1] - a[1] - k[:17].sum()) <= 1e-10 and abs(b[2] - a[2] - k[:11].sum()) <= 1e-10
            assert _same(b[3], a[3], 1e-11)


def test_dead_empty_and_uncommitted_conventions(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    rng = np.random.default_rng(56)
    V = rng.standard_normal((10, g.P))
    Vd = V.copy()
    Vd[4, :] = -np.inf
    for closed in (False, True):
        # the mass dies at frame 4 (counted from 0): no gamma, no ttl; the prefix's state_out and lcommit while c <= 4
        alive = wr.reference(g, V, 9, 10, None, closed, 3)
        gam, ttl, lc, so = wr.reference(g, Vd, 9, 10, None, closed, 3)
        assert (gam == 0).all() and np.isneginf(ttl) and lc == alive[2] and np.array_equal(so, alive[3])
        gam, ttl, lc, so = wr.reference(g, Vd, 9, 10, None, closed, 4)
        assert np.isfinite(lc) and np.isfinite(so).any()
        for c in (5, 9, None):
            gam, ttl, lc, so = wr.reference(g, Vd, 9, 10, None, closed, c)
            assert (gam == 0).all() and np.isneginf(ttl) and np.isneginf(lc) and np.isneginf(so).all()
        assert not any(np.isnan(x).any() for x in (gam, so))
        # a start vector without a live state
        gam, ttl, lc, so = wr.reference(g, V, 10, 10, np.full(g.S + 1, -np.inf), closed)
        assert (gam == 0).all() and np.isneginf(ttl) and np.isneginf(lc) and np.isneginf(so).all()
        # len = 0 and c = 0: the start vector passes through, its final entry included; NULL stands for ln alpha_hat
        st = np.log(rng.random(g.S + 1))
        gam, ttl, lc, so = wr.reference(g, V, 0, 10, st, closed)
        assert (gam == 0).all() and np.isneginf(ttl) and lc == 0 and np.array_equal(so, st)
        assert np.array_equal(wr.reference(g, V, 0, 10, None, closed)[3], fr.start_vector(g))
        gam, ttl, lc, so = wr.reference(g, V, 10, 10, st, closed, 0)
        assert np.isfinite(ttl) and np.allclose(gam.sum(-1), 1.0) and lc == 0 and np.array_equal(so, st)
        gam, ttl, lc, so = wr.reference(g, V, 10, 10, None, closed, -3)
        assert lc == 0 and np.array_equal(so, fr.start_vector(g))
    # a closed window whose final weights accept none of the mass: alive in every frame, no total
    g = wl.l2r_hmm(3)
    V = rng.standard_normal((2, g.P))
    assert np.isneginf(wr.enumerate_paths(g, V, 2, None, True)[1])
    gam, ttl, lc, so = wr.reference(g, V, 2, 2, None, True)
    assert (gam == 0).all() and np.isneginf(ttl) and np.isfinite(lc) and np.isfinite(so).any()
    gam, ttl, lc2, so2 = wr.reference(g, V, 2, 2)
    assert np.allclose(gam.sum(-1), 1.0) and np.isfinite(ttl) and lc2 == lc and np.array_equal(so, so2)


# ---- the inputs of tests/test_gpu_windowposteriors.py (module level: the float32 mode below runs on the very same inputs)
def case_random40(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    N = 30
    lens = np.array([30, 25, 1, 0, 28, 30], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((6, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf  # a frame with -inf entries
    V[4, 14, :] = -np.inf  # utterance 4 dies mid-window, behind its commit frame
    closed = np.array([0, 1, 1, 0, 0, 1], dtype=np.int32)
    commit = np.array([0, 25, 40, 3, 9, 17], dtype=np.int32)  # 0, len, beyond len (clamped), beyond len 0, before the death, inside
    return [g] * 6, V, lens, closed, commit


def distinct_graphs(wl):
    return [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]


def case_distinct(wl):
    gs = distinct_graphs(wl)
    V = np.random.default_rng(5).standard_normal((4, 40, 5)).astype(np.float32)
    return gs, V, np.array([40, 33, 20, 38], dtype=np.int32), np.array([1, 0, 1, 0], dtype=np.int32), np.array([12, 33, 0, 37], dtype=np.int32)


def case_den600(wl):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    V = np.random.default_rng(1).standard_normal((4, 150, g.P)).astype(np.float32)
    return [g] * 4, V, np.array([150, 120, 150, 33], dtype=np.int32), np.array([0, 1, 1, 0], dtype=np.int32), np.array([100, 120, 1, 20], dtype=np.int32)


def references(case, state_in=None, dtype=np.float64):
    """The references of a case, one (gamma, ttl, lcommit, state_out) per utterance."""
    gs, V, lens, closed, commit = case
    return [wr.reference(gs[b], V[b].astype(np.float64), int(lens[b]), V.shape[1], state_in, bool(closed[b]) if closed is not None else False,
                         int(commit[b]) if commit is not None else None, dtype) for b in range(len(gs))]


def check_against_reference(gamma, ttl, lcommit, so, ref, L):
    """One utterance against its float64 reference under the project's bars -- gamma: check_gamma of tests/test_gpu_parity.py; ttl
    and lcommit: np.allclose(rtol=1e-5, atol=1e-4); state_out: the bar of test_filterposteriors.check_against_reference -- and a
    window without mass, an empty one and a dead prefix by their exact conventions.  Returns the worst error over its bar of
    (gamma, ttl / lcommit, state_out)."""
    g_ref, t_ref, l_ref, s_ref = ref
    gamma, so = np.asarray(gamma, dtype=np.float64), np.asarray(so, dtype=np.float64)
    assert not (np.isnan(gamma).any() or np.isnan(so).any() or np.isnan(ttl) or np.isnan(lcommit))
    assert (gamma[L:] == 0).all()
    wg = wt = ws = 0.0
    if np.isfinite(t_ref):
        wg = check_gamma(gamma[None], g_ref[None], [L])
        assert np.isclose(ttl, t_ref, rtol=1e-5, atol=1e-4), (ttl, t_ref)
        wt = abs(ttl - t_ref) / (1e-4 + 1e-5 * abs(t_ref))
    else:
        assert (gamma == 0).all() and np.isneginf(ttl), ttl
    if np.isfinite(l_ref):
        assert np.isclose(lcommit, l_ref, rtol=1e-5, atol=1e-4), (lcommit, l_ref)
        wt = max(wt, abs(lcommit - l_ref) / (1e-4 + 1e-5 * abs(l_ref)))
    else:
        assert np.isneginf(lcommit), lcommit
    assert (np.isneginf(so) == np.isneginf(s_ref)).all()
    m = s_ref > np.log(1e-30)
    if m.any():
        e = np.abs(so[m] - s_ref[m]) / (1e-4 * np.maximum(np.abs(s_ref[m]), 1.0))
        assert (e <= 1.0).all(), e.max()
        ws = float(e.max())
    return wg, wt, ws


def test_float32_mode_within_the_bars(wl):
    """The recursions carried in float32 against float64 on the GPU tests' inputs: below half of every bar the kernels are held to
    (were it more on an input, the input would have to change, not the bar)."""
    worst = np.zeros(3)
    for case in (case_random40(wl), case_distinct(wl), case_den600(wl)):
        lens = case[2]
        for b, (r64, r32) in enumerate(zip(references(case), references(case, dtype=np.float32))):
            worst = np.maximum(worst, check_against_reference(r32[0], r32[1], r32[2], r32[3], r64, int(lens[b])))
    print(f"float32 recursions: worst error over its bar: gamma {worst[0]:.3g}, ttl / lcommit {worst[1]:.3g}, state_out {worst[2]:.3g}")
    assert (worst <= 0.5).all()


class SmootherModel:
    """streaming.FixedLagSmoother's bookkeeping for one utterance in NumPy, on the reference."""

    def __init__(self, g, lag):
        self.g, self.lag = g, lag
        self.state, self.loglik, self.pending = None, 0.0, np.zeros((0, g.P))

    def push(self, chunk):
        win = np.concatenate([self.pending, chunk])
        n = win.shape[0]
        c = max(0, n - self.lag)
        if n == 0:
            return np.zeros((0, self.g.P))
        gam, _, lc, so = wr.reference(self.g, win, n, n, self.state, False, c)
        self.state, self.loglik, self.pending = so, self.loglik + lc, win[c:]
        return gam[:c]

    def finish(self):
        n = self.pending.shape[0]
        gam, ttl, _, _ = wr.reference(self.g, self.pending, n, max(n, 1), self.state, True)
        return gam[:n], self.loglik + ttl


def test_fixed_lag_bookkeeping(wl):
    """Every frame is emitted once, in order, with the open-window posterior given ALL frames pushed so far (not only lag of them);
    the frames finish emits have the smoothing posterior of the whole audio, and loglik + the closed ttl is its log Z."""
    rng = np.random.default_rng(57)
    for g in (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), wl.random_fsm(40, 6, 3.0, seed=1)):
        for lag, chunks in ((5, (1, 9, 3, 0, 12, 7)), (8, (3, 3, 1, 20)), (40, (10, 10))):
            T = sum(chunks)
            V = rng.standard_normal((T, g.P))
            whole = wr.reference(g, V, T, T, None, True)
            m = SmootherModel(g, lag)
            n0 = emitted = 0
            for ch in chunks:
                out = m.push(V[n0 : n0 + ch])
                n0 += ch
                assert out.shape[0] == max(0, n0 - lag) - emitted and m.pending.shape[0] == min(n0, lag)
                if out.shape[0]:
                    prefix = wr.reference(g, V, n0, n0)
                    assert np.abs(out - prefix[0][emitted : emitted + out.shape[0]]).max() <= 1e-10, (g.name, lag, n0)
                    assert abs(m.loglik - fr.reference(g, V, emitted + out.shape[0], T)[1].sum()) <= 1e-9
                emitted += out.shape[0]
            rest, logz = m.finish()
            assert emitted + rest.shape[0] == T
            assert np.abs(rest - whole[0][emitted:]).max() <= 1e-10 and abs(logz - whole[1]) <= 1e-9, (g.name, lag)
