"""Forward filtering posteriors with a carried state (mm_filterposteriors_f32) without a GPU: the bindings of the new entry, the
argument checks that need no device, and the float64 reference of tests/filter_reference.py -- the header's definition -- against
brute-force enumeration, against the existing oracle's alpha-recursion and log Z, and against the identities the definition
implies: exact chunking, causality, the uniform-final-weights identity, the level shift, the dead-frame and len = 0 conventions."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np

import arc_reference as ar
import filter_reference as fr
import graphs
from test_gpu_parity import check_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_filterposteriors_f32" in mm.SYMBOLS
    assert lib.mm_filterposteriors_f32.argtypes is not None and len(lib.mm_filterposteriors_f32.argtypes) == 16
    assert callable(mm.filterposteriors) and hasattr(mm.BatchedFSM, "filterposteriors")
    assert hasattr(mm, "ForwardFilter") and all(hasattr(mm.ForwardFilter, k) for k in ("push", "logz", "reset"))
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_filterposteriors_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_filterposteriors_f32, LIB\)", src) and re.search(r"function filterposteriors\(", src)


def test_error_codes_that_need_no_device(mm):
    """What the arguments alone show is refused ahead of the batch: all outputs NULL (-1), i_stride_b < N (-2), f strides that
    cannot even hold the N frames (-2); with those in order the NULL batch is what is refused (-1)."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(state_out=None, filt=None, fs=(0, 0, 0), incr=None, isb=0, ttl=None, N=8):
        return lib.mm_filterposteriors_f32(None, p, 8, 1, None, N, None, state_out, filt, fs[0], fs[1], fs[2], incr, isb, ttl, None)

    assert call() == -1 and b"all NULL" in lib.mm_last_error()
    assert call(incr=p, isb=7) == -2 and b"i_stride_b" in lib.mm_last_error()
    assert call(filt=p, fs=(64, 0, 1)) == -2 and b"f strides" in lib.mm_last_error()
    assert call(filt=p, fs=(8, 1, 1), incr=p, isb=8) == -1 and b"NULL batch" in lib.mm_last_error()
    assert call(ttl=p) == -1 and b"NULL batch" in lib.mm_last_error()


def _uniform_final(g, w=-1.25):
    """g with the same final weight on every real state."""
    return dataclasses.replace(g, name=g.name + "_uf", final_idx=np.arange(g.S), final_w=np.full(g.S, w))


def _oracle(o, oc, g, V, L, N):
    """gamma [N, P], log Z and the un-normalised alpha [S + 1, N + 1] (natural log) of the C oracle in float64."""
    gam, ttl, A, _ = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, ar.expand_log(V, L, N), dtype=np.float64, want_ab=True)
    gam = np.nan_to_num(gam.T.copy(), nan=0.0)
    gam[L:] = 0
    return gam, (float(ttl) if np.isfinite(ttl) else -np.inf), A


def _graphs(wl):
    return [wl.l2r_hmm(3), wl.random_fsm(6, 3, mean_deg=2.0, seed=4), wl.random_fsm(40, 6, 3.0, seed=1), wl.lfmmi_denominator(300, 20)]


def test_reference_against_path_enumeration(wl):
    rng = np.random.default_rng(41)
    for g, L in ((wl.l2r_hmm(3), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 6), (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), 4)):
        V = rng.standard_normal((6, g.P))
        for state_in in (None, np.log(rng.random(g.S + 1))):
            filt, incr, ttl, so = fr.reference(g, V, L, 6, state_in)
            f_e, i_e, so_e = fr.enumerate_prefixes(g, V, L, state_in)
            assert np.abs(filt[:L] - f_e).max() <= 1e-10 and (filt[L:] == 0).all(), g.name
            assert np.abs(incr[:L] - i_e).max() <= 1e-10 and (incr[L:] == 0).all(), g.name
            m = np.isfinite(so_e)
            assert (np.isneginf(so) == ~m).all() and np.abs(so[m] - so_e[m]).max() <= 1e-10, g.name
            assert abs(ttl - (i_e.sum() + so_e[g.S])) <= 1e-10, g.name


def test_reference_against_the_oracle(wl, oracle):
    """filt = the oracle's alpha-recursion normalised per frame and summed per pdf; sum incr + state_out(final) = its log Z."""
    o, oc = oracle
    rng = np.random.default_rng(42)
    for g in _graphs(wl):
        N, L = 25, 21
        V = rng.standard_normal((N, g.P))
        filt, incr, ttl, so = fr.reference(g, V, L, N)
        _, z, A = _oracle(o, oc, g, V, L, N)
        s2p = np.asarray(g.state2pdf)
        l = ar._lse(A[: g.S, :L], axis=0)  # l_n
        ref = np.zeros((N, g.P))
        for n in range(L):
            ref[n] = np.bincount(s2p, weights=np.exp(A[: g.S, n] - l[n]), minlength=g.P)
        assert np.abs(filt - ref).max() <= 1e-10, (g.name, np.abs(filt - ref).max())
        assert np.abs(incr[:L] - np.diff(np.concatenate([[0.0], l]))).max() <= 1e-10, g.name
        assert abs(incr.sum() + so[g.S] - z) <= 1e-10 and abs(ttl - z) <= 1e-10, (g.name, ttl, z)
        assert abs(so[g.S] - (A[g.S, L] - l[L - 1])) <= 1e-10
        assert np.allclose(filt[:L].sum(-1), 1.0, atol=1e-12)


def test_chunk_concatenation_is_the_whole(wl):
    rng = np.random.default_rng(43)
    for g in _graphs(wl):
        N = 25
        V = rng.standard_normal((N, g.P))
        filt, incr, ttl, so = fr.reference(g, V, N, N)
        for cut in ((10, 15), (1, 24), (24, 1)):
            f1, i1, _, s1 = fr.reference(g, V[: cut[0]], cut[0], cut[0])
            f2, i2, _, s2 = fr.reference(g, V[cut[0] :], cut[1], cut[1], s1)
            assert np.abs(np.concatenate([f1, f2]) - filt).max() <= 1e-12, (g.name, cut)
            assert np.abs(np.concatenate([i1, i2]) - incr).max() <= 1e-12, (g.name, cut)
            m = np.isfinite(so)
            assert (np.isneginf(s2) == ~m).all() and np.abs(s2[m] - so[m]).max() <= 1e-12
            assert abs(i1.sum() + i2.sum() + s2[g.S] - ttl) <= 1e-12 * max(1.0, abs(ttl)), (g.name, cut)


def test_causality_is_bit_exact(wl):
    rng = np.random.default_rng(44)
    for g in _graphs(wl):
        V = rng.standard_normal((25, g.P))
        V2 = V.copy()
        V2[15:] = rng.standard_normal((10, g.P))
        a, b = fr.reference(g, V, 25, 25), fr.reference(g, V2, 25, 25)
        assert np.array_equal(a[0][:15], b[0][:15]) and np.array_equal(a[1][:15], b[1][:15]), g.name
        assert not np.array_equal(a[0][15:], b[0][15:])


def test_uniform_final_weights_identity(wl, oracle):
    """Final weights equal on every real state: filt(len) is the smoothing posterior gamma(len).  Other graphs: it is not."""
    o, oc = oracle
    rng = np.random.default_rng(45)
    for g0 in (wl.random_fsm(6, 3, mean_deg=2.0, seed=4), wl.random_fsm(40, 6, 3.0, seed=1)):
        N, L = 12, 10
        V = rng.standard_normal((N, g0.P))
        g = _uniform_final(g0)
        filt = fr.reference(g, V, L, N)[0]
        gam = _oracle(o, oc, g, V, L, N)[0]
        assert np.abs(filt[L - 1] - gam[L - 1]).max() <= 1e-10, g.name
        assert np.abs(filt[: L - 1] - gam[: L - 1]).max() > 1e-3
        filt0 = fr.reference(g0, V, L, N)[0]
        gam0 = _oracle(o, oc, g0, V, L, N)[0]
        assert np.abs(filt0[L - 1] - gam0[L - 1]).max() > 1e-3, g0.name


def test_level_shift(wl):
    rng = np.random.default_rng(46)
    for g in _graphs(wl):
        V = rng.standard_normal((20, g.P))
        c = rng.standard_normal(20) * 30
        a, b = fr.reference(g, V, 17, 20), fr.reference(g, V + c[:, None], 17, 20)
        assert np.abs(a[0] - b[0]).max() <= 1e-12, g.name
        assert np.abs(b[1][:17] - a[1][:17] - c[:17]).max() <= 1e-11 and (b[1][17:] == 0).all(), g.name
        m = np.isfinite(a[3])
        assert np.abs(a[3][m] - b[3][m]).max() <= 1e-11 and abs(b[2] - a[2] - c[:17].sum()) <= 1e-10


def test_dead_frame_and_empty_conventions(wl):
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    rng = np.random.default_rng(47)
    V = rng.standard_normal((10, g.P))
    alive = fr.reference(g, V, 10, 10)
    Vd = V.copy()
    Vd[4, :] = -np.inf
    filt, incr, ttl, so = fr.reference(g, Vd, 9, 10)
    assert np.array_equal(filt[:4], alive[0][:4]) and np.array_equal(incr[:4], alive[1][:4])
    assert (filt[4:] == 0).all() and np.isneginf(incr[4:9]).all() and incr[9] == 0
    assert np.isneginf(ttl) and np.isneginf(so).all()
    assert not any(np.isnan(x).any() for x in (filt, incr, so))
    # a start vector without a live state: dead from the first frame
    filt, incr, ttl, so = fr.reference(g, V, 10, 10, np.full(g.S + 1, -np.inf))
    assert (filt == 0).all() and np.isneginf(incr).all() and np.isneginf(ttl) and np.isneginf(so).all()
    # len = 0: the state passes through, its final entry included; NULL stands for ln alpha_hat
    st = np.log(rng.random(g.S + 1))
    filt, incr, ttl, so = fr.reference(g, V, 0, 10, st)
    assert (filt == 0).all() and (incr == 0).all() and np.isneginf(ttl) and np.array_equal(so, st)
    so0 = fr.reference(g, V, 0, 10)[3]
    assert np.array_equal(so0, fr.start_vector(g)) and np.isneginf(so0[g.S])
    # ... and that vector given back as state_in is the start NULL stands for
    a, b = fr.reference(g, V, 10, 10), fr.reference(g, V, 10, 10, so0)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2]


def small_gpu_inputs(wl):
    """The small inputs of tests/test_gpu_filterposteriors.py the float32 mode is run on: (graph, V [N, P] float32, length)."""
    out = []
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    V = np.random.default_rng(0).standard_normal((6, 30, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf
    out += [(g, V[0], 30), (g, V[1], 25), (g, V[2], 1)]
    gs = [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    V = np.random.default_rng(5).standard_normal((4, 40, 5)).astype(np.float32)
    out += [(g, V[b], L) for b, (g, L) in enumerate(zip(gs, (40, 33, 20, 38)))]
    g = wl.lfmmi_denominator(600, 40, seed=5)
    V = np.random.default_rng(1).standard_normal((4, 150, g.P)).astype(np.float32)
    out += [(g, V[0], 150), (g, V[3], 33)]
    return out


def check_against_reference(filt, incr, ttl, so, ref, L):
    """One utterance against its float64 reference under the project's bars; dead and empty utterances by their exact conventions.
    Returns the worst error over its bar of (filt, incr / ttl, state_out)."""
    f_ref, i_ref, t_ref, s_ref = ref
    N = f_ref.shape[0]
    filt, incr, so = np.asarray(filt, dtype=np.float64), np.asarray(incr, dtype=np.float64), np.asarray(so, dtype=np.float64)
    assert not (np.isnan(filt).any() or np.isnan(incr).any() or np.isnan(so).any() or np.isnan(ttl))
    assert (incr[L:] == 0).all() and (filt[L:] == 0).all()
    dead = np.flatnonzero(np.isneginf(i_ref[:L]))
    d = int(dead[0]) if dead.size else L  # the frames before d are alive
    assert (filt[d:L] == 0).all() and np.isneginf(incr[d:L]).all()
    wf = check_gamma(filt[None, :d], f_ref[None, :d], [d]) if d else 0.0
    tol = 1e-4 + 1e-5 * np.abs(i_ref[:d])
    assert (np.abs(incr[:d] - i_ref[:d]) <= tol).all(), np.abs(incr[:d] - i_ref[:d]).max()
    wi = float(np.max(np.abs(incr[:d] - i_ref[:d]) / tol)) if d else 0.0
    if np.isfinite(t_ref):
        assert np.isclose(ttl, t_ref, rtol=1e-5, atol=1e-4), (ttl, t_ref)
        wi = max(wi, abs(ttl - t_ref) / (1e-4 + 1e-5 * abs(t_ref)))
    else:
        assert np.isneginf(ttl)
    if L == 0:
        m = np.isfinite(s_ref)
        assert (np.isneginf(so) == ~m).all()
    m = s_ref > np.log(1e-30)
    assert (np.isneginf(so) == np.isneginf(s_ref)).all()
    ws = 0.0
    if m.any():
        e = np.abs(so[m] - s_ref[m]) / (1e-4 * np.maximum(np.abs(s_ref[m]), 1.0))
        assert (e <= 1.0).all(), e.max()
        ws = float(e.max())
    return wf, wi, ws


def test_float32_mode_within_the_bars(wl):
    """The recursion carried in float32 against float64 on the GPU tests' small inputs: within the bars the kernel is held to."""
    worst = np.zeros(3)
    for g, V, L in small_gpu_inputs(wl):
        V = V.astype(np.float64)
        N = V.shape[0]
        ref = fr.reference(g, V, L, N)
        f32 = fr.reference(g, V, L, N, dtype=np.float32)
        worst = np.maximum(worst, check_against_reference(f32[0], f32[1], f32[2], f32[3], ref, L))
    print(f"float32 recursion: worst error over its bar: filt {worst[0]:.3g}, incr / ttl {worst[1]:.3g}, state_out {worst[2]:.3g}")
    assert (worst <= 1.0).all()
