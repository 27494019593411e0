"""Test helper: float64 reference values of the per-frame arc-class posteriors (include/markovmodels_amd.h,
mm_arcclassposteriors_f32), from the C oracle's alpha / beta in log space on the pattern of arc_reference.reference, and by
enumerating every path of a tiny graph."""
import itertools

import numpy as np

import arc_reference as ar
import graphs


def frame_rule(xi, exact, cls, f, L):
    """Frames >= L of xi [C, N]: only the phony self-loop is alive -- its class, if it has one, exactly 1, every other exactly 0."""
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    xi[:, L:] = 0.0
    exact[:, L:] = True
    k = np.flatnonzero((i == fs) & (j == fs))
    if k.size and cls[k[0]] >= 0:
        xi[cls[k[0]], L:] = 1.0


def reference(o, oc, g, f, cls, C, V, L, N, want_gamma=False):
    """xi [C, N], log Z and the mask of the values that are structural (exact 0 or 1: empty classes, frames >= L, no path) of
    one utterance: cls [nnz] class ids in f's CSC entry order (-1: not counted), V [>= L, P] log-likelihoods, length L, N
    frames.  Per frame the terms A[i, t] + w + lhs[j, t+1] + B[j, t+1] - log Z of a class go through one log-sum-exp.
    want_gamma: also the state-map posteriors gamma [P + 1, N + 1] of the same alpha / beta."""
    cls = np.asarray(cls, dtype=np.int64)
    Vhat = ar.expand_log(V, L, N)
    _, _, A, Bm = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64, want_ab=True)
    i, j, w = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    lhs = Vhat[s2p]
    with np.errstate(invalid="ignore"):
        logZ = ar._lse(A[:, 0] + Bm[:, 0])
    xi = np.zeros((C, N))
    exact = np.zeros((C, N), dtype=bool)
    gamma = np.zeros((g.P + 1, N + 1))
    if not np.isfinite(logZ):
        exact[:] = True
        return (xi, -np.inf, exact, gamma) if want_gamma else (xi, -np.inf, exact)
    with np.errstate(invalid="ignore"):
        t = A[i, :N] + w[:, None] + lhs[j, 1 : N + 1] + Bm[j, 1 : N + 1] - logZ  # [nnz, N]
        t = np.where(np.isnan(t), -np.inf, t)
    for c in range(C):
        m = cls == c
        if m.any():
            xi[c] = np.exp(ar._lse(t[m], axis=0))
        else:
            exact[c] = True
    frame_rule(xi, exact, cls, f, L)
    if want_gamma:
        with np.errstate(invalid="ignore"):
            sp = np.exp(np.where(np.isnan(A + Bm), -np.inf, A + Bm) - logZ)  # [S1, N + 1]
        np.add.at(gamma, s2p, sp)
        return xi, float(logZ), exact, gamma
    return xi, float(logZ), exact


def enumerate_paths(g, f, cls, C, V, L, N):
    """xi [C, N] and log Z by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only)."""
    cls = np.asarray(cls, dtype=np.int64)
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    T = np.full((S1, S1), -np.inf)
    T[i, j] = w
    pair_cls = np.full((S1, S1), -1, dtype=np.int64)
    pair_cls[i, j] = cls
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[ar._s2p_full(g)]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
    for n in range(N):
        lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
    logZ = ar._lse(lw)
    xi = np.zeros((C, N))
    if not np.isfinite(logZ):
        return xi, -np.inf
    p = np.exp(lw - logZ)
    for n in range(N):
        pc = pair_cls[paths[:, n], paths[:, n + 1]]
        for c in range(C):
            xi[c, n] = np.sum(p[pc == c])
    return xi, float(logZ)


def check(xi, ttl, xi_ref, logz_ref, exact=None):
    """The accuracy bar of the arc-class posteriors against a float64 reference (one utterance, xi [C, N]).  Per value
    |d| <= 1e-4 xi_ref + 1e-6 -- arc_reference.check's bar for ONE frame: its 1e-6 len absolute part is per frame here --, per
    frame |sum_c xi - sum_c xi_ref| <= 1e-4, exact values where the reference's are structural (`exact`), ttl as
    arc_reference.check.  Returns the measured worst error over its bar."""
    xi = np.asarray(xi, dtype=np.float64)
    assert xi.shape == xi_ref.shape, (xi.shape, xi_ref.shape)
    if not np.isfinite(logz_ref):
        assert (xi == 0).all() and np.isneginf(ttl)
        return 0.0
    assert np.isfinite(xi).all()
    if exact is not None:
        assert (xi[exact] == xi_ref[exact]).all(), "structural values must be exact"
    bar = 1e-4 * xi_ref + 1e-6
    err = np.abs(xi - xi_ref)
    assert (err <= bar).all(), (err.max(), np.unravel_index(int(np.argmax(err - bar)), err.shape))
    worst = float(np.max(err / bar))
    fs = np.abs(xi.sum(axis=0) - xi_ref.sum(axis=0))
    assert (fs <= 1e-4).all(), (fs.max(), int(np.argmax(fs)))
    worst = max(worst, float(fs.max() / 1e-4))
    assert np.isclose(ttl, logz_ref, rtol=1e-5, atol=1e-5 * max(1.0, abs(logz_ref)) + 1e-4), (ttl, logz_ref)
    return worst
