"""Test helper: float64 reference of the posteriors with per-frame arc-class scores (include/markovmodels_amd.h,
mm_scoredposteriors_f32).  It does not go through the C oracle, which cannot take time-varying weights: a log-domain
forward-backward in NumPy over the entry list (i, j, w) of arc_reference.fsm_entries, every entry k scored at transition t by
U[t, cls[k]] (no score for class -1, for the phony self-loop and for t >= L).  Plus log Z alone for central differences, and
brute-force enumeration for tiny graphs."""
import itertools

import numpy as np

import arc_reference as ar
import arcclass_reference as acr
from weighted_reference import _seg_lse


def entry_scores(f, cls, U, L, N):
    """s [nnz, N]: what entry k adds to its weight at transition t."""
    i, j, _ = ar.fsm_entries(f)
    cls = np.asarray(cls, dtype=np.int64)
    s = np.zeros((i.size, N))
    if U is None:
        return s
    U = np.asarray(U, dtype=np.float64)
    fs = f.colptr.size - 2
    scored = (cls >= 0) & ~((i == fs) & (j == fs))
    T = min(L, N)
    s[scored, :T] = U[:T, cls[scored]].T
    return s


def _setup(g, f, cls, U, V, L, N):
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[ar._s2p_full(g)]  # [S1, N + 1]
    return i, j, w, S1, a, lhs, entry_scores(f, cls, U, L, N)


def log_z(g, f, cls, U, V, L, N):
    """log Z(U) alone (the forward recursion): what the central differences perturb."""
    i, j, w, S1, a, lhs, s = _setup(g, f, cls, U, V, L, N)
    with np.errstate(invalid="ignore"):
        x = a + lhs[:, 0]
        for n in range(N):
            x = _seg_lse(x[i] + w + s[:, n], j, S1) + lhs[:, n + 1]
        return float(ar._lse(x))


def reference(g, f, cls, C, U, V, L, N):
    """gamma [N, P], xi [C, N], log Z and the mask of xi's structural values (exact 0 or 1: empty classes, frames >= L, a class
    whose score is -inf at the frame, no path) of one utterance: cls [nnz] in f's CSC entry order, U [>= L, C] or None, V [>= L, P]."""
    cls = np.asarray(cls, dtype=np.int64)
    i, j, w, S1, a, lhs, s = _setup(g, f, cls, U, V, L, N)
    P = g.P
    A = np.full((S1, N + 1), -np.inf)
    Bm = np.full((S1, N + 1), -np.inf)
    with np.errstate(invalid="ignore"):
        A[:, 0] = a + lhs[:, 0]
        for n in range(N):
            A[:, n + 1] = _seg_lse(A[i, n] + w + s[:, n], j, S1) + lhs[:, n + 1]
        Bm[:, N] = 0.0
        for n in range(N - 1, -1, -1):
            Bm[:, n] = _seg_lse(w + s[:, n] + lhs[j, n + 1] + Bm[j, n + 1], i, S1)
        logZ = float(ar._lse(A[:, 0] + Bm[:, 0]))
    gamma = np.zeros((N, P))
    xi = np.zeros((C, N))
    exact = np.zeros((C, N), dtype=bool)
    if not np.isfinite(logZ):
        exact[:] = True
        return gamma, xi, -np.inf, exact
    s2p = ar._s2p_full(g)
    with np.errstate(invalid="ignore"):
        post = np.exp(A + Bm - logZ)
        post = np.where(np.isfinite(post), post, 0.0)
        for n in range(min(L, N)):
            gamma[n] = np.bincount(s2p, weights=post[:, n], minlength=P + 1)[:P]
        t = A[i, :N] + w[:, None] + s + lhs[j, 1 : N + 1] + Bm[j, 1 : N + 1] - logZ  # [nnz, N]
        t = np.where(np.isnan(t), -np.inf, t)
    for c in range(C):
        m = cls == c
        if m.any():
            xi[c] = np.exp(ar._lse(t[m], axis=0))
        else:
            exact[c] = True
    if U is not None:
        T = min(L, N)
        exact[:, :T] |= np.isneginf(np.asarray(U, dtype=np.float64)[:T].T)
    acr.frame_rule(xi, exact, cls, f, L)
    return gamma, xi, logZ, exact


def enumerate_paths(g, f, cls, C, U, V, L, N):
    """gamma [N, P], xi [C, N] and log Z by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only); parallel
    entries between two states are scored one by one and share the pair's posterior in proportion to their scored weights."""
    cls = np.asarray(cls, dtype=np.int64)
    i, j, w, S1, a, lhs, s = _setup(g, f, cls, U, V, L, N)
    P = g.P
    Tt = np.full((N, S1, S1), -np.inf)
    for n in range(N):
        np.logaddexp.at(Tt[n], (i, j), w + s[:, n])
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    with np.errstate(invalid="ignore"):
        lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
        for n in range(N):
            lw = lw + Tt[n][paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
    lw = np.where(np.isnan(lw), -np.inf, lw)
    logZ = float(ar._lse(lw))
    gamma = np.zeros((N, P))
    xi = np.zeros((C, N))
    if not np.isfinite(logZ):
        return gamma, xi, -np.inf
    p = np.exp(lw - logZ)
    s2p = ar._s2p_full(g)
    for n in range(min(L, N)):
        gamma[n] = np.bincount(s2p[paths[:, n]], weights=p, minlength=P + 1)[:P]
    for n in range(N):
        pair = np.zeros((S1, S1))
        np.add.at(pair, (paths[:, n], paths[:, n + 1]), p)
        for k in range(i.size):
            if cls[k] >= 0 and pair[i[k], j[k]] > 0 and np.isfinite(w[k] + s[k, n]):
                xi[cls[k], n] += pair[i[k], j[k]] * np.exp(w[k] + s[k, n] - Tt[n][i[k], j[k]])
    return gamma, xi, logZ
