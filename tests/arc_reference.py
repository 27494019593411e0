"""Test helper: float64 reference values of the arc posteriors (include/markovmodels_amd.h, mm_arcposteriors_f32), from the C
oracle's alpha / beta in log space, and by enumerating every path of a tiny graph."""
import itertools

import numpy as np

import graphs


def fsm_entries(f):
    """The stored entries of a product FSM's T_hat in CSC data order: (source i, destination j, natural-log weight)."""
    S1 = f.colptr.size - 1
    j = np.repeat(np.arange(S1), np.diff(np.asarray(f.colptr)))
    return np.asarray(f.rowval, dtype=np.int64), j.astype(np.int64), np.asarray(f.nzval, dtype=np.float64)


def expand_log(V, L, N):
    """expand(V[:L]) over N frames: [(P+1), (N+1)] natural-log emissions, float64."""
    P = V.shape[1]
    out = np.full((P + 1, N + 1), -np.inf)
    out[:P, :L] = np.asarray(V, dtype=np.float64)[:L].T
    out[P, L:] = 0.0
    return out


def _lse(x, axis=None):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True)), axis=axis)


def _s2p_full(g):
    return np.concatenate([np.asarray(g.state2pdf, dtype=np.int64), [g.P]])


def reference(o, oc, g, f, V, L, N, chunk=64):
    """Arc counts [nnz] (entries in f's CSC order), initial-state counts [n_init] (f.alpha_idx order) and log Z of one
    utterance: V [>= L, P] log-likelihoods, length L, N frames.  From the C oracle's float64 alpha / beta (natural log,
    un-normalised), combined in log space frame chunk by frame chunk."""
    Vhat = expand_log(V, L, N)
    _, _, A, Bm = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64, want_ab=True)
    i, j, w = fsm_entries(f)
    lhs = Vhat[_s2p_full(g)]  # [S1, N+1]
    with np.errstate(invalid="ignore"):
        logZ = _lse(A[:, 0] + Bm[:, 0])
    counts = np.zeros(i.size)
    init = np.zeros(len(f.alpha_idx))
    if not np.isfinite(logZ):
        return counts, init, -np.inf
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        t = A[i, n0:n1] + w[:, None] + lhs[j, n0 + 1 : n1 + 1] + Bm[j, n0 + 1 : n1 + 1] - logZ
        counts += np.exp(_lse(t, axis=1))
    ai = np.asarray(f.alpha_idx, dtype=np.int64)
    init = np.exp(A[ai, 0] + Bm[ai, 0] - logZ)
    return counts, init, float(logZ)


def enumerate_paths(g, f, V, L, N):
    """The same three by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only)."""
    i, j, w = fsm_entries(f)
    S1 = f.colptr.size - 1
    T = np.full((S1, S1), -np.inf)
    T[i, j] = w
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = expand_log(V, L, N)[_s2p_full(g)]  # [S1, N+1]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))  # [n_paths, N+1]
    lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
    for n in range(N):
        lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
    logZ = _lse(lw)
    counts = np.zeros(i.size)
    init = np.zeros(len(f.alpha_idx))
    if not np.isfinite(logZ):
        return counts, init, -np.inf
    p = np.exp(lw - logZ)
    for k in range(i.size):
        used = ((paths[:, :-1] == i[k]) & (paths[:, 1:] == j[k])).sum(axis=1)
        counts[k] = np.sum(p * used)
    for m, s in enumerate(np.asarray(f.alpha_idx)):
        init[m] = np.sum(p[paths[:, 0] == s])
    return counts, init, float(logZ)


def check(c, init, ttl, c_ref, init_ref, logz_ref, L, N):
    """The accuracy bar of the arc posteriors against a float64 reference (one utterance).  Returns the measured worst
    per-arc error over its bar."""
    c = np.asarray(c, dtype=np.float64)
    if not np.isfinite(logz_ref):
        assert (c == 0).all() and np.isneginf(ttl)
        if init is not None:
            assert (np.asarray(init) == 0).all()
        return 0.0
    err = np.abs(c - c_ref)
    assert (err <= 1e-4 * c_ref + 1e-6 * max(L, 1)).all(), (err.max(), int(np.argmax(err - 1e-4 * c_ref)))
    worst = float(np.max(err / (1e-4 * c_ref + 1e-6 * max(L, 1))))
    assert abs(c.sum() - N) <= 1e-4 * N, (c.sum(), N)
    assert np.isclose(ttl, logz_ref, rtol=1e-5, atol=1e-5 * max(1.0, abs(logz_ref)) + 1e-4), (ttl, logz_ref)
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        assert abs(init.sum() - 1.0) <= 1e-5, init.sum()
        assert (np.abs(init - init_ref) <= 1e-4 * init_ref + 1e-6).all()
    return worst
