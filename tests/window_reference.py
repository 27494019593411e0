"""Test helper: float64 reference of the fixed-lag smoothing posteriors (include/markovmodels_amd.h, mm_windowposteriors_f32) by the
header's definition -- the sparse extended system of leaky_reference.entries; the forward vector carried normalised by the maximum
of the frame before with the frame's largest emission in a float64 offset, the backward vector likewise, as the kernels carry
them --, a float32 mode of the same recursions (vectors and sums rounded to float32: what float32 arithmetic alone costs), and a
brute-force enumeration of every state sequence of a tiny graph for both end modes."""
import itertools

import numpy as np

import arc_reference as ar
import filter_reference as fr
import leaky_reference as lr


def _clamp_commit(commit, L):
    return L if commit is None else min(max(int(commit), 0), L)


def _start_copy(g, state_in):
    """What state_out holds when nothing is committed: the start vector as given (its final entry included)."""
    return np.asarray(state_in, dtype=np.float64).copy() if state_in is not None else fr.start_vector(g)


def reference(g, V, L, N, state_in=None, closed=False, commit=None, dtype=np.float64):
    """(gamma [N, P], ttl, lcommit, state_out [S + 1]) of one utterance: V [>= L, P] natural-log likelihoods, length L, N frames,
    state_in [S + 1] natural log or None, the end mode and the commit frame (None: L).  dtype = float32 rounds the vectors and
    every sum over them to float32."""
    dt = np.dtype(dtype).type
    S, S1, P = g.S, g.S + 1, g.P
    i, j, w, _ = lr.entries(g)
    s2p = ar._s2p_full(g)
    gamma = np.zeros((N, P))
    c = _clamp_commit(commit, L)
    if L == 0:
        return gamma, -np.inf, 0.0, _start_copy(g, state_in)
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        E = np.max(V[:L], axis=1)
    E = np.where(np.isfinite(E), E, 0.0)  # the frame's largest emission: in the offsets, not in the vectors
    lhs = ar.expand_log(V, L, N)[s2p]  # [S1, N+1]
    of, ff, kf = lr._segments(j)
    ob, fb, kb = lr._segments(i)
    i_f, w_f = i[of], w.astype(dt)[of]
    j_b, w_b = j[ob], w.astype(dt)[ob]
    so, lc = (_start_copy(g, state_in), 0.0) if c == 0 else (np.full(S1, -np.inf), -np.inf)
    A = np.full((S1, L), -np.inf, dtype=dt)
    C = np.zeros(L)
    total = -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (fr.start_vector(g, state_in).astype(dt) + (lhs[:, 0] - E[0]).astype(dt)).astype(dt)  # a~_n = ln a_n - C_n
        Cc = float(E[0])
        for n in range(L):
            A[:, n], C[n] = a, Cc
            M = a.max()
            if not np.isfinite(M):  # no live state: no mass from here on
                break
            lt = dt(np.log(np.sum(np.exp(a[:S] - M), dtype=dt)))
            v = (lr._seg_lse(a[i_f] + w_f, ff, kf, S1, dt) - M).astype(dt)  # ln sum_i a_n(i) T_hat(i, .) - C_n - M
            if n + 1 == c:
                so, lc = (v - lt).astype(np.float64), Cc + float(M) + float(lt)
            if n + 1 == L:
                total = Cc + float(M) + (float(v[S]) if closed else float(lt))
            else:
                Cc += float(M) + float(E[n + 1])
                a = (v + (lhs[:, n + 1] - E[n + 1]).astype(dt)).astype(dt)
        if not np.isfinite(total):
            return gamma, -np.inf, lc, so
        # backward: b~_n = ln b_n - D_n
        if closed:
            y = np.full(S1, -np.inf, dtype=dt)
            y[S] = 0
            bt = lr._seg_lse(w_b + y[j_b], fb, kb, S1, dt)
        else:
            bt = np.zeros(S1, dtype=dt)
            bt[S] = -np.inf
        D = 0.0
        for n in range(L - 1, -1, -1):
            lg = A[:, n].astype(np.float64) + bt.astype(np.float64) + (C[n] + D - total)
            q = np.exp(lg[:S].astype(dt)).astype(np.float64)
            s = q.sum()
            if s > 0:
                gamma[n] = np.bincount(s2p[:S], weights=q, minlength=P)[:P] / s
            y = (bt + (lhs[:, n] - E[n]).astype(dt)).astype(dt)
            M = y.max()
            M = M if np.isfinite(M) else dt(0)
            D += float(M) + float(E[n])
            bt = (lr._seg_lse(w_b + y[j_b], fb, kb, S1, dt) - M).astype(dt)
    return gamma, total, lc, so


def enumerate_paths(g, V, L, state_in=None, closed=False, commit=None):
    """(gamma [L, P], ttl, lcommit, state_out [S + 1]) by brute force over every state sequence s_1 .. s_L of the real states (tiny
    graphs only): a sequence weighs start(s_1) prod lhs prod T, times the final weight of s_L when the window is closed."""
    S, P = g.S, g.P
    i, j, w, _ = lr.entries(g)
    T = np.full((S + 1, S + 1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    st = fr.start_vector(g, state_in)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float64)
    c = _clamp_commit(commit, L)

    def weights(n):
        seqs = np.array(list(itertools.product(range(S), repeat=n)))  # [S^n, n]
        lw = st[seqs[:, 0]] + V[0, s2p[seqs[:, 0]]]
        for k in range(1, n):
            lw = lw + T[seqs[:, k - 1], seqs[:, k]] + V[k, s2p[seqs[:, k]]]
        return seqs, lw

    with np.errstate(invalid="ignore", divide="ignore"):
        seqs, lw = weights(L)
        if closed:
            lw = lw + T[seqs[:, -1], S]
        ttl = ar._lse(lw)
        pr = np.exp(lw - ttl)
        gamma = np.stack([np.bincount(s2p[seqs[:, n]], weights=pr, minlength=P)[:P] for n in range(L)])
        if c == 0:
            return gamma, ttl, 0.0, _start_copy(g, state_in)
        seqs, lw = weights(c)
        lc = ar._lse(lw)
        so = np.array([ar._lse(lw + T[seqs[:, -1], jj]) for jj in range(S + 1)]) - lc
    return gamma, ttl, lc, so
