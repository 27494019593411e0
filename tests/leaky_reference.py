"""Test helper: float64 reference of the leaky-HMM pdf posteriors (include/markovmodels_amd.h, mm_leakyposteriors_f32) by the
header's recursion -- sparse T_hat plus the rank-one leak term, never an S x S matrix --, a float32 mode of the same recursion
(what float32 arithmetic alone costs), and `densify`, which writes T_eps = (I + eps u pi') T_hat out as the arcs of a GraphSpec so
that the existing oracle can run the leaky system as a plain FSM."""
import numpy as np

import arc_reference as ar


def _segments(key):
    """Entries sorted by `key`: the order, the first entry of every non-empty segment, the segments' keys."""
    order = np.argsort(key, kind="stable")
    ks = key[order]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    return order, first, ks[first]


def _seg_lse(t, first, keys, n, dt):
    """Per segment log sum exp of t (already in segment order), scattered to [n]; -inf for a state without a segment."""
    out = np.full(n, -np.inf, dtype=dt)
    m = np.maximum.reduceat(t, first)
    m0 = np.where(np.isfinite(m), m, 0).astype(dt)
    cnt = np.diff(np.concatenate([first, [t.size]]))
    with np.errstate(divide="ignore"):
        out[keys] = m0 + np.log(np.add.reduceat(np.exp(t - np.repeat(m0, cnt)), first)).astype(dt)
    return out


def _lse(x, dt):
    m = np.max(x)
    m0 = m if np.isfinite(m) else dt(0)
    with np.errstate(divide="ignore"):
        return dt(m0 + np.log(np.sum(np.exp(x - m0), dtype=dt)))


def entries(g):
    """The extended system of a GraphSpec: the stored entries (i, j, natural-log weight) of T_hat = [T omega; 0 1], pi [S + 1]."""
    S = g.S
    i = np.concatenate([g.src, g.final_idx, [S]]).astype(np.int64)
    j = np.concatenate([g.dst, np.full(g.final_idx.size, S), [S]]).astype(np.int64)
    w = np.concatenate([g.w, g.final_w, [0.0]]).astype(np.float64)
    pi = np.full(S + 1, -np.inf)
    for k, x in zip(g.init_idx, g.init_w):
        pi[k] = np.logaddexp(pi[k], x)
    return i, j, w, pi


def rho(g):
    """rho(j) = log sum_k pi(k) T_hat(k, j), [S + 1] (the phony final column included)."""
    i, j, w, pi = entries(g)
    order, first, keys = _segments(j)
    return _seg_lse((pi[i] + w)[order], first, keys, g.S + 1, np.float64)


def reference(g, V, L, N, eps, dtype=np.float64):
    """gamma [N, P] and log Z (= ttl) of one utterance of the leaky HMM: V [>= L, P] natural-log likelihoods, length L, N frames,
    leak coefficient eps.  The vectors are carried normalised by the maximum of the frame before (forward) / after (backward)
    with float64 offsets, as the kernels carry them; dtype = float32 rounds the vectors and every sum over them to float32."""
    dt = np.dtype(dtype).type
    S, S1, P = g.S, g.S + 1, g.P
    i, j, w, pi = entries(g)
    s2p = ar._s2p_full(g)
    lhs = ar.expand_log(V, L, N)[s2p].astype(dt)  # [S1, N+1]
    leps = dt(np.log(eps)) if eps > 0 else dt(-np.inf)
    r = rho(g).astype(dt)
    pi_t, w_t = pi.astype(dt), w.astype(dt)
    of, ff, kf = _segments(j)
    ob, fb, kb = _segments(i)
    i_f, w_f = i[of], w_t[of]
    j_b, w_b = j[ob], w_t[ob]
    gamma = np.zeros((N, P))
    with np.errstate(invalid="ignore"):
        A = np.full((S1, N + 1), -np.inf, dtype=dt)
        C = np.zeros(N + 1)
        A[:, 0] = pi_t + lhs[:, 0]
        for n in range(1, N + 1):
            a = A[:, n - 1]
            M = a.max()
            M = M if np.isfinite(M) else dt(0)
            C[n] = C[n - 1] + float(M)
            v = _seg_lse(a[i_f] + w_f, ff, kf, S1, dt)
            leak = leps + _lse(a[:S], dt) + r
            A[:, n] = (lhs[:, n] + np.logaddexp(v, leak) - M).astype(dt)
        logZ = float(A[S, N]) + C[N]
        if not np.isfinite(logZ):
            return gamma, -np.inf
        Bm = np.full((S1, N + 1), -np.inf, dtype=dt)
        D = np.zeros(N + 1)
        Bm[:, N] = 0
        for n in range(N - 1, -1, -1):
            y = Bm[:, n + 1] + lhs[:, n + 1]
            M = y.max()
            M = M if np.isfinite(M) else dt(0)
            D[n] = D[n + 1] + float(M)
            z = (_seg_lse(w_b + y[j_b], fb, kb, S1, dt) - M).astype(dt)
            c = _lse(pi_t + z, dt)
            Bm[:S, n] = np.logaddexp(z[:S], leps + c)
            Bm[S, n] = z[S]
        lg = A.astype(np.float64) + Bm.astype(np.float64) + (C + D)[None, :]  # [S1, N+1] log alpha beta
    ttl = np.inf
    for n in range(N + 1):
        m = lg[:, n].max()
        s = m + np.log(np.sum(np.exp(lg[:, n] - m)))
        ttl = min(ttl, s)
        if n < L:
            q = np.exp(lg[:S, n] - s)
            gamma[n] = np.bincount(s2p[:S], weights=q, minlength=P)[:P]
    return gamma, float(ttl)


def densify(g, eps):
    """A GraphSpec whose arcs are T_eps = (I + eps u pi') T_hat written out: arc i -> j of weight T(i, j) + eps rho(j) for every real
    i and every j that T or rho reaches, final weight omega(i) + eps rho(final).  O(S^2) arcs: small graphs only."""
    import dataclasses

    S = g.S
    T = np.full((S, S + 1), -np.inf)
    np.logaddexp.at(T, (g.src, g.dst), g.w)
    np.logaddexp.at(T, (g.final_idx, np.full(g.final_idx.size, S)), g.final_w)
    if eps > 0:
        T = np.logaddexp(T, np.log(eps) + rho(g)[None, :])
    src, dst = np.nonzero(np.isfinite(T[:, :S]))
    fin = np.flatnonzero(np.isfinite(T[:, S]))
    return dataclasses.replace(g, name=g.name + "_dense", src=src, dst=dst, w=T[src, dst], final_idx=fin, final_w=T[fin, S])
