"""Test helper: float64 reference of the forward filtering posteriors with a carried state (include/markovmodels_amd.h,
mm_filterposteriors_f32) by the header's definition -- the sparse extended system of leaky_reference.entries, the vector carried
normalised by the maximum of the frame before with a float64 offset, as the kernel carries it --, a float32 mode of the same
recursion (vectors and sums rounded to float32: what float32 arithmetic alone costs), and a brute-force enumeration of every state
sequence of a tiny graph."""
import itertools

import numpy as np

import arc_reference as ar
import leaky_reference as lr


def start_vector(g, state_in=None):
    """The start vector [S + 1], natural log: the FSM's own initial vector, or state_in with its final entry ignored."""
    if state_in is None:
        return lr.entries(g)[3]
    st = np.asarray(state_in, dtype=np.float64).copy()
    st[g.S] = -np.inf
    return st


def reference(g, V, L, N, state_in=None, dtype=np.float64):
    """(filt [N, P], incr [N], ttl, state_out [S + 1]) of one utterance: V [>= L, P] natural-log likelihoods, length L, N frames,
    state_in [S + 1] natural log or None.  dtype = float32 rounds the vectors and every sum over them to float32."""
    dt = np.dtype(dtype).type
    S, S1, P = g.S, g.S + 1, g.P
    i, j, w, _ = lr.entries(g)
    s2p = ar._s2p_full(g)
    filt, incr = np.zeros((N, P)), np.zeros(N)
    if L == 0:  # the state passes through
        so = np.asarray(state_in, dtype=np.float64).copy() if state_in is not None else start_vector(g)
        return filt, incr, -np.inf, so
    lhs = ar.expand_log(V, L, N)[s2p].astype(dt)  # [S1, N+1]
    of, ff, kf = lr._segments(j)
    i_f, w_f = i[of], w.astype(dt)[of]
    dead = (filt, incr, -np.inf, np.full(S1, -np.inf))
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (start_vector(g, state_in).astype(dt) + lhs[:, 0]).astype(dt)  # a~_n = ln a_n - C
        C, ltp = 0.0, dt(0)
        for n in range(L):
            M = a.max()
            if not np.isfinite(M):  # no live state: the conventions from here on
                incr[n:L] = -np.inf
                return dead
            x = np.exp(a - M)
            tot = np.sum(x, dtype=dt)
            filt[n] = np.bincount(s2p[:S], weights=x[:S].astype(np.float64), minlength=P)[:P] / float(tot)
            lt = dt(np.log(tot))
            incr[n] = float(dt(M + (lt - ltp)))
            ltp = lt
            C += float(M)
            v = (lr._seg_lse(a[i_f] + w_f, ff, kf, S1, dt) - M).astype(dt)  # ln sum_i a_n(i) T_hat(i, .) - C
            a = (v + lhs[:, n + 1]).astype(dt)
        state_out = (v - ltp).astype(np.float64)
        ttl = C + float(v[S])
    return filt, incr, (ttl if np.isfinite(ttl) else -np.inf), state_out


def enumerate_prefixes(g, V, L, state_in=None):
    """(filt [L, P], incr [L], state_out [S + 1]) by brute force over every state sequence s_1 .. s_n of the real states, n = 1..L
    (tiny graphs only)."""
    S, P = g.S, g.P
    i, j, w, _ = lr.entries(g)
    T = np.full((S + 1, S + 1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    st = start_vector(g, state_in)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float64)
    filt, incr = np.zeros((L, P)), np.zeros(L)
    lprev = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in range(1, L + 1):
            seqs = np.array(list(itertools.product(range(S), repeat=n)))  # [S^n, n]
            lw = st[seqs[:, 0]] + V[0, s2p[seqs[:, 0]]]
            for k in range(1, n):
                lw = lw + T[seqs[:, k - 1], seqs[:, k]] + V[k, s2p[seqs[:, k]]]
            ln = ar._lse(lw)
            incr[n - 1] = ln - lprev
            lprev = ln
            pr = np.exp(lw - ln)
            filt[n - 1] = np.bincount(s2p[seqs[:, -1]], weights=pr, minlength=P)[:P]
        state_out = np.array([ar._lse(lw + T[seqs[:, -1], jj]) for jj in range(S + 1)]) - ln
    return filt, incr, state_out
