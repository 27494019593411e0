"""Test helper: float64 reference of the segment posteriors (include/markovmodels_amd.h, mm_segmentposteriors_f32) by the header's
definition -- tests/window_reference.py's recursions (the sparse extended system of leaky_reference.entries; both vectors carried
normalised by the maximum of the frame before, the frame's largest emission in a float64 offset) with an end vector: the third way
to start the backward recursion, and one more backward step behind the first frame for end_out and lend --, a float32 mode of the
same recursions (vectors and sums rounded to float32: what float32 arithmetic alone costs), a brute-force enumeration of every state
sequence of a tiny graph for the three end modes, and `chained`, the two-pass scheme over chunks on the references."""
import itertools

import numpy as np

import arc_reference as ar
import filter_reference as fr
import leaky_reference as lr


def end_kind(mode, end_in):
    """'open', 'final' or 'carried', as the header decides it."""
    if int(mode) == 0:
        return "open"
    return "carried" if int(mode) == 2 and end_in is not None else "final"


def _final_weights(g, dt=np.float64):
    """ln T_hat(i, f) [S + 1], the entry of f itself -inf."""
    S1 = g.S + 1
    i, j, w, _ = lr.entries(g)
    ob, fb, kb = lr._segments(i)
    y = np.full(S1, -np.inf, dtype=dt)
    y[g.S] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        bt = lr._seg_lse(w.astype(dt)[ob] + y[j[ob]], fb, kb, S1, dt)
    bt[g.S] = -np.inf
    return bt


def reference(g, V, L, N, state_in=None, mode=0, end_in=None, dtype=np.float64):
    """(gamma [N, P], ttl, lend, end_out [S + 1]) of one utterance: V [>= L, P] natural-log likelihoods, length L, N frames,
    state_in [S + 1] natural log or None, the end mode and end_in [S + 1] natural log or None.  dtype = float32 rounds the vectors
    and every sum over them to float32."""
    dt = np.dtype(dtype).type
    S, S1, P = g.S, g.S + 1, g.P
    kind = end_kind(mode, end_in)
    gamma = np.zeros((N, P))
    dead = (gamma, -np.inf, -np.inf, np.full(S1, -np.inf))
    if L == 0:  # the end vector the segment was given
        if kind == "carried":
            return gamma, -np.inf, 0.0, np.asarray(end_in, dtype=np.float64).copy()
        if kind == "open":
            e = np.zeros(S1)
            e[S] = -np.inf
            return gamma, -np.inf, 0.0, e
        fw = _final_weights(g, dt).astype(np.float64)
        m = fw.max()
        return (gamma, -np.inf, float(m), fw - m) if np.isfinite(m) else dead
    i, j, w, _ = lr.entries(g)
    s2p = ar._s2p_full(g)
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        E = np.max(V[:L], axis=1)
    E = np.where(np.isfinite(E), E, 0.0)  # the frame's largest emission: in the offsets, not in the vectors
    lhs = ar.expand_log(V, L, N)[s2p]  # [S1, N+1]
    of, ff, kf = lr._segments(j)
    ob, fb, kb = lr._segments(i)
    i_f, w_f = i[of], w.astype(dt)[of]
    j_b, w_b = j[ob], w.astype(dt)[ob]
    A = np.full((S1, L), -np.inf, dtype=dt)
    C = np.zeros(L)
    total = -np.inf
    D = 0.0
    bt = None
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "carried":  # b~_len = end_in - its maximum, the maximum in the offset
            be = np.asarray(end_in, dtype=np.float64).astype(dt)
            be[S] = -np.inf
            m1 = be.max()
            if not np.isfinite(m1):
                return dead
            bt, D = (be - m1).astype(dt), float(m1)
        elif kind == "open":
            bt = np.zeros(S1, dtype=dt)
            bt[S] = -np.inf
        a = (fr.start_vector(g, state_in).astype(dt) + (lhs[:, 0] - E[0]).astype(dt)).astype(dt)  # a~_n = ln a_n - C_n
        Cc = float(E[0])
        for n in range(L):
            A[:, n], C[n] = a, Cc
            M = a.max()
            if not np.isfinite(M):  # no live state: no mass from here on
                break
            if n + 1 == L:
                if kind == "carried":
                    lg = (a + bt).astype(dt)
                    m2 = lg.max()
                    if np.isfinite(m2):
                        total = Cc + D + float(m2) + float(dt(np.log(np.sum(np.exp(lg - m2), dtype=dt))))
                elif kind == "open":
                    total = Cc + float(M) + float(dt(np.log(np.sum(np.exp(a[:S] - M), dtype=dt))))
                else:
                    v = (lr._seg_lse(a[i_f] + w_f, ff, kf, S1, dt) - M).astype(dt)
                    total = Cc + float(M) + float(v[S])
            else:
                v = (lr._seg_lse(a[i_f] + w_f, ff, kf, S1, dt) - M).astype(dt)  # ln sum_i a_n(i) T_hat(i, .) - C_n - M
                Cc += float(M) + float(E[n + 1])
                a = (v + (lhs[:, n + 1] - E[n + 1]).astype(dt)).astype(dt)
        if not np.isfinite(total):
            return dead
        if kind == "final":
            y = np.full(S1, -np.inf, dtype=dt)
            y[S] = 0
            bt = lr._seg_lse(w_b + y[j_b], fb, kb, S1, dt)
        # backward: b~_n = ln b_n - D_n
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
        # bt is b~_0 on every row of the extended system; the final state hands nothing back
        b0 = bt.astype(np.float64)
        b0[S] = -np.inf
        m0 = b0.max()
        if not np.isfinite(m0):
            return gamma, total, -np.inf, np.full(S1, -np.inf)
        return gamma, total, D + float(m0), b0 - m0


def enumerate_paths(g, V, L, state_in=None, mode=0, end_in=None):
    """(gamma [L, P], ttl, lend, end_out [S + 1]) by brute force over every state sequence s_1 .. s_L of the real states (tiny graphs
    only, L >= 1): a sequence weighs start(s_1) prod lhs prod T times the end weight of s_L -- 1, the final weight, or
    exp(end_in); b_0(i) is the sum over the sequences entered from i."""
    S, P = g.S, g.P
    i, j, w, _ = lr.entries(g)
    T = np.full((S + 1, S + 1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    st = fr.start_vector(g, state_in)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float64)
    kind = end_kind(mode, end_in)
    seqs = np.array(list(itertools.product(range(S), repeat=L)))  # [S^L, L]
    with np.errstate(invalid="ignore", divide="ignore"):
        body = V[0, s2p[seqs[:, 0]]]  # what the sequence weighs behind its entry
        for k in range(1, L):
            body = body + T[seqs[:, k - 1], seqs[:, k]] + V[k, s2p[seqs[:, k]]]
        if kind == "final":
            body = body + T[seqs[:, -1], S]
        elif kind == "carried":
            body = body + np.asarray(end_in, dtype=np.float64)[seqs[:, -1]]
        lw = st[seqs[:, 0]] + body
        ttl = ar._lse(lw)
        gamma = np.zeros((L, P))
        if np.isfinite(ttl):
            pr = np.exp(lw - ttl)
            gamma = np.stack([np.bincount(s2p[seqs[:, n]], weights=pr, minlength=P)[:P] for n in range(L)])
        b0 = np.array([ar._lse(T[ii, seqs[:, 0]] + body) for ii in range(S + 1)])
        b0[S] = -np.inf
        m0 = b0.max()
    if not np.isfinite(m0):
        return gamma, ttl, -np.inf, np.full(S + 1, -np.inf)
    return gamma, ttl, m0, b0 - m0


def chained(g, V, L, N, chunk, dtype=np.float64):
    """BatchedFSM.chunkedposteriors' bookkeeping for one utterance on the references: (gamma [N, P], ttl, the most frames one call
    saw).  Pass 1: the filter per chunk, each chunk's start state saved, ttl by the filter's book; pass 2: the segments in reverse,
    mode 1 where the utterance ends in the chunk or before it, else 2 on the end vector the chunk behind handed back."""
    V = np.asarray(V, dtype=np.float64)
    P = g.P
    gamma = np.zeros((N, P))
    if chunk >= N:
        gam, ttl, _, _ = reference(g, V, L, N, None, 1, None, dtype)
        return gam, ttl, N
    K = -(-N // chunk)
    lens = [min(max(L - k * chunk, 0), chunk) for k in range(K)]
    starts, state, loglik = [], None, 0.0
    for k in range(K):
        starts.append(state)
        _, incr, _, state = fr.reference(g, V[k * chunk :], lens[k], chunk, state, dtype)
        loglik += incr.sum()
    ttl = loglik + state[g.S]
    end, seen = None, 0
    for k in range(K - 1, -1, -1):
        n = min(chunk, N - k * chunk)
        seen = max(seen, n)
        mode = 1 if L <= (k + 1) * chunk else 2
        gam, _, _, end = reference(g, V[k * chunk :], lens[k], n, starts[k], mode, end, dtype)
        gamma[k * chunk : k * chunk + n] = gam
    return gamma, (float(ttl) if np.isfinite(ttl) else -np.inf), seen
