"""Test helper: NumPy restatement of the windowed best paths (include/markovmodels_amd.h, mm_viterbiwindow_f32) by the header's
definition -- the sparse extended system of leaky_reference.entries with max in the place of the sum; dtype = float32 performs the
kernels' single-rounded operations in their order (one add per arc, a max, one add of the emission, one subtraction for
state_out), so its results are the kernels' bit for bit --, a brute-force enumeration of every state sequence of a tiny graph for
both end modes (best path, score and the surviving sets), the float64 score of a given path, and a host replay of
streaming.OnlineViterbi's policy on top of the restatement."""
import itertools
from types import SimpleNamespace

import numpy as np

import leaky_reference as lr


def system(g):
    """The extended tropical system of a GraphSpec as the device holds it (float32 weights): the entries (i, j, w) sorted by
    (j, i), the first entry and the key of every column that has one, and alpha_hat [S + 1]."""
    i, j, w, _ = lr.entries(g)
    w = w.astype(np.float32)
    order = np.lexsort((i, j))
    i, j, w = i[order], j[order], w[order]
    first = np.flatnonzero(np.r_[True, j[1:] != j[:-1]])
    pi = np.full(g.S + 1, -np.inf, dtype=np.float32)
    np.maximum.at(pi, np.asarray(g.init_idx, dtype=np.int64), np.asarray(g.init_w).astype(np.float32))
    seg = np.cumsum(np.r_[False, j[1:] != j[:-1]])  # entry -> its column's rank among the columns that have entries
    return SimpleNamespace(i=i, j=j, w=w, first=first, keys=j[first], seg=seg, pi=pi)


def start_vector(g, state_in=None, sys=None):
    """The start vector [S + 1]: alpha_hat, or state_in with its final entry ignored."""
    if state_in is None:
        return (sys or system(g)).pi.copy()
    st = np.asarray(state_in).copy()
    st[g.S] = -np.inf
    return st


def _start_copy(g, state_in, sys):
    """What state_out holds when nothing is committed: the start vector as given (its final entry included)."""
    return np.asarray(state_in).copy() if state_in is not None else sys.pi.copy()


def _step(sys, d, S1):
    """best(j) = max_i d(i) + T_hat(i, j) and bp(j) = the lowest i among the maximisers (-1: the max is -inf)."""
    val = d[sys.i] + sys.w.astype(d.dtype)
    best = np.full(S1, -np.inf, dtype=d.dtype)
    bp = np.full(S1, -1, dtype=np.int64)
    if val.size:
        mx = np.maximum.reduceat(val, sys.first)
        best[sys.keys] = mx
        cand = np.where(val == mx[sys.seg], sys.i, np.iinfo(np.int64).max)
        lo = np.minimum.reduceat(cand, sys.first)
        bp[sys.keys] = np.where(mx > -np.inf, lo, -1)
    return best, bp


def _lhs(g, V, L, n, dt):
    """lhs_n [S + 1], n counted from 1: the emissions of frame n by state (the phony final state: -inf up to len, 0 behind it)."""
    out = np.full(g.S + 1, -np.inf, dtype=dt)
    if n <= L:
        out[: g.S] = np.asarray(V[n - 1], dtype=np.float32).astype(dt)[np.asarray(g.state2pdf)]
    else:
        out[g.S] = 0
    return out


def reference(g, V, L, N, state_in=None, closed=False, commit=None, commit_converged=False, dtype=np.float64, sys=None):
    """One utterance: V [>= L, P] natural-log likelihoods (float32 values), length L, N frames, state_in [S + 1] or None, the end
    mode, the commit frame (None: L, or 0 with commit_converged).  Returns path [N] (0-based, -1 beyond L or without a path),
    score, converged, ncommit, mcommit, state_out [S + 1] and sets: the surviving sets A_1 .. A_L as sorted arrays."""
    dt = np.dtype(dtype).type
    sys = sys or system(g)
    S, S1 = g.S, g.S + 1
    path = np.full(N, -1, dtype=np.int32)
    c = (0 if commit_converged else L) if commit is None else min(max(int(commit), 0), L)
    res = SimpleNamespace(path=path, score=-np.inf, converged=0, ncommit=0, mcommit=dt(0), state_out=_start_copy(g, state_in, sys).astype(dt), sets=[])
    if L == 0:
        return res
    with np.errstate(invalid="ignore"):
        d = (start_vector(g, state_in, sys).astype(dt) + _lhs(g, V, L, 1, dt)).astype(dt)
        D, BEST, BP = [None, d], [None, None], [None, None]  # by frame, counted from 1
        for n in range(2, L + 2):
            best, bp = _step(sys, d, S1)
            d = (best + _lhs(g, V, L, n, dt)).astype(dt)
            D.append(d)
            BEST.append(best)
            BP.append(bp)
        dl = D[L]
        if closed:
            score, end = D[L + 1][S], int(BP[L + 1][S])
            e = np.full(S1, -np.inf, dtype=dt)
            fin = sys.j == S
            np.maximum.at(e, sys.i[fin], (dl[sys.i[fin]] + sys.w[fin].astype(dt)).astype(dt))
            e[S] = -np.inf
        else:
            e = dl.copy()
            e[S] = -np.inf
            score, end = e.max(), int(np.argmax(e))
    if score > -np.inf:
        res.score = score
        s = end
        for n in range(L, 0, -1):
            path[n - 1] = s
            if n >= 2:
                s = int(BP[n][s])
        A = np.flatnonzero(e > -np.inf)
        sets = [A]
        for n in range(L, 1, -1):
            A = np.unique(BP[n][A])
            sets.append(A)
        res.sets = sets[::-1]
        res.converged = max([n + 1 for n, A in enumerate(res.sets) if A.size == 1], default=0)
    else:
        res.score = dt(-np.inf)
    if commit_converged:
        c = max(c, res.converged)
    res.ncommit = c
    if c >= 1:
        mc = D[c][:S].max()
        res.mcommit = mc
        res.state_out = (BEST[c + 1] - mc).astype(dt) if mc > -np.inf else np.full(S1, -np.inf, dtype=dt)
    return res


def path_score(g, V, path, state_in=None, closed=False):
    """The float64 weight of a given state sequence (a window's whole path) from the start vector."""
    sys = system(g)
    T = np.full((g.S + 1, g.S + 1), -np.inf)
    np.maximum.at(T, (sys.i, sys.j), sys.w.astype(np.float64))
    st = start_vector(g, state_in, sys).astype(np.float64)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float64)
    path = [int(s) for s in path]
    if not path:
        return -np.inf
    tot = st[path[0]] + V[0, s2p[path[0]]]
    for k in range(1, len(path)):
        tot += T[path[k - 1], path[k]] + V[k, s2p[path[k]]]
    return tot + (T[path[-1], g.S] if closed else 0.0)


def enumerate_paths(g, V, L, state_in=None, closed=False):
    """By brute force over every state sequence s_1 .. s_L of the real states (tiny graphs only, float64): the best sequence, its
    weight, and the surviving sets -- per end state with a finite weight the best sequence that ends there; A_n = their n-th
    states.  (Inputs without ties: the best sequences are unique.)"""
    sys = system(g)
    S = g.S
    T = np.full((S + 1, S + 1), -np.inf)
    np.maximum.at(T, (sys.i, sys.j), sys.w.astype(np.float64))
    st = start_vector(g, state_in, sys).astype(np.float64)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    seqs = np.array(list(itertools.product(range(S), repeat=L)))  # [S^L, L]
    with np.errstate(invalid="ignore"):
        lw = st[seqs[:, 0]] + V[0, s2p[seqs[:, 0]]]
        for k in range(1, L):
            lw = lw + T[seqs[:, k - 1], seqs[:, k]] + V[k, s2p[seqs[:, k]]]
        if closed:
            lw = lw + T[seqs[:, -1], S]
    score = lw.max()
    if not score > -np.inf:
        return np.full(L, -1), -np.inf, [], 0
    survivors = []
    for i in range(S):
        m = seqs[:, -1] == i
        if m.any() and lw[m].max() > -np.inf:
            survivors.append(seqs[m][np.argmax(lw[m])])
    survivors = np.array(survivors)
    sets = [np.unique(survivors[:, n]) for n in range(L)]
    conv = max([n + 1 for n, A in enumerate(sets) if A.size == 1], default=0)
    return seqs[np.argmax(lw)], score, sets, conv


def enumerate_commit(g, V, c, state_in=None):
    """(m_c, state_out [S + 1]) for a commit frame c >= 1 by brute force over every state sequence of c real states (float64)."""
    sys = system(g)
    S = g.S
    T = np.full((S + 1, S + 1), -np.inf)
    np.maximum.at(T, (sys.i, sys.j), sys.w.astype(np.float64))
    st = start_vector(g, state_in, sys).astype(np.float64)
    s2p = np.asarray(g.state2pdf)
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    seqs = np.array(list(itertools.product(range(S), repeat=c)))
    with np.errstate(invalid="ignore"):
        lw = st[seqs[:, 0]] + V[0, s2p[seqs[:, 0]]]
        for k in range(1, c):
            lw = lw + T[seqs[:, k - 1], seqs[:, k]] + V[k, s2p[seqs[:, k]]]
        mc = lw.max()
        if not mc > -np.inf:
            return mc, np.full(S + 1, -np.inf)
        return mc, np.array([(lw + T[seqs[:, -1], j]).max() for j in range(S + 1)]) - mc


def replay_online(g, V, chunk_lens, max_pending, dtype=np.float32, finish=True):
    """streaming.OnlineViterbi's policy for one utterance on the host: `chunk_lens[k]` frames of V arrive with push k.  Returns
    (emitted: per push the newly committed states, and last the states of finish; score: the running score behind the pushes;
    nforced; total: the score finish returns, None without finish)."""
    sys = system(g)
    P = g.P
    state, pending, n0 = None, np.zeros((0, P), dtype=np.float32), 0
    emitted, score, nforced = [], 0.0, 0
    for k in chunk_lens:
        win = np.concatenate([pending, np.asarray(V[n0 : n0 + k], dtype=np.float32)])
        n0 += k
        wlen = win.shape[0]
        r = reference(g, win, wlen, max(wlen, 1), state, False, max(0, wlen - max_pending), True, dtype, sys)
        emitted.append(r.path[: r.ncommit].copy())
        score += float(r.mcommit)
        nforced += max(0, r.ncommit - r.converged)
        state, pending = r.state_out, win[r.ncommit :]
    total = None
    if finish:
        wlen = pending.shape[0]
        r = reference(g, pending, wlen, max(wlen, 1), state, True, None, False, dtype, sys)
        emitted.append(r.path[:wlen].copy())
        # (nothing pending: the carried state's final entry, the best final weight behind the last frame)
        total = score + float(r.score if wlen else (state[g.S] if state is not None else sys.pi[g.S]))
    return emitted, score, nforced, total
