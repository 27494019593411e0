"""Test helper: NumPy restatement of the best paths with arc classes (include/markovmodels_amd.h, mm_classpath_f32) by the header's
definition, over the entry list (i, j, w) of arc_reference.fsm_entries -- the stored entries of T_hat in the caller's order,
parallel entries between two states kept apart.  dtype = float32 performs the kernel's single-rounded operations in its order: one
add per arc, one more for the arc's score (U given: every arc adds its class's entry of the transition's row, an unclassified arc
and the phony self-loop the row's zero; U None: no second add), a max with the stated tie rule -- the lowest source, among
parallel maximisers from that source the lowest class id with -1 behind every class --, one add of the emission.  So its results
are the kernel's bit for bit.  dtype = float64 is the same recursion in double.  Plus a brute-force enumeration of every state
sequence of a tiny graph, and the score along a given path."""
import itertools
from types import SimpleNamespace

import numpy as np

import arc_reference as ar


def system(f, cls, C):
    """The entries of FSM f sorted by (destination, source, class key), the class key of an unclassified entry being C; the first
    entry of every destination that has one; alpha_hat [S1]; the phony self-loop's mask.  Weights as the device holds them: float32."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    cls = np.full(i.size, -1, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    key = np.where(cls < 0, C, cls)
    order = np.lexsort((key, i, j))
    i, j, w, key, cls = i[order], j[order], w[order].astype(np.float32), key[order], cls[order]
    first = np.flatnonzero(np.r_[True, j[1:] != j[:-1]])
    seg = np.cumsum(np.r_[False, j[1:] != j[:-1]])
    pi = np.full(S1, -np.inf, dtype=np.float32)
    np.maximum.at(pi, np.asarray(f.alpha_idx, dtype=np.int64), np.asarray(f.alpha_val).astype(np.float32))
    pi[S1 - 1] = -np.inf  # (the phony final state starts empty)
    phony = (i == S1 - 1) & (j == S1 - 1)
    newgrp = np.r_[True, (i[1:] != i[:-1]) | (j[1:] != j[:-1])]  # the (destination, source) groups: parallel entries share one
    grp = np.cumsum(newgrp) - 1
    return SimpleNamespace(i=i, j=j, w=w, key=key, cls=cls, first=first, seg=seg, keys=j[first], pi=pi, phony=phony, S1=S1, k=order, grp=grp,
                           gseg=seg[newgrp])


def _lhs(s2p, P, V, L, n, S1, dt):
    """lhs_n [S1], n counted from 1 (the phony final state: -inf up to len, 0 behind it)."""
    out = np.full(S1, -np.inf, dtype=dt)
    if n <= L:
        out[: S1 - 1] = np.asarray(V[n - 1], dtype=np.float32).astype(dt)[np.asarray(s2p)]
    else:
        out[S1 - 1] = 0
    return out


def reference(f, s2p, P, cls, C, U, V, L, N, dtype=np.float32):
    """One utterance: f an FSM, s2p [S] its pdfs, cls [nnz] in {-1, .., C-1} in f's entry order (None: no plan), U [>= L, C] or None,
    V [>= L, P], length L, N frames.  Returns path [N], classes [N] (-1 beyond L, without a path and for an unclassified entry),
    score, entries [N] (the caller's entry index taken at each transition, -1 where there is none), and the ties the tie rule
    decided along the recursion: src_ties (a maximum attained from several source states) and par_ties (attained by several
    entries from the winning source)."""
    dt = np.dtype(dtype).type
    sy = system(f, cls, C)
    S1 = sy.S1
    fs = S1 - 1
    path = np.full(N, -1, dtype=np.int32)
    classes = np.full(N, -1, dtype=np.int32)
    entries = np.full(N, -1, dtype=np.int64)
    res = SimpleNamespace(path=path, classes=classes, score=dt(-np.inf), entries=entries, src_ties=0, par_ties=0)
    if L == 0:
        return res
    w = sy.w.astype(dt)
    scored = (sy.cls >= 0) & ~sy.phony
    pos = np.arange(sy.i.size)
    big = np.iinfo(np.int64).max
    BP, BK, BE = [None, None], [None, None], [None, None]  # by frame, counted from 1
    with np.errstate(invalid="ignore"):
        d = (sy.pi.astype(dt) + _lhs(s2p, P, V, L, 1, S1, dt)).astype(dt)
        for n in range(2, L + 2):
            x = (w + d[sy.i]).astype(dt)
            if U is not None:
                u = np.zeros(sy.i.size, dtype=dt)
                u[scored] = np.asarray(U[n - 2], dtype=np.float32).astype(dt)[sy.cls[scored]]
                x = (x + u).astype(dt)
            best = np.full(S1, -np.inf, dtype=dt)
            bp = np.full(S1, -1, dtype=np.int64)
            bk = np.full(S1, -1, dtype=np.int64)
            be = np.full(S1, -1, dtype=np.int64)
            mx = np.maximum.reduceat(x, sy.first)
            hit = (x == mx[sy.seg]) & (mx[sy.seg] > -np.inf)
            at = np.minimum.reduceat(np.where(hit, pos, big), sy.first)  # (sorted by (source, key): the first hit is THE maximiser)
            ok = at < big
            best[sy.keys] = mx
            a = at[ok]
            bp[sy.keys[ok]] = sy.i[a]
            bk[sy.keys[ok]] = sy.cls[a]
            be[sy.keys[ok]] = sy.k[a]
            # the ties decided at this step: hits per (destination, source) group, hitting groups per destination
            ghit = np.bincount(sy.grp[hit], minlength=sy.gseg.size)
            nsrc = np.bincount(sy.gseg[ghit > 0], minlength=sy.first.size)
            res.src_ties += int((nsrc > 1).sum())
            res.par_ties += int((ghit[sy.grp[a]] > 1).sum())
            d = (best + _lhs(s2p, P, V, L, n, S1, dt)).astype(dt)
            BP.append(bp)
            BK.append(bk)
            BE.append(be)
    score = d[fs]
    if not score > -np.inf:
        return res
    res.score = score
    s = fs
    for n in range(L + 1, 1, -1):
        classes[n - 2] = BK[n][s]
        entries[n - 2] = BE[n][s]
        s = int(BP[n][s])
        path[n - 2] = s
    return res


def path_score(f, s2p, P, cls, U, V, path, entries, dtype=np.float32):
    """(d): the sum along a returned path in the recursion's order -- alpha_hat + lhs_1, then per transition (w + d) [+ u] + lhs."""
    dt = np.dtype(dtype).type
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    L = len(path)
    pi = np.full(S1, -np.inf, dtype=np.float32)
    np.maximum.at(pi, np.asarray(f.alpha_idx, dtype=np.int64), np.asarray(f.alpha_val).astype(np.float32))
    states = [int(s) for s in path] + [S1 - 1]
    d = dt(pi[states[0]]) + _lhs(s2p, P, V, L, 1, S1, dt)[states[0]]
    for t in range(L):
        k = int(entries[t])
        assert i[k] == states[t] and j[k] == states[t + 1]
        x = dt(dt(np.float32(w[k])) + d)
        if U is not None:
            c = -1 if cls is None else int(cls[k])
            x = dt(x + (dt(np.float32(U[t][c])) if c >= 0 else dt(0)))
        d = dt(x + _lhs(s2p, P, V, L, t + 2, S1, dt)[states[t + 1]])
    return d


def enumerate_paths(f, s2p, P, cls, C, U, V, L):
    """By brute force over every sequence s_1 .. s_L of the real states, float64 (tiny graphs, inputs without ties between state
    sequences): per transition and state pair the best parallel entry -- the greatest w + u, among equals the lowest class id, -1
    last --, then the best sequence.  Returns (path [L], classes [L], score), or (None, None, -inf)."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    S = S1 - 1
    cls = np.full(i.size, -1, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    w = w.astype(np.float32).astype(np.float64)
    pi = np.full(S1, -np.inf)
    np.maximum.at(pi, np.asarray(f.alpha_idx, dtype=np.int64), np.asarray(f.alpha_val).astype(np.float32).astype(np.float64))
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    T = np.full((L, S1, S1), -np.inf)
    K = np.full((L, S1, S1), -1, dtype=np.int64)
    for t in range(L):
        for k in range(i.size):
            x = w[k]
            if U is not None and cls[k] >= 0 and not (i[k] == S and j[k] == S):
                x = x + float(np.float32(U[t][cls[k]]))
            cur = K[t, i[k], j[k]]
            ck = C if cls[k] < 0 else cls[k]
            if x > T[t, i[k], j[k]] or (x == T[t, i[k], j[k]] and x > -np.inf and (cur < 0 or ck < (C if cls[cur] < 0 else cls[cur]))):
                T[t, i[k], j[k]] = x
                K[t, i[k], j[k]] = k
    s2p = np.asarray(s2p)
    seqs = np.array(list(itertools.product(range(S), repeat=L)))
    with np.errstate(invalid="ignore"):
        lw = pi[seqs[:, 0]] + Vd[0, s2p[seqs[:, 0]]]
        for t in range(L - 1):
            lw = lw + T[t][seqs[:, t], seqs[:, t + 1]] + Vd[t + 1, s2p[seqs[:, t + 1]]]
        lw = lw + T[L - 1][seqs[:, -1], S]
    lw = np.where(np.isnan(lw), -np.inf, lw)
    if not lw.max() > -np.inf:
        return None, None, -np.inf
    q = seqs[int(np.argmax(lw))]
    nxt = list(q[1:]) + [S]
    ks = [K[t, q[t], nxt[t]] for t in range(L)]
    return q, np.array([cls[k] for k in ks]), float(lw.max())
