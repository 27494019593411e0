"""Test helper: float64 reference of the posteriors with call-time weights (include/markovmodels_amd.h, mm_weightedposteriors_f32).
The definition, stated on the stored entries of T_hat / alpha_hat with W / W_init substituted for their weights (the entries ARE
the dense matrices: an entry list adds parallel entries in the log semiring exactly as a dense T_hat built from it would, and it
also fits the 70 000-state graph of the GPU tests): the forward and backward recursions in natural log, gamma from alpha + beta,
the counts from alpha + w + lhs + beta, all over log Z.  Plus brute-force enumeration for tiny graphs, and the graph REBUILT
with the substituted weights for the checks against the oracle."""
import dataclasses
import itertools

import numpy as np

import arc_reference as ar


def call_weights(f, W=None, W_init=None):
    """(i, j, w [nnz], a [S1]) of the call: W / W_init substituted (None: the FSM's own), the phony self-loop at one(K)."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    if W is not None:
        w = np.asarray(W, dtype=np.float64)[: i.size].copy()
    w = np.where((i == S1 - 1) & (j == S1 - 1), 0.0, w)
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val if W_init is None else W_init, dtype=np.float64)[: len(f.alpha_idx)]
    return i, j, w, a


def _seg_lse(x, idx, n):
    """out[s] = log sum_{k: idx[k] = s} exp(x[k]), -inf for an empty or all -inf segment."""
    m = np.full(n, -np.inf)
    np.maximum.at(m, idx, x)
    m0 = np.where(np.isfinite(m), m, 0.0)
    s = np.zeros(n)
    np.add.at(s, idx, np.exp(x - m0[idx]))
    with np.errstate(divide="ignore"):
        return m0 + np.log(s)


def reference(f, state2pdf, P, V, L, N, W=None, W_init=None):
    """gamma [N, P], counts [nnz] (f's CSC order), init [n_init] (f.alpha_idx order) and log Z of one utterance: V [>= L, P]
    log-likelihoods, length L, N frames, under the call's weights."""
    i, j, w, a = call_weights(f, W, W_init)
    S1 = f.colptr.size - 1
    s2p = np.concatenate([np.asarray(state2pdf, dtype=np.int64), [P]])
    lhs = ar.expand_log(V, L, N)[s2p]  # [S1, N + 1]
    A = np.full((S1, N + 1), -np.inf)
    Bm = np.full((S1, N + 1), -np.inf)
    with np.errstate(invalid="ignore"):
        A[:, 0] = a + lhs[:, 0]
        for n in range(N):
            A[:, n + 1] = _seg_lse(A[i, n] + w, j, S1) + lhs[:, n + 1]
        Bm[:, N] = 0.0
        for n in range(N - 1, -1, -1):
            Bm[:, n] = _seg_lse(w + lhs[j, n + 1] + Bm[j, n + 1], i, S1)
        logZ = float(ar._lse(A[:, 0] + Bm[:, 0]))
    gamma = np.zeros((N, P))
    counts = np.zeros(i.size)
    init = np.zeros(len(f.alpha_idx))
    if not np.isfinite(logZ):
        return gamma, counts, init, -np.inf
    with np.errstate(invalid="ignore"):
        post = np.exp(A + Bm - logZ)  # [S1, N + 1]
        post = np.where(np.isfinite(post), post, 0.0)
        for n in range(min(L, N)):
            gamma[n] = np.bincount(s2p, weights=post[:, n], minlength=P + 1)[:P]
        for n in range(N):
            t = A[i, n] + w + lhs[j, n + 1] + Bm[j, n + 1] - logZ
            counts += np.where(np.isfinite(t), np.exp(t), 0.0)
    init = post[np.asarray(f.alpha_idx, dtype=np.int64), 0].copy()
    return gamma, counts, init, logZ


def log_z(f, state2pdf, P, V, L, N, W=None, W_init=None):
    """log Z alone (the forward recursion): what the central differences perturb."""
    i, j, w, a = call_weights(f, W, W_init)
    S1 = f.colptr.size - 1
    s2p = np.concatenate([np.asarray(state2pdf, dtype=np.int64), [P]])
    lhs = ar.expand_log(V, L, N)[s2p]
    with np.errstate(invalid="ignore"):
        x = a + lhs[:, 0]
        for n in range(N):
            x = _seg_lse(x[i] + w, j, S1) + lhs[:, n + 1]
        return float(ar._lse(x))


def enumerate_paths(f, state2pdf, P, V, L, N, W=None, W_init=None):
    """The same four by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only)."""
    i, j, w, a = call_weights(f, W, W_init)
    S1 = f.colptr.size - 1
    T = np.full((S1, S1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    s2p = np.concatenate([np.asarray(state2pdf, dtype=np.int64), [P]])
    lhs = ar.expand_log(V, L, N)[s2p]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    with np.errstate(invalid="ignore"):
        lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
        for n in range(N):
            lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
    lw = np.where(np.isnan(lw), -np.inf, lw)
    logZ = float(ar._lse(lw))
    gamma = np.zeros((N, P))
    counts = np.zeros(i.size)
    init = np.zeros(len(f.alpha_idx))
    if not np.isfinite(logZ):
        return gamma, counts, init, -np.inf
    p = np.exp(lw - logZ)
    for n in range(min(L, N)):
        gamma[n] = np.bincount(s2p[paths[:, n]], weights=p, minlength=P + 1)[:P]
    for k in range(i.size):  # (parallel entries share the arc's posterior in proportion to their weights)
        used = ((paths[:, :-1] == i[k]) & (paths[:, 1:] == j[k])).sum(axis=1)
        share = np.exp(w[k] - T[i[k], j[k]]) if np.isfinite(w[k]) else 0.0
        counts[k] = np.sum(p * used) * share
    for m, s in enumerate(np.asarray(f.alpha_idx)):
        init[m] = np.sum(p[paths[:, 0] == s])
    return gamma, counts, init, logZ


def rebuilt(g, f, W=None, W_init=None):
    """The GraphSpec of g with the call's weights in the place of its own (graphs without parallel arcs): what `mm.compile` and the
    oracle are given when the weights are to be compiled in.  Entries at -inf are left out of the graph."""
    i, j, w, _ = call_weights(f, W, W_init)
    S = g.S
    arc = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(g.src, g.dst))}
    fin = {int(s): k for k, s in enumerate(g.final_idx)}
    gw = np.array(g.w, dtype=np.float64)
    fw = np.array(g.final_w, dtype=np.float64)
    for k in range(i.size):
        if i[k] == S and j[k] == S:
            continue
        if j[k] == S:
            fw[fin[int(i[k])]] = w[k]
        else:
            gw[arc[(int(i[k]), int(j[k]))]] = w[k]
    pos = {int(s): m for m, s in enumerate(np.asarray(f.alpha_idx))}
    wi = np.asarray(f.alpha_val if W_init is None else W_init, dtype=np.float64)  # (the FSM's own: what it holds, in its float type)
    iw = np.array([wi[pos[int(s)]] for s in g.init_idx])
    ka, kf, ki = np.isfinite(gw), np.isfinite(fw), np.isfinite(iw)
    return dataclasses.replace(g, name=g.name + "_w", src=g.src[ka], dst=g.dst[ka], w=gw[ka], final_idx=g.final_idx[kf], final_w=fw[kf],
                               init_idx=g.init_idx[ki], init_w=iw[ki])
