"""Test helper for the posterior path sampling (include/markovmodels_amd.h, mm_samplepaths_f32), float64, NumPy: the exact
posterior over the state sequences of a tiny graph by enumeration, the log-probability of one state sequence on any graph, a
plain forward-filter / backward-sample sampler, and the acceptance rule of the distribution tests (Bernstein's inequality)."""
import itertools

import numpy as np

import arc_reference as ar

#: the tiny cases of the distribution tests: (states, seed, frames N, length); graph wl.random_fsm(S, 3, 2.0, seed)
TINY_CASES = [(5, 1, 6, 6), (5, 2, 6, 6), (5, 3, 6, 6), (5, 4, 6, 6), (6, 1, 6, 5), (6, 2, 6, 5), (6, 3, 6, 5), (6, 4, 6, 5)]
#: their support sizes, as enumerated when the tests were written (a check of the enumeration itself)
TINY_SUPPORT = [50, 3, 5, 137, 14, 11, 9, 30]


def tiny_case(mm, wl, S, seed, N):
    g = wl.random_fsm(S, 3, 2.0, seed)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    V = np.random.default_rng(100 + seed).standard_normal((N, 3))
    return g, f, V


class Graph:
    """One FSM for the helpers below: the merged transitions (parallel entries of one (source, destination) log-added: the
    probabilities are over STATE sequences) as sorted keys i * S1 + j, alpha_hat, the state -> pdf map."""

    def __init__(self, g, f):
        i, j, w = ar.fsm_entries(f)
        self.S1 = f.colptr.size - 1
        self.fin = self.S1 - 1
        key = i * self.S1 + j
        self.keys, inv = np.unique(key, return_inverse=True)
        self.w = np.full(self.keys.size, -np.inf)
        np.logaddexp.at(self.w, inv, w)
        self.a = np.full(self.S1, -np.inf)
        self.a[np.asarray(f.alpha_idx, dtype=np.int64)] = np.asarray(f.alpha_val, dtype=np.float64)
        self.s2p = np.concatenate([np.asarray(g.state2pdf, dtype=np.int64), [g.P]])

    def weight(self, i, j):
        """log T_hat[i, j] of arrays of states (-inf where there is no arc)."""
        key = np.asarray(i, dtype=np.int64) * self.S1 + np.asarray(j, dtype=np.int64)
        pos = np.minimum(np.searchsorted(self.keys, key), self.keys.size - 1)
        return np.where(self.keys[pos] == key, self.w[pos], -np.inf)

    def dense(self):
        T = np.full((self.S1, self.S1), -np.inf)
        T[self.keys // self.S1, self.keys % self.S1] = self.w
        return T


def path_logprob(gr, V, paths):
    """Un-normalised natural-log weight of state sequences paths [K, L] (0-based real states) under emissions V [>= L, P]:
    log alpha_hat(s_1) + sum log lhs + sum log T_hat + log omega(s_L).  Subtract log Z for the posterior probability."""
    paths = np.asarray(paths, dtype=np.int64)
    K, L = paths.shape
    V = np.asarray(V, dtype=np.float64)
    lw = gr.a[paths[:, 0]] + gr.weight(paths[:, -1], np.full(K, gr.fin))
    for n in range(L):
        lw = lw + V[n, gr.s2p[paths[:, n]]]
    for n in range(L - 1):
        lw = lw + gr.weight(paths[:, n], paths[:, n + 1])
    return lw


def enumerate_posterior(gr, V, L):
    """Every state sequence of L frames with positive posterior: (paths [M, L], log p [M], log Z)."""
    S = gr.S1 - 1
    paths = np.array(list(itertools.product(range(S), repeat=L)), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        lw = path_logprob(gr, V, paths)
    keep = np.isfinite(lw)
    paths, lw = paths[keep], lw[keep]
    logZ = float(np.logaddexp.reduce(lw))
    return paths, lw - logZ, logZ


def path_codes(gr, paths):
    """One integer per row of paths [K, L]."""
    paths = np.asarray(paths, dtype=np.int64)
    code = np.zeros(paths.shape[0], dtype=np.int64)
    for n in range(paths.shape[1]):
        code = code * gr.S1 + paths[:, n]
    return code


def frequencies(gr, support, samples):
    """Empirical frequency of every support path among samples [K, L], and how many samples lie outside the support."""
    sc = path_codes(gr, support)
    order = np.argsort(sc)
    code = path_codes(gr, samples)
    pos = np.minimum(np.searchsorted(sc[order], code), sc.size - 1)
    hit = sc[order][pos] == code
    cnt = np.bincount(order[pos[hit]], minlength=sc.size)
    return cnt / float(samples.shape[0]), int((~hit).sum())


def ffbs(gr, V, L, K, rng):
    """K state sequences [K, L] from the posterior: float64 forward filter, backward sampling (dense: small graphs)."""
    V = np.asarray(V, dtype=np.float64)
    T = gr.dense()
    S1 = gr.S1
    A = np.full((L, S1), -np.inf)
    A[0] = gr.a + np.append(V[0], -np.inf)[gr.s2p]
    for n in range(1, L):
        A[n] = np.logaddexp.reduce(A[n - 1][:, None] + T, axis=0) + np.append(V[n], -np.inf)[gr.s2p]
    out = np.zeros((K, L), dtype=np.int64)
    j = np.full(K, gr.fin)
    for n in range(L - 1, -1, -1):
        x = A[n][None, :] + T[:, j].T  # [K, S1]
        p = np.exp(x - x.max(axis=1, keepdims=True))
        c = np.cumsum(p, axis=1)
        u = rng.random(K) * c[:, -1]
        j = np.minimum((c <= u[:, None]).sum(axis=1), S1 - 1)
        out[:, n] = j
    return out


def bernstein_bound(p, K, M, delta=1e-6):
    """The Bernstein rule: for M cells with true probabilities p and K independent samples, a correct sampler has every
    |p_hat - p| <= sqrt(2 p (1 - p) L / K) + 2 L / (3 K), L = ln(2 M / delta), with probability above 1 - delta (Bernstein's
    inequality and a union bound over the cells); + 1e-4 * p, the project's parity bar for posteriors, for the float32 alpha."""
    p = np.asarray(p, dtype=np.float64)
    Lg = np.log(2.0 * M / delta)
    return np.sqrt(2.0 * p * (1.0 - p) * Lg / K) + 2.0 * Lg / (3.0 * K) + 1e-4 * p


def bernstein_ratio(p_hat, p, K, M=None, delta=1e-6):
    """max over the cells of |p_hat - p| / bound: the rule holds when this is <= 1."""
    p = np.asarray(p, dtype=np.float64)
    M = p.size if M is None else M
    return float(np.max(np.abs(np.asarray(p_hat, dtype=np.float64) - p) / bernstein_bound(p, K, M, delta)))
