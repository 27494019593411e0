"""Test helper: float64 reference values of the expected arc-class cost and its gradient (include/markovmodels_amd.h,
mm_classcost_f32).  Like scored_reference it does not go through the C oracle: a log-domain forward-backward in NumPy over the
entry list (i, j, w) of arc_reference.fsm_entries gives alpha and beta; r and s follow the header's recursions, carried centred as
the kernels carry them, with the class cost A[t, cls[k]] on every entry k taken at transition t (nothing for class -1, for the
phony self-loop and for t >= L) beside the pdf cost D of cost_reference.  A float32 mode of the same recursion (what float32
arithmetic alone costs: the source of the gradient's absolute bar), and a brute-force enumeration of every path of a tiny graph."""
import itertools

import numpy as np

import arc_reference as ar
from cost_reference import _cond_mean, _segments
from weighted_reference import _seg_lse

# The absolute part `a` of the gradient's bar |grad - grad_ref| <= 1e-4 |grad_ref| + a * G_b, G_b = max |grad_ref,b|.
# Measured on the CPU, before any kernel was judged: `reference(..., dtype=np.float32)` (r', t' and every sum over them in float32,
# the offsets in float64) against `reference(...)` in float64 on the inputs of tests/test_gpu_classcost.py
# (tools/measure_classcost_floor.py prints the table; profiles/classcost_floor.json keeps it).  Worst |grad_f32 - grad_f64| / G_b:
#   40-state random graph, T = 30, one class per entry / destination pdf / sparse   5.2e-7 / 5.5e-7 / 5.5e-7
#   denominator graph of 600 states, T = 30 (the streamed instance)                9.1e-8 .. 3.7e-7
#   12 500 states, T = 40 (vectors in global memory)                               4.7e-7
#   wide rows (hundreds of arcs per row), T = 30                                   2.0e-7
#   four distinct graphs with their own classes, T = 40                            1.07e-6
#   C = cap classes on a 20-state graph, T = 10                                    4.0e-7
# each with D given and with D NULL; the worst is the left-to-right HMM of the four distinct graphs with D given.
# a = min(10 x the worst, 1e-4): the factor is for what the NumPy run does not have (the hardware's exp2 / log2 approximations in
# alpha~ and beta~, the kernel's reduction order, float32 partial sums per pdf), as in cost_reference.py.
GRAD_F32_FLOOR = 1.07e-6
GRAD_ABS_A = min(10 * GRAD_F32_FLOOR, 1e-4)


def entry_costs(f, cls, A, L, N):
    """ac [nnz, N]: what entry k costs at transition t."""
    i, j, _ = ar.fsm_entries(f)
    cls = np.asarray(cls, dtype=np.int64)
    ac = np.zeros((i.size, N))
    fs = f.colptr.size - 2
    costed = (cls >= 0) & ~((i == fs) & (j == fs))
    T = min(L, N)
    ac[costed, :T] = np.asarray(A, dtype=np.float64)[:T, cls[costed]].T
    return ac


def _alpha_beta(g, f, V, L, N):
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[ar._s2p_full(g)]  # [S1, N + 1]
    Al = np.full((S1, N + 1), -np.inf)
    Bm = np.full((S1, N + 1), -np.inf)
    with np.errstate(invalid="ignore"):
        Al[:, 0] = a + lhs[:, 0]
        for n in range(N):
            Al[:, n + 1] = _seg_lse(Al[i, n] + w, j, S1) + lhs[:, n + 1]
        Bm[:, N] = 0.0
        for n in range(N - 1, -1, -1):
            Bm[:, n] = _seg_lse(w + lhs[j, n + 1] + Bm[j, n + 1], i, S1)
        logZ = float(ar._lse(Al[:, 0] + Bm[:, 0]))
    return i, j, w, S1, lhs, Al, Bm, logZ


def reference(g, f, cls, V, A, D, L, N, dtype=np.float64):
    """risk, grad [N, P], gamma [N, P], log Z and the mass sum gamma |D| + sum_{t<L} xi |A| (the risk's bar) of one utterance:
    cls [nnz] in f's CSC entry order, V [>= L, P], A [>= L, C], D [>= L, P] or None, length L, N frames.  r' = r - O and
    t' = D + s - Q with the float64 offsets O_n (filtering means of r' of the frames before n) and Q_n (posterior means of t' of
    the frames after n); the class cost enters both conditional means before the offsets are taken.  dtype = float32 rounds the
    weights, r', t', the class term and every sum over them to float32: the float32 floor of the recursion."""
    dt = np.dtype(dtype).type
    i, j, w, S1, lhs, Al, Bm, logZ = _alpha_beta(g, f, V, L, N)
    s2p = ar._s2p_full(g)
    P = g.P
    grad, gamma = np.zeros((N, P)), np.zeros((N, P))
    if not np.isfinite(logZ):
        return 0.0, grad, gamma, -np.inf, 0.0
    ac64 = entry_costs(f, cls, A, L, N)
    ac = ac64.astype(dt)
    cs64 = np.zeros((P + 1, N + 1))
    if D is not None:
        cs64[:P, :L] = np.asarray(D, dtype=np.float64)[:L].T
    cs64 = cs64[s2p]
    cs = cs64.astype(dt)  # [S1, N+1] the pdf cost of a state at a frame
    with np.errstate(invalid="ignore"):
        post = np.exp(Al + Bm - logZ)  # [S1, N+1] state posteriors
        filt = np.exp(Al - ar._lse(Al, axis=0)[None, :])
        xk = np.exp(Al[i, :N] + w[:, None] + lhs[j, 1 : N + 1] + Bm[j, 1 : N + 1] - logZ)  # [nnz, N] entry posteriors
    post = np.where(np.isfinite(post), post, 0.0)
    filt = np.where(np.isfinite(filt), filt, 0.0)
    xk = np.where(np.isfinite(xk), xk, 0.0)
    mass = float(np.sum(post[:, :N] * np.abs(cs64[:, :N])) + np.sum(xk * np.abs(ac64)))
    # forward: r' and O
    of, ff, kf = _segments(j, S1)
    i_f, w_f = i[of], w[of]
    r = np.zeros((S1, N + 1), dtype=dt)
    O = np.zeros(N + 1)
    r[:, 0] = cs[:, 0]
    for n in range(1, N + 1):
        mu = float(np.sum(filt[:, n - 1].astype(dt) * r[:, n - 1], dtype=dt))
        O[n] = O[n - 1] + mu
        rb = _cond_mean(Al[i_f, n - 1] + w_f, (r[i_f, n - 1] + ac[of, n - 1]).astype(dt), ff, kf, S1, dt)
        r[:, n] = np.where(np.isfinite(Al[:, n]), cs[:, n] + rb - dt(mu), 0).astype(dt)
    risk = float(r[S1 - 1, N]) + O[N]
    # backward: t' = D + s' and Q
    ob, fb, kb = _segments(i, S1)
    j_b, w_b = j[ob], w[ob]
    t = np.zeros((S1, N + 1), dtype=dt)  # t'_{N+1} = 0
    s = np.zeros((S1, N + 1), dtype=dt)
    Q = np.zeros(N + 1)  # Q[n]: s_n = s'_n + Q[n]
    for n in range(N - 1, -1, -1):
        mu = float(np.sum(post[:, n + 1].astype(dt) * t[:, n + 1], dtype=dt)) if n + 1 < N else 0.0
        Q[n] = (Q[n + 1] if n + 1 < N else 0.0) + mu
        sb = _cond_mean(w_b + lhs[j_b, n + 1] + Bm[j_b, n + 1], (t[j_b, n + 1] + ac[ob, n]).astype(dt), fb, kb, S1, dt)
        s[:, n] = np.where(np.isfinite(Bm[:, n]), sb - dt(mu), 0).astype(dt)
        t[:, n] = cs[:, n] + s[:, n]
    off = (O[:N] + Q[:N] - risk).astype(dt)
    d = (r[:, :N] + s[:, :N] + off[None, :]).astype(np.float64)  # E[A | s_n = j] - risk
    qd = post[:, :N] * d
    for p in range(P):
        m = s2p == p
        gamma[:, p] = post[m, :N].sum(axis=0)
        grad[:, p] = qd[m].sum(axis=0)
    grad[L:] = 0
    gamma[L:] = 0
    return risk, grad, gamma, logZ, mass


def risk_only(g, f, cls, V, A, D, L, N):
    """The float64 risk alone: what the central differences perturb."""
    return reference(g, f, cls, V, A, D, L, N)[0]


def enumerate_paths(g, f, cls, V, A, D, L, N):
    """risk, grad, gamma, log Z by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only).  Parallel entries
    between two states are costed one by one and share the pair's posterior in proportion to their weights: a path through the
    pair pays their weighted mean at that transition.  grad is the covariance of the path's cost with the indicator
    [pdf(s_n) = p]."""
    i, j, w = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    S1, P = s2p.size, g.P
    ac = entry_costs(f, cls, A, L, N)
    T = np.full((S1, S1), -np.inf)
    np.logaddexp.at(T, (i, j), w)
    pc = np.zeros((N, S1, S1))  # the pair's cost at transition n
    with np.errstate(invalid="ignore"):
        share = np.where(np.isfinite(w), np.exp(w - T[i, j]), 0.0)
    for n in range(N):
        np.add.at(pc[n], (i, j), share * ac[:, n])
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[s2p]
    cs = np.zeros((P + 1, N + 1))
    if D is not None:
        cs[:P, :L] = np.asarray(D, dtype=np.float64)[:L].T
    cs = cs[s2p]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    with np.errstate(invalid="ignore"):
        lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
        Apath = cs[paths[:, 0], 0].copy()
        for n in range(N):
            lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
            Apath += cs[paths[:, n + 1], n + 1] + pc[n][paths[:, n], paths[:, n + 1]]
    lw = np.where(np.isnan(lw), -np.inf, lw)
    logZ = ar._lse(lw)
    grad, gamma = np.zeros((N, P)), np.zeros((N, P))
    if not np.isfinite(logZ):
        return 0.0, grad, gamma, -np.inf
    pr = np.exp(lw - logZ)
    risk = float(np.sum(pr * Apath))
    for n in range(L):
        pdf = s2p[paths[:, n]]
        for p in range(P):
            m = pdf == p
            gamma[n, p] = pr[m].sum()
            grad[n, p] = np.sum(pr[m] * (Apath[m] - risk))
    return risk, grad, gamma, float(logZ)


def check(risk, grad, ttl, ref, A, D, L, a=None):
    """The accuracy bars of risk, grad and ttl against a float64 reference (one utterance; `ref` what reference() returns); gamma
    has check_gamma of tests/test_gpu_parity.py.
        risk:  |risk - ref| <= 1e-4 (sum gamma |D| + sum xi |A|) + 1e-6 L max(|A|, |D|)   (the maxima over the rows that are read)
        grad:  |grad - ref| <= 1e-4 |ref| + a G_b,  G_b = max |grad_ref,b|
        ttl:   as cost_reference.check
    Returns the measured (risk error / its bar, worst gradient error / G_b)."""
    a = GRAD_ABS_A if a is None else a
    risk_ref, grad_ref, gamma_ref, logz_ref, mass = ref
    grad = np.asarray(grad, dtype=np.float64)
    if not np.isfinite(logz_ref):
        assert risk == 0 and (grad == 0).all() and np.isneginf(ttl)
        return 0.0, 0.0
    amax = float(np.abs(np.asarray(A, dtype=np.float64)[:L]).max()) if L > 0 else 0.0
    dmax = float(np.abs(np.asarray(D, dtype=np.float64)[:L]).max()) if (D is not None and L > 0) else 0.0
    bar = 1e-4 * mass + 1e-6 * L * max(amax, dmax)
    assert np.isfinite(risk) and abs(float(risk) - risk_ref) <= bar, (float(risk), risk_ref, bar)
    assert (grad[L:] == 0).all(), "frames beyond the sequence length must be exact zeros"
    G = float(np.abs(grad_ref).max())
    err = np.abs(grad - grad_ref)
    assert np.isfinite(grad).all() and (err <= 1e-4 * np.abs(grad_ref) + a * G).all(), (float(err.max()), G, float(err.max() / max(G, 1e-300)))
    assert np.isclose(ttl, logz_ref, rtol=1e-5, atol=1e-5 * max(1.0, abs(logz_ref)) + 1e-4), (ttl, logz_ref)
    return abs(float(risk) - risk_ref) / max(bar, 1e-300), float(err.max() / max(G, 1e-300))
