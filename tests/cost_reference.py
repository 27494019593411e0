"""Test helper: float64 reference values of the expected path cost and its gradient (include/markovmodels_amd.h,
mm_expectedcost_f32) from the C oracle's alpha / beta in log space, a float32 mode of the same centred recursion (what float32
arithmetic alone costs: the source of the gradient's absolute bar), and a brute-force enumeration of every path of a tiny graph."""
import itertools

import numpy as np

import arc_reference as ar
import graphs

# The absolute part `a` of the gradient's bar |grad - grad_ref| <= 1e-4 |grad_ref| + a * G_b, G_b = max |grad_ref,b|.
# Measured on the CPU, before any kernel was judged: `reference(..., dtype=np.float32)` (the centred recursion with r and s
# carried in float32, the offsets in float64) against `reference(...)` in float64 on the inputs of tests/test_gpu_expectedcost.py
# (tools/measure_cost_floor.py prints the table; profiles/expectedcost_floor.json keeps it).  Worst |grad_f32 - grad_f64| / G_b:
#   40-state random graph, T = 30                     3.8e-7
#   config 3 graph, T = 1500, randn, sMBR cost        2.5e-7
#   config 3 graph, T = 500, log_softmax(10 x)        2.1e-6
#   WSJ denominator / numerator, T = 700              6.7e-7 / 3.0e-6
#   four distinct graphs / 12 500 states, T = 40      1.6e-6 / 1.2e-6
#   the cases of tests/test_gpu_itemform.py (70 000 states, the boundaries, wide rows), T <= 60   <= 3.0e-7
# a = 10 x the worst (the factor is for what the NumPy run does not have: the hardware's exp2 / log2 approximations in alpha~ and
# beta~, the kernel's reduction order, float32 partial sums per pdf), capped at the project's own 1e-4.
GRAD_F32_FLOOR = 3.01e-6
GRAD_ABS_A = min(10 * GRAD_F32_FLOOR, 1e-4)


def _segments(key, n):
    """Arcs sorted by `key`: the order, the first arc of every non-empty segment, the segments' keys."""
    order = np.argsort(key, kind="stable")
    ks = key[order]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if ks.size else np.zeros(0, dtype=np.int64)
    return order, first, ks[first] if ks.size else ks


def _cond_mean(t, val, first, seg_keys, n, dt):
    """Per segment: sum_k softmax(t)_k val_k (0 for a segment without weight), scattered to [n].  t float64 log weights; the
    weights are rounded to `dt` and the sums run in `dt`."""
    out = np.zeros(n, dtype=dt)
    if t.size == 0:
        return out
    m = np.maximum.reduceat(t, first)
    m = np.where(np.isfinite(m), m, 0.0)
    cnt = np.diff(np.concatenate([first, [t.size]]))
    e = np.exp(t - np.repeat(m, cnt)).astype(dt)
    den = np.add.reduceat(e, first)
    num = np.add.reduceat(e * val, first)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[seg_keys] = np.where(den > 0, num / den, 0).astype(dt)
    return out


def reference(o, oc, g, f, V, cost, L, N, dtype=np.float64):
    """risk, grad [N, P], gamma [N, P] and log Z of one utterance: V, cost [>= L, P], length L, N frames.  alpha and beta from the
    C oracle in float64 log space; r and s by the header's recursions with the conditional probabilities taken from those alpha /
    beta.  r and s are carried centred, as the kernels carry them: r'_n = r_n - O_n and t'_n = cost_n + s_n - Q_n with the
    float64 offsets O_n (filtering means of r' of the frames before n) and Q_n (posterior means of t' of the frames after n).
    dtype = float32 rounds the weights, r', t' and every sum over them to float32: the float32 floor of the recursion."""
    dt = np.dtype(dtype).type
    Vhat = ar.expand_log(V, L, N)
    _, _, A, Bm = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64, want_ab=True)
    i, j, w = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    S1, P = s2p.size, g.P
    lhs = Vhat[s2p]
    with np.errstate(invalid="ignore"):
        logZ = ar._lse(A[:, 0] + Bm[:, 0])
    grad, gamma = np.zeros((N, P)), np.zeros((N, P))
    if not np.isfinite(logZ):
        return 0.0, grad, gamma, -np.inf
    cs = np.zeros((P + 1, N + 1))
    cs[:P, :L] = np.asarray(cost, dtype=np.float64)[:L].T
    cs = cs[s2p].astype(dt)  # [S1, N+1] the cost of a state at a frame
    with np.errstate(invalid="ignore"):
        post = np.exp(A + Bm - logZ)  # [S1, N+1] state posteriors
        filt = np.exp(A - ar._lse(A, axis=0)[None, :])
    post = np.where(np.isfinite(post), post, 0.0)
    filt = np.where(np.isfinite(filt), filt, 0.0)
    # forward: r' and O
    of, ff, kf = _segments(j, S1)
    i_f, j_f, w_f = i[of], j[of], w[of]
    r = np.zeros((S1, N + 1), dtype=dt)
    O = np.zeros(N + 1)
    r[:, 0] = cs[:, 0]
    for n in range(1, N + 1):
        mu = float(np.sum(filt[:, n - 1].astype(dt) * r[:, n - 1], dtype=dt))
        O[n] = O[n - 1] + mu
        rb = _cond_mean(A[i_f, n - 1] + w_f, r[i_f, n - 1], ff, kf, S1, dt)
        r[:, n] = np.where(np.isfinite(A[:, n]), cs[:, n] + rb - dt(mu), 0).astype(dt)
    risk = float(r[S1 - 1, N]) + O[N]
    # backward: t' = cost + s' and Q
    ob, fb, kb = _segments(i, S1)
    i_b, j_b, w_b = i[ob], j[ob], w[ob]
    t = np.zeros((S1, N + 1), dtype=dt)  # t'_{N+1} = 0
    s = np.zeros((S1, N + 1), dtype=dt)
    Q = np.zeros(N + 1)  # Q[n]: s_n = s'_n + Q[n]
    for n in range(N - 1, -1, -1):
        mu = float(np.sum(post[:, n + 1].astype(dt) * t[:, n + 1], dtype=dt)) if n + 1 < N else 0.0
        Q[n] = (Q[n + 1] if n + 1 < N else 0.0) + mu
        sb = _cond_mean(w_b + lhs[j_b, n + 1] + Bm[j_b, n + 1], t[j_b, n + 1], fb, kb, S1, dt)
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
    return risk, grad, gamma, float(logZ)


def enumerate_paths(g, f, V, cost, L, N):
    """risk, grad, gamma, log Z by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only): grad is the
    covariance of the path's cost with the indicator [pdf(s_n) = p]."""
    i, j, w = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    S1, P = s2p.size, g.P
    T = np.full((S1, S1), -np.inf)
    T[i, j] = w
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[s2p]
    cs = np.zeros((P + 1, N + 1))
    cs[:P, :L] = np.asarray(cost, dtype=np.float64)[:L].T
    cs = cs[s2p]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
    Apath = cs[paths[:, 0], 0].copy()
    for n in range(N):
        lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
        Apath += cs[paths[:, n + 1], n + 1]
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


def check(risk, grad, ttl, ref, cost, L, a=GRAD_ABS_A):
    """The accuracy bars of risk, grad and ttl against a float64 reference (one utterance); gamma has check_gamma of
    tests/test_gpu_parity.py.  Returns the measured (risk error / its bar, worst gradient error / G_b)."""
    risk_ref, grad_ref, gamma_ref, logz_ref = ref
    grad = np.asarray(grad, dtype=np.float64)
    if not np.isfinite(logz_ref):
        assert risk == 0 and (grad == 0).all() and np.isneginf(ttl)
        return 0.0, 0.0
    c = np.abs(np.asarray(cost, dtype=np.float64)[:L])
    bar = 1e-4 * float(np.sum(gamma_ref[:L] * c)) + 1e-6 * L * (float(c.max()) if c.size else 0.0)
    assert np.isfinite(risk) and abs(float(risk) - risk_ref) <= bar, (float(risk), risk_ref, bar)
    assert (grad[L:] == 0).all(), "frames beyond the sequence length must be exact zeros"
    G = float(np.abs(grad_ref).max())
    err = np.abs(grad - grad_ref)
    assert np.isfinite(grad).all() and (err <= 1e-4 * np.abs(grad_ref) + a * G).all(), (float(err.max()), G, float(err.max() / max(G, 1e-300)))
    assert np.isclose(ttl, logz_ref, rtol=1e-5, atol=1e-5 * max(1.0, abs(logz_ref)) + 1e-4), (ttl, logz_ref)
    return abs(float(risk) - risk_ref) / max(bar, 1e-300), float(err.max() / max(G, 1e-300))
