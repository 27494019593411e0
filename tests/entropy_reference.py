"""Test helper: float64 reference values of the posterior path entropy and its gradient (include/markovmodels_amd.h,
mm_pathentropy_f32) from the C oracle's alpha / beta in log space, a float32 mode of the same centred recursion (what float32
arithmetic alone costs: the source of the absolute parts of the bars), and a brute-force enumeration of every path of a tiny graph."""
import itertools

import numpy as np

import arc_reference as ar
import graphs
from cost_reference import _segments

# The bars (one utterance, against the float64 reference):
#     |H - H_ref|       <= 1e-4 H_ref + h * len
#     |grad - grad_ref| <= 1e-4 |grad_ref| + a * G_b,      G_b = max |grad_ref,b|
# h (nats per frame) and a were measured on the CPU, before any kernel was judged: `reference(..., dtype=np.float32)` (the centred
# recursion with the weights, Hf', Hb' and their sums in float32, the offsets in float64, the frame's mean taken out of grad as
# the kernel takes it out) against `reference(...)` in float64 on the inputs of tests/test_gpu_pathentropy.py
# (tools/measure_entropy_floor.py prints the table; profiles/pathentropy_floor.json keeps it).  Worst over the checked utterances:
#                                                   |H_f32 - H_f64| / len    |grad_f32 - grad_f64| / G_b
#   40-state random graph, T = 30                          1.7e-8                   1.4e-7
#   four distinct graphs, T = 40                           8.6e-9                   3.7e-7
#   config 3 graph, T = 1500, randn                        2.3e-9                   2.9e-7
#   config 3 graph, T = 500, log_softmax(10 x)             5.5e-9                   5.1e-7
#   WSJ denominator, T = 700                               4.4e-9                   1.0e-7
#   WSJ numerator, T = 700                                 1.8e-8                   5.2e-6
#   12 500 states, T = 40                                  1.9e-8                   8.3e-8
# h = 10 x the worst of the first column, a = min(10 x the worst of the second, 1e-4): the factor is for what the NumPy run does
# not have -- the hardware's exp2 / log2 / reciprocal approximations, the kernel's reduction order, float32 partial sums per pdf.
H_F32_FLOOR = 1.88e-8
GRAD_F32_FLOOR = 5.22e-6
H_ABS_PER_FRAME = 10 * H_F32_FLOOR
GRAD_ABS_A = min(10 * GRAD_F32_FLOOR, 1e-4)


def _row_value(t, val, first, seg_keys, n, dt):
    """Per segment, with P_k = softmax(t)_k: sum_k P_k (val_k - ln P_k) = [sum_k e_k (val_k - d_k)] / den + ln den, d_k = t_k - max,
    e_k = exp(d_k), den = sum e_k (0 for a segment without weight; a term without weight is 0: 0 ln 0 := 0), scattered to [n].
    t float64 log weights; d, e and the sums are rounded to / run in `dt`."""
    out = np.zeros(n, dtype=dt)
    if t.size == 0:
        return out
    m = np.maximum.reduceat(t, first)
    m = np.where(np.isfinite(m), m, 0.0)
    cnt = np.diff(np.concatenate([first, [t.size]]))
    d = t - np.repeat(m, cnt)
    e = np.exp(d).astype(dt)
    with np.errstate(invalid="ignore"):
        term = np.where(e > 0, e * (val - np.where(e > 0, d, 0.0).astype(dt)), 0).astype(dt)
    den = np.add.reduceat(e, first)
    num = np.add.reduceat(term, first)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[seg_keys] = np.where(den > 0, num / den + np.log(den), 0).astype(dt)
    return out


def reference(o, oc, g, f, V, L, N, dtype=np.float64, demean=None, want_mean=False):
    """H, grad [N, P], gamma [N, P] and log Z of one utterance: V [>= L, P], length L, N frames.  alpha and beta from the C oracle
    in float64 log space; Hf and Hb by the header's recursions with the conditional probabilities taken from those alpha / beta,
    carried centred as the kernels carry them: Hf'_n = Hf_n - O_n, Hb'_n = Hb_n - Q_n with the float64 offsets O_n (filtering means
    of Hf' of the frames before n) and Q_n (posterior means of Hb' of the frames after n).  dtype = float32 rounds the weights, Hf',
    Hb' and every sum over them to float32: the float32 floor of the recursion.  demean (default: in the float32 mode only) takes
    the frame's posterior mean of the bracket out of grad, as the kernel does; in exact arithmetic that mean is zero, and the
    float64 mode leaves it in so that the tests see it.  want_mean: also return the largest |mean| over the frames."""
    dt = np.dtype(dtype).type
    demean = (dt is np.float32) if demean is None else demean
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
        return (0.0, grad, gamma, -np.inf) + ((0.0,) if want_mean else ())
    with np.errstate(invalid="ignore"):
        lq = A + Bm - logZ  # [S1, N+1] log state posteriors
        post = np.exp(lq)
        filt = np.exp(A - ar._lse(A, axis=0)[None, :])
    post = np.where(np.isfinite(post), post, 0.0)
    filt = np.where(np.isfinite(filt), filt, 0.0)
    # forward: Hf' and O
    of, ff, kf = _segments(j, S1)
    i_f, w_f = i[of], w[of]
    Hf = np.zeros((S1, N + 1), dtype=dt)
    O = np.zeros(N + 1)
    for n in range(1, N + 1):
        mu = float(np.sum(filt[:, n - 1].astype(dt) * Hf[:, n - 1], dtype=dt))
        O[n] = O[n - 1] + mu
        hb = _row_value(A[i_f, n - 1] + w_f, Hf[i_f, n - 1], ff, kf, S1, dt)
        Hf[:, n] = np.where(np.isfinite(A[:, n]), hb - dt(mu), 0).astype(dt)
    H = float(Hf[S1 - 1, N]) + O[N]
    # backward: Hb' and Q
    ob, fb, kb = _segments(i, S1)
    j_b, w_b = j[ob], w[ob]
    Hb = np.zeros((S1, N + 1), dtype=dt)  # Hb'_{N+1} = 0
    Q = np.zeros(N + 1)  # Q[n]: Hb_n = Hb'_n + Q[n]
    for n in range(N - 1, -1, -1):
        mu = float(np.sum(post[:, n + 1].astype(dt) * Hb[:, n + 1], dtype=dt)) if n + 1 < N else 0.0
        Q[n] = Q[n + 1] + mu
        sb = _row_value(w_b + lhs[j_b, n + 1] + Bm[j_b, n + 1], Hb[j_b, n + 1], fb, kb, S1, dt)
        Hb[:, n] = np.where(np.isfinite(Bm[:, n]), sb - dt(mu), 0).astype(dt)
    off = (O[:N] + Q[:N] - H).astype(dt)
    lqd = np.where(post[:, :N] > 0, lq[:, :N], 0.0).astype(dt)
    d = (Hf[:, :N] + Hb[:, :N] + off[None, :] - lqd).astype(np.float64)  # Hf + Hb - ln q - H
    qd = np.where(post[:, :N] > 0, post[:, :N] * d, 0.0)
    mean = qd.sum(axis=0) / np.maximum(post[:, :N].sum(axis=0), 1e-300)  # zero in exact arithmetic (chain rule)
    if demean:
        qd = qd - post[:, :N] * mean[None, :]
    for p in range(P):
        m = s2p == p
        gamma[:, p] = post[m, :N].sum(axis=0)
        grad[:, p] = qd[m].sum(axis=0)
    grad[L:] = 0
    gamma[L:] = 0
    return (H, grad, gamma, float(logZ)) + ((float(np.abs(mean[:L]).max()) if L else 0.0,) if want_mean else ())


def enumerate_paths(g, f, V, L, N):
    """H, grad, gamma, log Z by brute force over every state sequence s_1 .. s_{N+1} (tiny graphs only): H = -sum P ln P, grad
    minus the covariance of ln P(path) with the indicator [pdf(s_n) = p]."""
    i, j, w = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    S1, P = s2p.size, g.P
    T = np.full((S1, S1), -np.inf)
    T[i, j] = w
    a = np.full(S1, -np.inf)
    a[np.asarray(f.alpha_idx)] = np.asarray(f.alpha_val, dtype=np.float64)
    lhs = ar.expand_log(V, L, N)[s2p]
    paths = np.array(list(itertools.product(range(S1), repeat=N + 1)))
    lw = a[paths[:, 0]] + lhs[paths[:, 0], 0]
    for n in range(N):
        lw = lw + T[paths[:, n], paths[:, n + 1]] + lhs[paths[:, n + 1], n + 1]
    logZ = ar._lse(lw)
    grad, gamma = np.zeros((N, P)), np.zeros((N, P))
    if not np.isfinite(logZ):
        return 0.0, grad, gamma, -np.inf
    live = np.isfinite(lw)
    paths, lp = paths[live], lw[live] - logZ
    pr = np.exp(lp)
    H = float(-np.sum(pr * lp))
    for n in range(L):
        pdf = s2p[paths[:, n]]
        for p in range(P):
            m = pdf == p
            gamma[n, p] = pr[m].sum()
            grad[n, p] = -np.sum(pr[m] * (lp[m] + H))
    return H, grad, gamma, float(logZ)


def assert_inputs_test_something(ref, L):
    """No test passes on nothing: an utterance of 20 frames or more that has a path has at least a nat of entropy and a gradient."""
    H_ref, grad_ref, _, logz_ref = ref
    if L >= 20 and np.isfinite(logz_ref):
        assert H_ref >= 1.0, H_ref
        assert np.abs(grad_ref).max() > 0


def check(H, grad, ttl, ref, L, h=None, a=None, label=""):
    """The accuracy bars of entropy, grad and ttl against a float64 reference (one utterance); gamma has check_gamma of
    tests/test_gpu_parity.py.  grad may be None (a value-only call).  Prints the measured figures over their bars, then asserts
    them; returns (entropy error / its bar, worst gradient error / G_b)."""
    h = H_ABS_PER_FRAME if h is None else h
    a = GRAD_ABS_A if a is None else a
    H_ref, grad_ref, gamma_ref, logz_ref = ref
    assert_inputs_test_something(ref, L)
    if not np.isfinite(logz_ref):
        print(f"{label}: len {L}, no accepting path")
        assert H == 0 and np.isneginf(ttl) and (grad is None or (np.asarray(grad) == 0).all())
        return 0.0, 0.0
    bar = 1e-4 * H_ref + h * L
    he = abs(float(H) - H_ref)
    G = float(np.abs(grad_ref).max())
    err = None if grad is None else np.abs(np.asarray(grad, dtype=np.float64) - grad_ref)
    ge = 0.0 if err is None else float(np.nanmax(err) / max(G, 1e-300))
    over = 0.0 if err is None else float(np.nanmax(err / np.maximum(1e-4 * np.abs(grad_ref) + a * G, 1e-300)))
    print(f"{label}: len {L}, H {float(H):.7g} (ref {H_ref:.7g}, |error| {he:.3g}, bar {bar:.3g}, error / bar {he / max(bar, 1e-300):.3g}), "
          f"max |grad error| / G {ge:.3g} (a = {a:.3g}, G = {G:.3g}, worst error / bar {over:.3g})")
    assert np.isfinite(H) and H >= 0 and he <= bar, (float(H), H_ref, bar)
    assert np.isclose(ttl, logz_ref, rtol=1e-5, atol=1e-5 * max(1.0, abs(logz_ref)) + 1e-4), (ttl, logz_ref)
    if grad is not None:
        grad = np.asarray(grad, dtype=np.float64)
        assert (grad[L:] == 0).all(), "frames beyond the sequence length must be exact zeros"
        assert np.isfinite(grad).all() and (err <= 1e-4 * np.abs(grad_ref) + a * G).all(), (float(err.max()), G, ge)
    return he / max(bar, 1e-300), ge
