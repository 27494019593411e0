"""Test helper: NumPy restatement of the beam-pruned best-path lattices (include/markovmodels_amd.h, mm_lattice_f32) by the header's
definition, over the entry list (i, j, w) of arc_reference.fsm_entries -- the stored entries of T_hat in the caller's order, parallel
entries between two states kept apart.  dtype = float32 forms the through-score of every entry with the header's three adds in its
grouping and one subtraction, over tropical alpha / beta recursions in float32 (adds and a max: on inputs that are multiples of 1/16
every sum is exact, so the result does not depend on the order the device adds in and is the device's bit for bit); dtype = float64
is the same in double.  Plus a brute force for tiny graphs: every state sequence and every choice among parallel entries."""
from types import SimpleNamespace

import numpy as np

import arc_reference as ar


def system(f):
    """The entries of FSM f (weights as the device holds them: float32), grouped by destination and by source for the two
    recursions; alpha_hat [S1]; the phony self-loop's mask."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    w = w.astype(np.float32)
    pi = np.full(S1, -np.inf, dtype=np.float32)
    np.maximum.at(pi, np.asarray(f.alpha_idx, dtype=np.int64), np.asarray(f.alpha_val).astype(np.float32))

    def groups(key):
        order = np.argsort(key, kind="stable")
        ks = key[order]
        first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if ks.size else np.zeros(0, dtype=np.int64)
        return order, first, ks[first]

    return SimpleNamespace(i=i, j=j, w=w, S1=S1, pi=pi, phony=(i == S1 - 1) & (j == S1 - 1), by_dst=groups(j), by_src=groups(i))


def lhs_rows(s2p, P, V, L, N, S1, dt):
    """lhs_n [N + 1, S1] for the frames n = 1 .. N + 1 (row n - 1): C_hat . expand(V[:L])."""
    out = np.full((N + 1, S1), -np.inf, dtype=dt)
    if L > 0:
        out[:L, : S1 - 1] = np.asarray(V[:L], dtype=np.float32).astype(dt)[:, np.asarray(s2p)[: S1 - 1]]
    out[L:, S1 - 1] = 0
    return out


def _group_max(x, grp, S1, dt):
    order, first, keys = grp
    out = np.full(S1, -np.inf, dtype=dt)
    if first.size:
        out[keys] = np.maximum.reduceat(x[order], first)
    return out


def recursions(sy, s2p, P, V, L, N, dtype=np.float32):
    """The tropical alpha and beta recursions as mm_alpharecursion_f32 / mm_betarecursion_f32 export them, [N + 1, S1] each (row
    n - 1: frame n; beta_n excludes frame n's emission, beta_{N+1} = one), and lhs."""
    dt = np.dtype(dtype).type
    S1 = sy.S1
    w = sy.w.astype(dt)
    lhs = lhs_rows(s2p, P, V, L, N, S1, dt)
    A = np.empty((N + 1, S1), dtype=dt)
    Bm = np.empty((N + 1, S1), dtype=dt)
    with np.errstate(invalid="ignore"):
        A[0] = sy.pi.astype(dt) + lhs[0]
        for n in range(1, N + 1):
            A[n] = _group_max((w + A[n - 1][sy.i]).astype(dt), sy.by_dst, S1, dt) + lhs[n]
        Bm[N] = 0
        for n in range(N - 1, -1, -1):
            c = (lhs[n + 1] + Bm[n + 1]).astype(dt)
            Bm[n] = _group_max((w + c[sy.j]).astype(dt), sy.by_src, S1, dt)
    return A, Bm, lhs


def reference(f, s2p, P, V, L, N, beam, dtype=np.float32, sy=None):
    """One utterance: f an FSM, s2p [S] its pdfs, V [>= L, P], length L, N frames, beam a number.  Returns counts [N] int32, the
    records t / arc / score (row-major in t, ascending entry within a transition), best, the through-scores s [L, nnz] of every
    entry (NaN never; -inf where there is no path through it), and mu [N + 1, S1], the max-marginals alpha + beta - best."""
    dt = np.dtype(dtype).type
    sy = sy or system(f)
    A, Bm, lhs = recursions(sy, s2p, P, V, L, N, dtype)
    best = A[N, sy.S1 - 1]
    w = sy.w.astype(dt)
    nnz = sy.i.size
    counts = np.zeros(N, dtype=np.int32)
    s_all = np.full((L, nnz), -np.inf, dtype=dt)
    ts, arcs, scores = [], [], []
    live = bool(best > -np.inf) and bool(dt(beam) >= 0)
    with np.errstate(invalid="ignore"):
        mu = (A + Bm - best).astype(dt) if best > -np.inf else np.full_like(A, -np.inf)
        for t in range(L):
            x = ((A[t][sy.i] + w).astype(dt) + (lhs[t + 1][sy.j] + Bm[t + 1][sy.j]).astype(dt)).astype(dt)
            s = (x - best).astype(dt)
            finite = (x > -np.inf) & ~sy.phony
            s_all[t] = np.where(finite & bool(best > -np.inf), s, -np.inf)
            keep = finite & (s >= -dt(beam)) if live else np.zeros(nnz, dtype=bool)
            k = np.flatnonzero(keep)
            counts[t] = k.size
            ts.append(np.full(k.size, t, dtype=np.int64))
            arcs.append(k.astype(np.int32))
            scores.append(s[k])
    cat = lambda parts, dtp: np.concatenate(parts).astype(dtp) if parts else np.zeros(0, dtype=dtp)
    return SimpleNamespace(counts=counts, t=cat(ts, np.int64), arc=cat(arcs, np.int32), score=cat(scores, dt), best=best, s=s_all, mu=mu,
                           alpha=A, beta=Bm)


def batch_reference(fs, gs, V, lens, beams, dtype=np.float32):
    """Every utterance of a batch, and the concatenation the entry returns: counts [B, N], offsets [B * N + 1], arc, score, best [B]."""
    B, N = V.shape[0], V.shape[1]
    beams = np.broadcast_to(np.asarray(beams, dtype=np.float32), (B,))
    lens = np.full(B, N) if lens is None else np.asarray(lens)
    sys = {}
    refs = []
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), N))
        sy = sys.setdefault(id(fs[b]), system(fs[b]))
        refs.append(reference(fs[b], gs[b].state2pdf, gs[b].P, V[b], L, N, beams[b], dtype, sy))
    counts = np.stack([r.counts for r in refs])
    offsets = np.concatenate([[0], np.cumsum(counts.reshape(-1), dtype=np.int64)])
    return SimpleNamespace(counts=counts, offsets=offsets, arc=np.concatenate([r.arc for r in refs]), score=np.concatenate([r.score for r in refs]),
                           best=np.array([r.best for r in refs]), refs=refs)


def brute_force(f, s2p, P, V, L, N, beam):
    """By enumeration of every complete path of a tiny graph -- every state sequence s_1 .. s_L and every choice among parallel
    entries --, float64: through[t, k] = the greatest weight of a complete path that takes entry k at transition t (-inf: none), and
    the best weight.  (t, k) is in the lattice iff through[t, k] >= best - beam.  Returns (kept {(t, k): through - best}, best)."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    fs = S1 - 1
    w = w.astype(np.float32).astype(np.float64)
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    s2p = np.asarray(s2p)
    out_of = [[k for k in range(i.size) if i[k] == s and not (i[k] == fs and j[k] == fs)] for s in range(S1)]
    through = np.full((max(L, 1), i.size), -np.inf)
    best = [-np.inf]

    def walk(t, state, weight, taken):
        for k in out_of[state]:
            d = int(j[k])
            if t == L - 1:
                if d != fs:
                    continue
                total = weight + w[k]
                if total > -np.inf:
                    best[0] = max(best[0], total)
                    for tt, kk in enumerate(taken + [k]):
                        through[tt, kk] = max(through[tt, kk], total)
            elif d != fs:
                nw = weight + w[k] + Vd[t + 1, s2p[d]]
                if nw > -np.inf:
                    walk(t + 1, d, nw, taken + [k])

    if L > 0:
        for s, a in zip(np.asarray(f.alpha_idx, dtype=np.int64), np.asarray(f.alpha_val).astype(np.float32).astype(np.float64)):
            if s != fs and a + Vd[0, s2p[s]] > -np.inf:
                walk(0, int(s), a + Vd[0, s2p[s]], [])
    kept = {}
    if best[0] > -np.inf and beam >= 0:
        for t in range(L):
            for k in range(i.size):
                if through[t, k] > -np.inf and through[t, k] >= best[0] - beam:
                    kept[(t, k)] = through[t, k] - best[0]
    return kept, best[0]


def tau(N, alpha):
    """The rounding bound of a float32 through-score: 2 (N + 3) 2^-24 max|alpha| over the finite entries of the reference's alpha."""
    fin = np.abs(alpha[np.isfinite(alpha)])
    return 2.0 * (N + 3) * 2.0 ** -24 * float(fin.max() if fin.size else 0.0)


def compare_unrounded(got_arc_sets, got_scores, ref64, beam, N):
    """The bar of the unrounded case for one utterance: got_arc_sets[t] the kept entries of transition t, got_scores[t] their scores
    (same order), ref64 the float64 reference at the same beam.  An entry may differ from the reference only if its float64 score
    lies within tau of -beam; scores agree within tau.  Returns (excused, kept by the reference, tau)."""
    tol = tau(N, ref64.alpha)
    excused = 0
    for t in range(ref64.s.shape[0]):
        ref_keep = set(ref64.arc[ref64.t == t].tolist())
        got = set(int(k) for k in got_arc_sets[t])
        for k in ref_keep ^ got:
            assert abs(float(ref64.s[t, k]) + beam) <= tol, (t, k, float(ref64.s[t, k]), beam, tol)
            excused += 1
        for k, s in zip(got_arc_sets[t], got_scores[t]):
            assert abs(float(s) - float(ref64.s[t, int(k)])) <= tol, (t, int(k), float(s), float(ref64.s[t, int(k)]), tol)
    return excused, int(ref64.arc.size), tol
