"""Test helper: NumPy float64 restatement of the lattice posteriors (include/markovmodels_amd.h, mm_latticeposteriors_f32) by the
header's definition, over a record list -- offsets [B * N + 1], arc [nrec], extra [nrec] or None -- and the entry lists of
lattice_reference.system.  The recursions are plain log-sum-exp accumulations in double (np.logaddexp.at), the posteriors are
normalised by logz itself (that a cell's posteriors sum to 1 is then a property to check, not one built in).  What the header says
of doctored input is restated too: entry indices outside the FSM and the phony self-loop are dead records, cells are clamped into
[0, nrec] and made non-decreasing, lens into [0, N].  Plus a brute force for tiny graphs: every lattice path, one record per
transition, every choice among parallel entries."""
from types import SimpleNamespace

import numpy as np

import lattice_reference as lr

NINF = -np.inf


def cells(offsets, nrec, b, N):
    """[(lo, hi)] of the N cells of utterance b, as the entry clamps them."""
    out = []
    for t in range(N):
        lo = min(max(int(offsets[b * N + t]), 0), nrec)
        hi = min(max(int(offsets[b * N + t + 1]), lo), nrec)
        out.append((lo, hi))
    return out


def _live(sy, k):
    """Which records name an entry of the FSM that is not the phony self-loop."""
    ok = (k >= 0) & (k < sy.i.size)
    ok[ok] &= ~sy.phony[k[ok]]
    return ok


def utterance(sy, s2p, P, V, L, N, cl, arc, extra, post, gamma):
    """One utterance: fills post[lo:hi] of its cells and gamma [N, P]; returns logz."""
    S1, f = sy.S1, sy.S1 - 1
    w = sy.w.astype(np.float64)
    lhs = lr.lhs_rows(s2p, P, V, L, N, S1, np.float64)
    s2p = np.asarray(s2p)
    for lo, hi in cl:
        post[lo:hi] = NINF
    if L == 0:
        return NINF
    recs = []
    with np.errstate(invalid="ignore"):
        a = sy.pi.astype(np.float64) + lhs[0]
        for t in range(L):
            lo, hi = cl[t]
            k = arc[lo:hi].astype(np.int64)
            ok = _live(sy, k)
            r = np.arange(lo, hi)[ok]
            k = k[ok]
            i, j = sy.i[k], sy.j[k]
            ex = extra[r].astype(np.float64) if extra is not None else np.zeros(r.size)
            wz = w[k] + ex + lhs[t + 1][j]
            x = a[i] + wz
            a = np.full(S1, NINF)
            np.logaddexp.at(a, j, x)
            recs.append((r, i, j, wz, x))
        logz = float(a[f])
        if not logz > NINF:
            return NINF
        bv = np.full(S1, NINF)
        bv[f] = 0.0
        for t in range(L - 1, -1, -1):
            r, i, j, wz, x = recs[t]
            y = x + bv[j]
            post[r] = np.where(y > NINF, y - logz, NINF)
            z = wz + bv[j]
            bv = np.full(S1, NINF)
            np.logaddexp.at(bv, i, z)
            real = i < S1 - 1
            np.add.at(gamma[t], s2p[i[real]], np.exp(post[r][real]))
    return logz


def reference(fs, gs, V, lens, offsets, arc, extra=None, nrec=None):
    """The batch: post [nrec] (NaN where no cell covers a record: the entry does not write there), logz [B], gamma [B, N, P], all
    float64.  fs / gs: the FSM and the GraphSpec-like (state2pdf, P) of every utterance."""
    V = np.asarray(V, dtype=np.float32)
    B, N, P = V.shape
    arc = np.asarray(arc)
    nrec = arc.size if nrec is None else int(nrec)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.full(B, N) if lens is None else np.asarray(lens)
    post = np.full(nrec, np.nan)
    logz = np.full(B, NINF)
    gamma = np.zeros((B, N, P))
    sys = {}
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), N))
        sy = sys.setdefault(id(fs[b]), lr.system(fs[b]))
        logz[b] = utterance(sy, gs[b].state2pdf, gs[b].P, V[b], L, N, cells(offsets, nrec, b, N), arc, extra, post, gamma[b])
    return SimpleNamespace(post=post, logz=logz, gamma=gamma)


def brute_force(f, s2p, P, V, L, N, cl, arc, extra=None):
    """By enumeration of every lattice path of one tiny utterance, float64, W(path) summed term by term as the header writes it:
    (through {record: log sum of exp W over the paths through it}, logz).  cl: the utterance's cells [(lo, hi)]."""
    sy = lr.system(f)
    fs = sy.S1 - 1
    w = sy.w.astype(np.float64)
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    s2p = np.asarray(s2p)
    pi = sy.pi.astype(np.float64)
    paths = []

    def walk(t, state, weight, taken):
        lo, hi = cl[t]
        for r in range(lo, hi):
            k = int(arc[r])
            if k < 0 or k >= sy.i.size or sy.phony[k] or int(sy.i[k]) != state:
                continue
            d = int(sy.j[k])
            nw = weight + w[k] + (float(extra[r]) if extra is not None else 0.0)
            if t == L - 1:
                if d == fs and nw > NINF:
                    paths.append((nw, taken + [r]))
            elif d != fs:
                nw += Vd[t + 1, s2p[d]]
                if nw > NINF:
                    walk(t + 1, d, nw, taken + [r])

    if L > 0:
        lo, hi = cl[0]
        for s in sorted({int(sy.i[int(arc[r])]) for r in range(lo, hi) if 0 <= int(arc[r]) < sy.i.size and not sy.phony[int(arc[r])]}):
            if s != fs and pi[s] + Vd[0, s2p[s]] > NINF:
                walk(0, s, pi[s] + Vd[0, s2p[s]], [])
    through = {}
    logz = NINF
    for wt, taken in paths:
        logz = np.logaddexp(logz, wt)
        for r in taken:
            through[r] = np.logaddexp(through.get(r, NINF), wt)
    return through, float(logz)


def check(got_post, got_logz, got_gamma, ref, what=""):
    """The project's parity bar against the float64 restatement: on p = exp(post) and on gamma |dp| <= 1e-4 max(p_ref, 1e-6); where
    p_ref > 1e-30, |d log p| <= 1e-4 max(1, |log p_ref|); logz to 1e-4 relative; -inf exactly where the reference has -inf; gamma
    exactly 0 where the reference's is exactly 0 (rows at or behind len, utterances without a path, pdfs no record's source has);
    nothing NaN.  Records no cell covers (NaN in the reference) are not compared.  Returns the largest errors seen."""
    got_post, got_logz = np.asarray(got_post, dtype=np.float64), np.asarray(got_logz, dtype=np.float64)
    seen = ~np.isnan(ref.post)
    gp, rp = got_post[seen], ref.post[seen]
    assert not np.isnan(gp).any() and not np.isnan(got_logz).any(), what
    assert np.array_equal(np.isneginf(gp), np.isneginf(rp)), (what, np.flatnonzero(np.isneginf(gp) != np.isneginf(rp))[:10])
    assert np.array_equal(np.isneginf(got_logz), np.isneginf(ref.logz)), (what, got_logz, ref.logz)
    assert (gp <= 0).all(), what
    fin = ~np.isneginf(rp)
    p, pr = np.exp(gp[fin]), np.exp(rp[fin])
    dp = np.abs(p - pr) / np.maximum(pr, 1e-6)
    big = pr > 1e-30
    dl = np.abs(gp[fin][big] - rp[fin][big]) / np.maximum(1.0, np.abs(rp[fin][big]))
    zf = ~np.isneginf(ref.logz)
    dz = np.abs(got_logz[zf] - ref.logz[zf]) / np.maximum(np.abs(ref.logz[zf]), 1e-30)
    worst = SimpleNamespace(p=float(dp.max()) if dp.size else 0.0, logp=float(dl.max()) if dl.size else 0.0, logz=float(dz.max()) if dz.size else 0.0, gamma=0.0)
    if got_gamma is not None:
        g = np.asarray(got_gamma, dtype=np.float64)
        assert g.shape == ref.gamma.shape and not np.isnan(g).any(), what
        assert (g[ref.gamma == 0] == 0).all(), what
        dg = np.abs(g - ref.gamma) / np.maximum(ref.gamma, 1e-6)
        worst.gamma = float(dg.max()) if dg.size else 0.0
    print(f"{what}: |dp| {worst.p:.3g}  |dlogp| {worst.logp:.3g}  |dlogz| {worst.logz:.3g}  |dgamma| {worst.gamma:.3g}  (bar 1e-4 each)")
    assert worst.p <= 1e-4 and worst.logp <= 1e-4 and worst.logz <= 1e-4 and worst.gamma <= 1e-4, (what, vars(worst))
    return worst
