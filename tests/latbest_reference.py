"""Test helper: NumPy float32 restatement of the lattice best paths (include/markovmodels_amd.h, mm_latticebest_f32) by the header's
definition, over a record list -- offsets [B * N + 1], arc [nrec], extra [nrec] or None -- and the entry lists of
lattice_reference.system.  Every value is a float32 formed by the header's adds in its grouping, the one subtraction and a maximum
in the floats' order with -0 below +0 (taken on the order-preserving integer code of the float, which is that order), so the device's
result is this one bit for bit, whatever the inputs.  What the header says of doctored input is restated too: entry indices outside
the FSM and the phony self-loop are dead records, cells are clamped into [0, nrec] and made non-decreasing, lens into [0, N].  Plus a
float64 brute force for tiny graphs: every lattice path, one record per transition, every choice among parallel entries, with the tie
rule applied to the enumerated prefixes."""
from types import SimpleNamespace

import numpy as np

import lattice_reference as lr
from latpost_reference import _live, cells

NINF = np.float32(-np.inf)
EMPTY = np.uint32(0x007FFFFF)  # the code of -inf


def enc(x):
    """float32 -> uint32 in the floats' order, -0 below +0."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec(c):
    c = np.asarray(c, dtype=np.uint32)
    return np.where(c & np.uint32(0x80000000), c & np.uint32(0x7FFFFFFF), ~c).astype(np.uint32).view(np.float32)


def _max_into(S1, idx, vals):
    """The vector [S1] of the maxima of vals by idx (-inf where none), values of -inf left out."""
    c = np.full(S1, EMPTY, dtype=np.uint32)
    on = vals > NINF
    np.maximum.at(c, idx[on], enc(vals[on]))
    return dec(c)


def utterance(sy, s2p, P, V, L, N, cl, arc, extra, score, rec, path):
    """One utterance: fills score[lo:hi] of its cells, rec [N] and path [N]; returns (best, the largest finite |forward value|)."""
    S1, f = sy.S1, sy.S1 - 1
    w = sy.w.astype(np.float32)
    lhs = lr.lhs_rows(s2p, P, V, L, N, S1, np.float32)
    for lo, hi in cl:
        score[lo:hi] = NINF
    rec[:] = -1
    path[:] = -1
    if L == 0:
        return NINF, 0.0
    recs = []
    with np.errstate(invalid="ignore"):
        a = (sy.pi.astype(np.float32) + lhs[0]).astype(np.float32)
        a = np.where(a > NINF, a, NINF)
        amax = float(np.abs(a[np.isfinite(a)]).max()) if np.isfinite(a).any() else 0.0
        for t in range(L):
            lo, hi = cl[t]
            k = arc[lo:hi].astype(np.int64)
            ok = _live(sy, k)
            r = np.arange(lo, hi)[ok]
            k = k[ok]
            i, j = sy.i[k], sy.j[k]
            ex = extra[r].astype(np.float32) if extra is not None else np.zeros(r.size, dtype=np.float32)
            wz = ((w[k] + ex).astype(np.float32) + lhs[t + 1][j]).astype(np.float32)
            fr = (a[i] + wz).astype(np.float32)
            fr = np.where(fr > NINF, fr, NINF)
            if np.isfinite(fr).any():
                amax = max(amax, float(np.abs(fr[np.isfinite(fr)]).max()))
            a = _max_into(S1, j, fr)
            recs.append((r, i, j, wz, fr))
        best = a[f]
        if not best > NINF:
            return NINF, amax
        bv = np.full(S1, NINF, dtype=np.float32)
        bv[f] = 0
        cur = f
        for t in range(L - 1, -1, -1):
            r, i, j, wz, fr = recs[t]
            y = (fr + bv[j]).astype(np.float32)
            score[r] = np.where(y > NINF, (y - best).astype(np.float32), NINF)
            z = (wz + bv[j]).astype(np.float32)
            bv = _max_into(S1, i, np.where(z > NINF, z, NINF))
            if cur >= 0:
                into = (j == cur) & (fr > NINF)
                if into.any():
                    c = enc(fr[into])
                    q = np.flatnonzero(into)[np.flatnonzero(c == c.max())[0]]  # (r ascends: the lowest of the ties)
                    rec[t], path[t], cur = r[q], i[q], int(i[q])
                else:
                    cur = -1
    return best, amax


def reference(fs, gs, V, lens, offsets, arc, extra=None, nrec=None):
    """The batch: best [B] float32, score [nrec] float32 (NaN where no cell covers a record: the entry does not write there), rec
    [B, N] int64, path [B, N] int32, amax [B].  fs / gs: the FSM and the GraphSpec-like (state2pdf, P) of every utterance."""
    V = np.asarray(V, dtype=np.float32)
    B, N, P = V.shape
    arc = np.asarray(arc)
    nrec = arc.size if nrec is None else int(nrec)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.full(B, N) if lens is None else np.asarray(lens)
    score = np.full(nrec, np.nan, dtype=np.float32)
    best = np.full(B, NINF, dtype=np.float32)
    rec = np.full((B, N), -1, dtype=np.int64)
    path = np.full((B, N), -1, dtype=np.int32)
    amax = np.zeros(B)
    sys = {}
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), N))
        sy = sys.setdefault(id(fs[b]), lr.system(fs[b]))
        best[b], amax[b] = utterance(sy, gs[b].state2pdf, gs[b].P, V[b], L, N, cells(offsets, nrec, b, N), arc, extra, score, rec[b], path[b])
    return SimpleNamespace(best=best, score=score, rec=rec, path=path, amax=amax)


def brute_force(f, s2p, P, V, L, N, cl, arc, extra=None):
    """By enumeration of every lattice path of one tiny utterance, float64, W(path) summed term by term as the header writes it:
    (through {record: the greatest W over the paths through it}, best, rec [L] -- the header's tie rule applied to the greatest
    weights of the enumerated PREFIXES that end in each record; [] without a path).  cl: the utterance's cells [(lo, hi)]."""
    sy = lr.system(f)
    fs = sy.S1 - 1
    w = sy.w.astype(np.float64)
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    s2p = np.asarray(s2p)
    pi = sy.pi.astype(np.float64)
    paths = []
    pre = {}  # record -> the greatest weight of a prefix that ends with it, the destination's emission included (f_r)

    def walk(t, state, weight, taken):
        lo, hi = cl[t]
        for r in range(lo, hi):
            k = int(arc[r])
            if k < 0 or k >= sy.i.size or sy.phony[k] or int(sy.i[k]) != state:
                continue
            d = int(sy.j[k])
            nw = weight + w[k] + (float(extra[r]) if extra is not None else 0.0)
            if t == L - 1:
                if d == fs and nw > -np.inf:
                    pre[r] = max(pre.get(r, -np.inf), nw)
                    paths.append((nw, taken + [r]))
            elif d != fs:
                nw += Vd[t + 1, s2p[d]]
                if nw > -np.inf:
                    pre[r] = max(pre.get(r, -np.inf), nw)
                    walk(t + 1, d, nw, taken + [r])

    if L > 0:
        lo, hi = cl[0]
        for s in sorted({int(sy.i[int(arc[r])]) for r in range(lo, hi) if 0 <= int(arc[r]) < sy.i.size and not sy.phony[int(arc[r])]}):
            if s != fs and pi[s] + Vd[0, s2p[s]] > -np.inf:
                walk(0, s, pi[s] + Vd[0, s2p[s]], [])
    through = {}
    best = -np.inf
    for wt, taken in paths:
        best = max(best, wt)
        for r in taken:
            through[r] = max(through.get(r, -np.inf), wt)
    rec = []
    if best > -np.inf:
        cur = fs
        for t in range(L - 1, -1, -1):
            lo, hi = cl[t]
            into = [r for r in range(lo, hi) if r in pre and int(sy.j[int(arc[r])]) == cur]
            top = max(pre[r] for r in into)
            r = min(r for r in into if pre[r] == top)
            rec.append(r)
            cur = int(sy.i[int(arc[r])])
        rec.reverse()
    return through, float(best), rec
