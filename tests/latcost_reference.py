"""Test helper: NumPy restatement of the lattice expected cost (include/markovmodels_amd.h, mm_latticecost_f32) by the header's
definition, on top of tests/latpost_reference.py: the same `system`, `cells` and `_live`, the same doctored-input rules, post / logz /
gamma taken from latpost_reference itself.  The cost recursions ca / cb are carried centred -- relative to the largest value of the
step, the offsets accumulated in float64 -- with the conditional probabilities exp(x_r - a_{t+1}(j)) / exp(z_r - b_t(i)) from the
float64 log recursions.  dtype = float64: the reference; diff is then E[A | through r] - risk written out with the offsets, the
posterior normalised by logz itself (that a cell's diff sums to 0 is a property to check, not one built in).  dtype = float32 rounds
the probabilities, the centred values and every sum over them to float32 and forms diff the way a float32 implementation has to,
against the cell's own posterior mean: what float32 arithmetic alone costs, the source of the absolute part of the gradient's bar.
Plus a brute force for tiny graphs: every lattice path."""
from types import SimpleNamespace

import numpy as np

import latpost_reference as lp
import lattice_reference as lr

NINF = -np.inf

# The absolute part `a` of the bars |diff - diff_ref| <= 1e-4 |diff_ref| + a * G_b and the same for grad, G_b = the utterance's largest
# |ref| of that output.  Measured on the CPU, before any kernel output was judged: reference(..., dtype=np.float32) against
# reference(...) in float64 on the inputs of tests/test_gpu_latticecost.py as tests/test_latticecost.py builds them
# (tools/measure_latticecost_floor.py prints the table; profiles/latticecost_floor.json keeps it).  Worst |x_f32 - x_f64| / G_b over
# diff and grad:
#   both small graphs, B = 3, N = 6, beams 0 / 2 / inf            <= 5.5e-6 (0 at beam 0 on the grid)
#   1 .. 2049 parallel self-loops; 257 / 1025 entries             <= 1.0e-6
#   four distinct graphs, beam 2 / inf; a chain of 3000 states    <= 3.0e-6
#   the 40-state graph, N = 200, beam 3; the same, costs + 64     1.5e-6; 9.1e-6 (float32 against the UNSHIFTED float64 reference)
# (utterances whose grad is a structural 0 -- `scales` below -- have no G_b of grad and count with their diff only.)  a = 10 x the worst (the factor is for what the NumPy run
# does not have: the hardware's exp / log and the 2^-40 fixed point of the sums), capped at the project's own 1e-4.
F32_FLOOR = 9.097e-06
DIFF_ABS_A = min(10 * F32_FLOOR, 1e-4)


def _wsum(n, idx, wts, val, dt):
    """out[s] = sum_{r: idx_r = s} wts_r val_r, in dt."""
    out = np.zeros(n, dtype=dt)
    np.add.at(out, idx, (wts.astype(dt) * val.astype(dt)).astype(dt))
    return out


def utterance(sy, s2p, P, V, L, N, cl, arc, extra, cost, post, diff, grad, touched, dtype):
    """One utterance, post [nrec] and logz given (latpost_reference's): fills diff[lo:hi] of its cells, grad [N, P] and touched
    [N, P] (which elements of grad a record with a path through it adds to); returns risk."""
    dt = np.dtype(dtype).type
    exact = dt is np.float64
    S1, f = sy.S1, sy.S1 - 1
    w = sy.w.astype(np.float64)
    lhs = lr.lhs_rows(s2p, P, V, L, N, S1, np.float64)
    s2p = np.asarray(s2p)
    for lo, hi in cl:
        diff[lo:hi] = 0.0
    if L == 0:
        return 0.0
    recs = []
    with np.errstate(invalid="ignore", over="ignore"):
        a = sy.pi.astype(np.float64) + lhs[0]
        C = np.zeros(S1, dtype=dt)  # ca_t - coff, centred: C - Cm is what a step reads
        Cm, coff = dt(0), 0.0
        for t in range(L):
            lo, hi = cl[t]
            k = arc[lo:hi].astype(np.int64)
            ok = lp._live(sy, k)
            r = np.arange(lo, hi)[ok]
            k = k[ok]
            i, j = sy.i[k], sy.j[k]
            ex = extra[r].astype(np.float64) if extra is not None else np.zeros(r.size)
            wz = w[k] + ex + lhs[t + 1][j]
            x = a[i] + wz
            live = x > NINF
            r, i, j, wz, x = r[live], i[live], j[live], wz[live], x[live]
            a = np.full(S1, NINF)
            np.logaddexp.at(a, j, x)
            v = ((C[i] - Cm).astype(dt) + cost[r].astype(dt)).astype(dt)
            recs.append((r, i, j, wz, v, coff))
            C = _wsum(S1, j, np.exp(x - a[j]), v, dt)
            if r.size:
                Cm = dt(C[np.unique(j)].max())
                coff += float(Cm)
        if not a[f] > NINF:  # (reference() does not come here: it reads logz first)
            return 0.0
        risk = coff + float(C[f] - Cm)
        bv = np.full(S1, NINF)
        bv[f] = 0.0
        C = np.zeros(S1, dtype=dt)
        Cm, boff = dt(0), 0.0
        for t in range(L - 1, -1, -1):
            r, i, j, wz, v, foff = recs[t]
            z = wz + bv[j]
            live = (z > NINF) & (post[r] > NINF)
            r, i, j, z, v = r[live], i[live], j[live], z[live], v[live]
            cbj = (C[j] - Cm).astype(dt)
            p = np.exp(post[r])
            if exact:
                d = p * ((foff + v) + (boff + cbj) - risk)
            else:
                u = (v + cbj).astype(dt)
                pd = p.astype(dt)
                ubar = dt((pd * u).astype(dt).sum(dtype=dt) / max(pd.sum(dtype=dt), dt(1e-30)))
                d = (pd * (u - ubar).astype(dt)).astype(dt)
            diff[r] = d
            real = i < S1 - 1
            np.add.at(grad[t], s2p[i[real]], np.asarray(d, dtype=np.float64)[real])
            touched[t, s2p[i[real]]] = True
            bv = np.full(S1, NINF)
            np.logaddexp.at(bv, i, z)
            wv = (cost[r].astype(dt) + cbj).astype(dt)
            C = _wsum(S1, i, np.exp(z - bv[i]), wv, dt)
            if r.size:
                Cm = dt(C[np.unique(i)].max())
                boff += float(Cm)
    return risk


def reference(fs, gs, V, lens, offsets, arc, cost, extra=None, nrec=None, dtype=np.float64):
    """The batch: risk [B], diff [nrec] (NaN where no cell covers a record), post, logz, grad [B, N, P], gamma, all float64 arrays,
    and touched [B, N, P]: False where grad is 0 by structure (rows at or behind len, utterances without a path, pdfs that no
    record with a path through it has at its source).
    fs / gs: the FSM and the GraphSpec-like (state2pdf, P) of every utterance."""
    V = np.asarray(V, dtype=np.float32)
    B, N, P = V.shape
    arc = np.asarray(arc)
    cost = np.asarray(cost, dtype=np.float32)
    nrec = arc.size if nrec is None else int(nrec)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.full(B, N) if lens is None else np.asarray(lens)
    base = lp.reference(fs, gs, V, lens, offsets, arc, extra, nrec=nrec)
    diff = np.full(nrec, np.nan)
    risk = np.zeros(B)
    grad = np.zeros((B, N, P))
    touched = np.zeros((B, N, P), dtype=bool)
    sys = {}
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), N))
        sy = sys.setdefault(id(fs[b]), lr.system(fs[b]))
        cl = lp.cells(offsets, nrec, b, N)
        if not base.logz[b] > NINF:
            for lo, hi in cl:
                diff[lo:hi] = 0.0
            continue
        risk[b] = utterance(sy, gs[b].state2pdf, gs[b].P, V[b], L, N, cl, arc, extra, cost, base.post, diff, grad[b], touched[b], dtype)
    return SimpleNamespace(risk=risk, diff=diff, post=base.post, logz=base.logz, grad=grad, gamma=base.gamma, touched=touched)


def brute_force(f, s2p, P, V, L, N, cl, arc, cost, extra=None):
    """By enumeration of every lattice path of one tiny utterance, float64: (risk, logz, mass {record: sum of exp W over the paths
    through it}, massA {record: sum of exp W * A(path) over them}); weights relative to the best path's.  No path: (0, -inf, {}, {})."""
    sy = lr.system(f)
    fs = sy.S1 - 1
    w = sy.w.astype(np.float64)
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    s2p = np.asarray(s2p)
    pi = sy.pi.astype(np.float64)
    cost = np.asarray(cost, dtype=np.float32).astype(np.float64)
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
    if not paths:
        return 0.0, NINF, {}, {}
    top = max(wt for wt, _ in paths)
    Z = sum(np.exp(wt - top) for wt, _ in paths)
    mass, massA = {}, {}
    risk = 0.0
    for wt, taken in paths:
        q = np.exp(wt - top) / Z
        A = float(sum(cost[r] for r in taken))
        risk += q * A
        for r in taken:
            mass[r] = mass.get(r, 0.0) + q
            massA[r] = massA.get(r, 0.0) + q * A
    return risk, float(top + np.log(Z)), mass, massA


def owners(offsets, nrec, B, N):
    """The utterance of every record a cell covers (-1: none), by the clamped cells."""
    own = np.full(nrec, -1, dtype=np.int64)
    for b in range(B):
        for lo, hi in lp.cells(offsets, nrec, b, N):
            own[lo:hi] = b
    return own


def scales(ref, offsets):
    """Per utterance (G of diff, G of grad, whether grad is degenerate): G the largest |ref| of the output.  Degenerate: the
    reference's grad is its own rounding noise, G_grad < 1e-9 G_diff -- every cell's records share their source's pdf (one real
    state, a chain), so a row is the cell's sum of diff, 0 in exact arithmetic and about 1e-16 G_diff in float64."""
    B, N = ref.grad.shape[:2]
    own = owners(offsets, ref.diff.size, B, N)
    out = []
    for b in range(B):
        m = own == b
        Gd = float(np.abs(ref.diff[m]).max()) if m.any() else 0.0
        Gg = float(np.abs(ref.grad[b]).max())
        out.append((Gd, Gg, Gg < 1e-9 * Gd))
    return out


def check(got, ref, cost, lens, offsets, what="", a=DIFF_ABS_A):
    """The bars against the float64 restatement.  risk: 1e-4 sum_r exp(post_ref) |cost| + 1e-6 L max |cost| (over the utterance's
    records in cells t < len).  diff and grad: 1e-4 |ref| + a G_b, G_b the utterance's largest |ref| of that output.  post, logz
    and gamma: latpost_reference.check.  Exact zeros where the reference has them by structure -- diff of records without a path
    through them, grad where `touched` is False (a sum of diff that merely cancels in float64 is not held to an exact 0) -- and
    nothing NaN.  Where an utterance's grad
    is degenerate (`scales`: the reference's values are float64 rounding noise around a sum that is 0 by structure, so their
    largest is no scale of anything) its rows are held to the bar of the header's identity instead -- a row of grad is a sum of
    the cell's diff, within the summed bars of its terms: |grad[b, n, p]| <= (records of the cell) * a * G_b(diff).  `got`:
    anything with the members of LatticeCost (grad / gamma may be None).  Returns the worst ratios (risk error / bar, diff and
    grad error / G_b)."""
    B, N = ref.grad.shape[0], ref.grad.shape[1]
    nrec = ref.diff.size
    lp.check(np.asarray(got.post)[:nrec], got.logz, got.gamma, ref, what)
    risk, diff = np.asarray(got.risk, dtype=np.float64), np.asarray(got.diff, dtype=np.float64)[:nrec]
    cost = np.abs(np.asarray(cost, dtype=np.float64))[:nrec]
    lens = np.full(B, N) if lens is None else np.clip(np.asarray(lens), 0, N)
    own = owners(offsets, nrec, B, N)
    seen = own >= 0
    assert not np.isnan(risk).any() and not np.isnan(diff[seen]).any(), what
    assert (diff[seen][np.isneginf(ref.post[seen])] == 0).all(), what
    worst = SimpleNamespace(risk=0.0, diff=0.0, grad=0.0)
    p = np.where(np.isneginf(ref.post) | np.isnan(ref.post), 0.0, np.exp(np.nan_to_num(ref.post, nan=NINF)))
    for b in range(B):
        m = own == b
        if not ref.logz[b] > NINF:
            assert risk[b] == 0 and (diff[m] == 0).all(), (what, b)
            continue
        live = m & (p > 0)
        bar = 1e-4 * float((p[live] * cost[live]).sum()) + 1e-6 * int(lens[b]) * (float(cost[live].max()) if live.any() else 0.0)
        err = abs(risk[b] - ref.risk[b])
        assert err <= bar, (what, b, risk[b], ref.risk[b], bar)
        worst.risk = max(worst.risk, err / max(bar, 1e-300))
        G = float(np.abs(ref.diff[m]).max()) if m.any() else 0.0
        e = np.abs(diff[m] - ref.diff[m])
        assert (e <= 1e-4 * np.abs(ref.diff[m]) + a * G).all(), (what, b, "diff", float(e.max()), G)
        worst.diff = max(worst.diff, float(e.max()) / G if G > 0 else 0.0)
    if got.grad is not None:
        g = np.asarray(got.grad, dtype=np.float64)
        assert g.shape == ref.grad.shape and not np.isnan(g).any(), what
        assert (g[~ref.touched] == 0).all(), what
        sc = scales(ref, offsets)
        for b in range(B):
            Gd, G, degenerate = sc[b]
            e = np.abs(g[b] - ref.grad[b])
            if degenerate:
                nc = np.array([hi - lo for lo, hi in lp.cells(offsets, nrec, b, N)], dtype=np.float64)
                assert (e <= 1e-4 * np.abs(ref.grad[b]) + (nc * a * Gd)[:, None]).all(), (what, b, "grad of one pdf per cell", float(e.max()), Gd)
                continue
            assert (e <= 1e-4 * np.abs(ref.grad[b]) + a * G).all(), (what, b, "grad", float(e.max()), G)
            worst.grad = max(worst.grad, float(e.max()) / G if G > 0 else 0.0)
    print(f"{what}: risk err / bar {worst.risk:.3g}  |ddiff| / G {worst.diff:.3g}  |dgrad| / G {worst.grad:.3g}  (a = {a:.3g})")
    return worst
