"""Test helper: NumPy float64 restatement of the lattice path sampling (include/markovmodels_amd.h, mm_latticesample_f32) by the
header's definition -- Philox-4x32-10 and unit_open restated (the integer part is exact, so the uniforms are the device's bit for
bit), the float64 forward over the records of a lattice, the backward Gumbel-max draw with the header's tie rule -- plus the
enumeration of every lattice path of a tiny utterance WITH its posterior, and the acceptance rules of the tests.

Device and restatement differ only by float32 rounding: of the forward values x_r and of the Gumbel variates g_r.  A key's error
budget is 1e-4 max(1, |c_r|) + 2e-5, c_r the log of the record's probability given its destination: the first term is the project's
parity bar on a log probability, the second 16 float32 ulps of |g| <= 16.7.  A decision is OPEN when another candidate's float64 key
lies within the sum of the two budgets of the winner's; a chain is open when any of its decisions is.  A chain that is not open
must be the restatement's, record for record; an open chain must still take, at every step and from its OWN current state, a
candidate within the budgets of that step's maximum."""
from types import SimpleNamespace

import numpy as np

import latpost_reference as lp
import lattice_reference as lr

NINF = -np.inf
M32 = np.uint64(0xFFFFFFFF)


def philox_4x32_10(k0, k1, c0, c1, c2, c3):
    """The first word of Philox-4x32-10 under the key (k0, k1) at the counter (c0, c1, c2, c3): uint64 arrays that hold 32-bit
    values, broadcast against each other."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def unit_open(w):
    """23 random bits -> a uniform strictly inside (0, 1): exact in float32, hence in float64."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(u):
    return -np.log(-np.log(u))


def seed_key(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def budget(c):
    """The error budget of a key whose record has the log conditional probability c."""
    c = np.where(np.isfinite(c), c, 0.0)  # (a record that is no candidate has no key)
    return 1e-4 * np.maximum(1.0, np.abs(c)) + 2e-5


def forward(sy, s2p, P, V, L, N, cl, arc, extra):
    """The float64 forward over the records of one utterance: a SimpleNamespace of logz, a0 [S1] = alpha_hat + the first frame's
    emissions, and per transition t < L the live records of the cell -- r, place (r - lo), i, j, wz, x = a_t(i) + wz and
    c = x - a_{t+1}(j), the log of the record's probability given its destination."""
    S1, f = sy.S1, sy.S1 - 1
    w = sy.w.astype(np.float64)
    lhs = lr.lhs_rows(s2p, P, V, L, N, S1, np.float64)
    steps = []
    if L == 0:
        return SimpleNamespace(logz=NINF, a0=None, steps=steps, L=L, f=f)
    with np.errstate(invalid="ignore"):
        a0 = sy.pi.astype(np.float64) + lhs[0]
        a = a0
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
            x = np.where(np.isnan(x), NINF, x)
            a = np.full(S1, NINF)
            np.logaddexp.at(a, j, x)
            c = np.where(x > NINF, x - a[j], NINF)
            steps.append(SimpleNamespace(r=r, place=r - lo, i=i, j=j, wz=wz, x=x, c=c))
    return SimpleNamespace(logz=float(a[f]), a0=a0, steps=steps, L=L, f=f)


def _keys(st, cur, b, ks, t, key):
    """[len(ks), records] the float64 keys of step st for chains ks that sit in the states cur: -inf for a record that is no
    candidate."""
    cand = (st.j[None, :] == cur[:, None]) & (st.x > NINF)[None, :]
    u = unit_open(philox_4x32_10(key[0], key[1], b, ks[:, None], t, st.place[None, :].astype(np.uint64)))
    return np.where(cand, st.x[None, :] + gumbel(u), NINF)


def draw(ut, b, N, ks, seed):
    """The samples ks (indices k) of utterance b: rec [K, N], path [K, N], logprob [K], open [K]."""
    ks = np.asarray(ks, dtype=np.uint64)
    K = ks.size
    rec = np.full((K, N), -1, dtype=np.int64)
    path = np.full((K, N), -1, dtype=np.int32)
    logprob = np.full(K, NINF)
    opened = np.zeros(K, dtype=bool)
    if not ut.logz > NINF:
        return rec, path, logprob, opened
    key = seed_key(seed)
    cur = np.full(K, ut.f, dtype=np.int64)
    W = np.zeros(K)
    rows = np.arange(K)
    for t in range(ut.L - 1, -1, -1):
        st = ut.steps[t]
        kv = _keys(st, cur, b, ks, t, key)
        win = np.argmax(kv, axis=1)  # (the first of equal keys: the lowest place)
        kw = kv[rows, win]
        assert (kw > NINF).all()  # (a chain of an utterance with a path never dies)
        bud = budget(st.c)
        near = kv + bud[None, :] + bud[win][:, None]
        near[rows, win] = NINF
        opened |= (near >= kw[:, None]).any(axis=1)
        rec[:, t] = st.r[win]
        path[:, t] = st.i[win]
        W += st.wz[win]
        cur = st.i[win]
    logprob = W + ut.a0[cur] - ut.logz
    return rec, path, logprob, opened


def reference(fs, gs, V, lens, offsets, arc, extra, K, seed, nrec=None, ks=None):
    """The batch: rec [B, K, N] int64, path [B, K, N] int32, logprob [B, K] and logz [B] float64, open [B, K] (which chains hold an
    open decision), and what check() needs.  fs / gs: the FSM and the GraphSpec-like (state2pdf, P) of every utterance; ks: the
    sample indices (default 0 .. K - 1)."""
    V = np.asarray(V, dtype=np.float32)
    B, N, P = V.shape
    arc = np.asarray(arc)
    nrec = arc.size if nrec is None else int(nrec)
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.full(B, N) if lens is None else np.asarray(lens)
    ks = np.arange(K) if ks is None else np.asarray(ks)
    out = SimpleNamespace(rec=np.empty((B, ks.size, N), dtype=np.int64), path=np.empty((B, ks.size, N), dtype=np.int32), logprob=np.empty((B, ks.size)),
                          logz=np.empty(B), open=np.empty((B, ks.size), dtype=bool), uts=[], seed=seed, ks=ks, N=N)
    sys = {}
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), N))
        sy = sys.setdefault(id(fs[b]), lr.system(fs[b]))
        ut = forward(sy, gs[b].state2pdf, gs[b].P, V[b], L, N, lp.cells(offsets, nrec, b, N), arc, extra)
        out.uts.append(ut)
        out.logz[b] = ut.logz
        out.rec[b], out.path[b], out.logprob[b], out.open[b] = draw(ut, b, N, ks, seed)
    return out


def follows(ut, b, k, seed, rec):
    """Whether the chain rec [N] of sample k of utterance b takes, at every step and from its own current state, a candidate whose
    float64 key lies within the two budgets of that step's maximum (and is -1 behind the length)."""
    key = seed_key(seed)
    cur = ut.f
    if (rec[ut.L :] != -1).any():
        return False
    for t in range(ut.L - 1, -1, -1):
        st = ut.steps[t]
        kv = _keys(st, np.array([cur]), b, np.array([k], dtype=np.uint64), t, key)[0]
        at = np.flatnonzero(st.r == rec[t])
        if at.size != 1 or not kv[at[0]] > NINF:
            return False
        bud = budget(st.c)
        top = int(np.argmax(kv))
        if kv[at[0]] + bud[at[0]] + bud[top] < kv[top]:
            return False
        cur = int(st.i[at[0]])
    return True


def check(got_rec, ref, what=""):
    """The decision rule on the device's rec [B, K, N] against reference(): every chain that is not open equals the restatement's;
    every open chain follows(); at most 5 % of the case's chains are open (a CONDITION on the case, asserted from the restatement
    alone).  Returns the number of open chains."""
    got_rec = np.asarray(got_rec)
    assert got_rec.shape == ref.rec.shape and got_rec.dtype == np.int64, (what, got_rec.shape, ref.rec.shape)
    assert ref.open.mean() <= 0.05, (what, "open chains", int(ref.open.sum()), ref.open.size)
    closed = ~ref.open
    bad = np.argwhere(closed & (got_rec != ref.rec).any(axis=2))
    assert bad.size == 0, (what, bad[:5], [(got_rec[b, k], ref.rec[b, k]) for b, k in bad[:2]])
    for b, q in np.argwhere(ref.open):
        assert follows(ref.uts[b], b, int(ref.ks[q]), ref.seed, got_rec[b, q]), (what, "open chain", b, q, got_rec[b, q], ref.rec[b, q])
    return int(ref.open.sum())


def enumerate_paths(f, s2p, P, V, L, N, cl, arc, extra=None):
    """Every lattice path of one tiny utterance -- one record per transition, every choice among parallel entries -- with its
    posterior, float64, W(path) summed term by term as the header writes it: (paths [M, L] int64 of records, log p [M], logz)."""
    sy = lr.system(f)
    fs = sy.S1 - 1
    w = sy.w.astype(np.float64)
    Vd = np.asarray(V, dtype=np.float32).astype(np.float64)
    s2p = np.asarray(s2p)
    pi = sy.pi.astype(np.float64)
    found = []

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
                    found.append((nw, taken + [r]))
            elif d != fs:
                nw += Vd[t + 1, s2p[d]]
                if nw > NINF:
                    walk(t + 1, d, nw, taken + [r])

    if L > 0:
        for s in range(fs):
            if pi[s] + Vd[0, s2p[s]] > NINF:
                walk(0, s, pi[s] + Vd[0, s2p[s]], [])
    if not found:
        return np.zeros((0, L), dtype=np.int64), np.zeros(0), NINF
    wt = np.array([x[0] for x in found])
    logz = float(np.logaddexp.reduce(wt))
    return np.array([x[1] for x in found], dtype=np.int64), wt - logz, logz


def path_frequencies(paths, samples):
    """The frequency of every enumerated record sequence among samples [K, L], and how many samples are none of them."""
    index = {tuple(p): q for q, p in enumerate(paths.tolist())}
    uniq, cnt = np.unique(np.asarray(samples), axis=0, return_counts=True)
    freq = np.zeros(len(index))
    outside = 0
    for row, c in zip(uniq.tolist(), cnt.tolist()):
        q = index.get(tuple(row))
        if q is None:
            outside += c
        else:
            freq[q] = c
    return freq / float(np.asarray(samples).shape[0]), outside
