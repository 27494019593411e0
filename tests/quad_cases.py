"""Fixtures of the quad-kernel tests (tests/test_quad_inputs.py without a GPU, tests/test_gpu_quad_instances.py on one): graphs and
inputs that reach every instance of mm_fbq_kernel<KQ,RPT,PASS> (csrc/mm_kernel_quad.hip, instances in csrc/mm_quad_tu.hip) and the
data-dependent branches inside it -- quads streamed on virtual lanes at both sides of the register window, rows of every number
of extra lane ends (row_short: 0, 1, 2; row_long: 3 and more) in both passes, rows beyond the RPT register-carried ones, the three
bodies of the exact fallback on rows of 1, 4, 5, 8 and 9 arcs, pdf counts on both sides of every 64-lane pass, every wave count
with a branch of its own, and the short lengths.  NumPy only; `wl` is the package's workloads module.

What a case reaches is stated HERE from the graphs' degrees, KQ and the wave count alone (quads per direction, NW and RPT as the
engine and the launcher derive them, the forward and the backward numbering, the kind of every row, the rows on virtual lanes) --
not read back from kernels().  tests/test_quad_inputs.py checks these statements against the host packer where it exposes them, and
from the float64 oracle that the rows, pdfs and frames a case is there for carry posterior mass."""
import dataclasses

import numpy as np

import stream_cases as sc
from stream_cases import _memo, emissions
from wave_cases import _chain, reference  # noqa: F401  (reference: the float64 oracle of a batch, memoised)

KQ16 = (1, 2, 3, 5, 6, 7, 9, 10, 11, 13)      # up to 16 waves
KQ8 = (15, 17, 19, 21, 23, 25, 27, 29)        # up to 8 waves
KQ_ALL = KQ16 + KQ8
OFF_TABLE_KQ = (4, 8, 12, 14, 16, 28)         # in 1 .. 29 and without an instance
FORCE_QUAD = {"MM_DEBUG": "1", "MM_KERNEL": "quad"}
UNDERFLOW_NATS = 90 * np.log(2.0)             # MM_Q_THR = 2^-90: a linear sum below it takes the exact fallback (62.4 nats)


def quad_env(kq=None, nwaves=None, no_xcsr=False):
    env = dict(FORCE_QUAD)
    if kq is not None:
        env["MM_KQ"] = str(kq)
    if nwaves is not None:
        env["MM_NWAVES"] = str(nwaves)
    if no_xcsr:
        env["MM_NO_XCSR"] = "1"
    return env


# ---- the geometry, from degrees, KQ and the wave count
MM_QS_PAD, MM_ROW_LONG = 2, 1    # the two zero slots ahead of the quad sums; the mark of a row with more than two lane ends
def row_lengths(g):
    """(forward rows, backward rows) [S + 1]: the arcs into / out of every state of the extended FSM, the phony final state last."""
    return sc.degrees(g)


def row_quads(deg):
    return (np.asarray(deg) + 3) // 4


def quads(g):
    """Quads per direction."""
    return tuple(int(row_quads(d).sum()) for d in row_lengths(g))


def wave_cap(kq):
    return 8 if kq > 13 else 16


def default_kq(nq):
    """pick_quad_geometry: the first KQ whose register window (16 waves up to 13, then 8 waves) holds the quads, else 29."""
    for k in KQ16:
        if 64 * 16 * k >= nq:
            return k
    for k in KQ8:
        if 64 * 8 * k >= nq:
            return k
    return 29


def geometry(gs, d, kq=None, nwaves=None):
    """(KQ, NW, RPT) of direction d for a batch of the graphs gs under MM_KQ = kq and MM_NWAVES = nwaves: the engine takes the largest
    quad count and state count of the batch, enough waves for the quads and for two rows per thread (up to the cap of KQ), and the
    launcher RPT = 2 where ceil(S1p / threads) <= 2, else 3."""
    gs = gs if isinstance(gs, (list, tuple)) else [gs]
    nq = max(quads(g)[d] for g in gs)
    S1 = max(g.S + 1 for g in gs)
    KQ = kq if kq in KQ_ALL else default_kq(nq)
    NW = min(wave_cap(KQ), max(1, -(-nq // (64 * KQ)), (S1 + 127) // 128))
    if nwaves is not None and 1 <= nwaves <= wave_cap(KQ):
        NW = nwaves
    S1p = (S1 + 4) // 4 * 4   # (a state vector's padded length: at least one slot beyond the last state, a multiple of 4)
    return KQ, NW, 2 if -(-S1p // (64 * NW)) <= 2 else 3


def instance(gs, d, kq=None, nwaves=None):
    """What kernels() prints for direction d."""
    KQ, NW, RPT = geometry(gs, d, kq, nwaves)
    return f"mm_fbq_kernel<{KQ},{RPT},{d}> x {NW} waves"


def instances(gs, kq=None, nwaves=None):
    return [instance(gs, d, kq, nwaves) for d in (0, 1)]


def hat_pdf(g):
    return np.append(np.asarray(g.state2pdf), g.P).astype(np.int64)


def numbering(g, d):
    """order [S + 1]: internal position -> state, of direction d.  Forward: rows by decreasing quad count, stable.  Backward: the pdfs
    by decreasing mean quad count of their rows (stable), inside a pdf the rows by decreasing quad count (stable)."""
    nq = row_quads(row_lengths(g)[d])
    if d == 0:
        return np.argsort(-nq, kind="stable")
    pdf = hat_pdf(g)
    tot = np.bincount(pdf, weights=nq.astype(np.float64), minlength=g.P + 1)
    cnt = np.bincount(pdf, minlength=g.P + 1).astype(np.float64)
    pdf_order = np.argsort(-(tot / np.maximum(cnt, 1.0)), kind="stable")
    rank = np.empty(g.P + 1, dtype=np.int64)
    rank[pdf_order] = np.arange(g.P + 1)
    return np.lexsort((np.arange(g.S + 1), -nq, rank[pdf]))


@dataclasses.dataclass
class Layout:
    order: np.ndarray    # position -> state
    nq: np.ndarray       # [position] quads of the row
    q0: np.ndarray       # [position] its first quad
    extra: np.ndarray    # [position] lane ends (q % KQ == KQ - 1) inside the row before its last quad
    total: int           # quads of the direction

    def kind(self, i):
        return "empty" if self.nq[i] == 0 else "long" if self.extra[i] >= 3 else "short"

    def position_of(self, state):
        return int(np.flatnonzero(self.order == state)[0])


def layout(g, d, KQ):
    """Where every row's quads lie: rows in the direction's numbering, their quads one after the other; quad q belongs to lane q // KQ.
    A row's sum is the running sum at its last quad plus the running sums at the lane ends before it."""
    order = numbering(g, d)
    nq = row_quads(row_lengths(g)[d])[order]
    q0 = np.concatenate([[0], np.cumsum(nq)[:-1]])
    qe = q0 + nq - 1
    first = q0 + (KQ - 1 - q0 % KQ)
    extra = np.where((nq > 0) & (first < qe), -(-(qe - first) // KQ), 0)
    return Layout(order, nq, q0, extra, int(nq.sum()))


def row_records(g, d, KQ):
    """[S + 1, 4] what the kernel's row records must hold, by position: 2 + the last quad (0: no arcs), 2 + the first lane end before
    it (0: none), the pdf, and 2 + the second lane end (0: none; MM_ROW_LONG: three or more)."""
    lay = layout(g, d, KQ)
    first = lay.q0 + (KQ - 1 - lay.q0 % KQ)
    qe = np.where(lay.nq > 0, lay.q0 + lay.nq - 1 + MM_QS_PAD, 0)
    i1 = np.where(lay.extra >= 1, first + MM_QS_PAD, 0)
    i2 = np.where(lay.extra >= 3, MM_ROW_LONG, np.where(lay.extra == 2, first + KQ + MM_QS_PAD, 0))
    return np.stack([qe, i1, hat_pdf(g)[lay.order], i2], axis=1)


def virtual_positions(lay, KQ, NT):
    """Positions of the rows with a quad beyond the register window of NT lanes x KQ quads (streamed from L2 by quad_phase)."""
    return np.flatnonzero((lay.nq > 0) & (lay.q0 + lay.nq - 1 >= NT * KQ))


def generic_positions(lay, RPT, NT):
    """Positions of the rows beyond the RPT register-carried ones of each thread: the generic loop."""
    return np.arange(RPT * NT, lay.order.size)


# ---- graphs
def trimmed(g):
    """g without the states that are not on any path from an initial to a final state (the kernel forms drop them: the rows of the
    forms are then the degrees of the graph); weights unchanged."""
    S = g.S
    A = np.zeros((S, S), dtype=bool)
    A[g.src, g.dst] = True
    def closure(seed, M):
        seen = seed.copy()
        front = seed.copy()
        while front.any():
            front = (M[front].any(axis=0)) & ~seen
            seen |= front
        return seen
    ini = np.zeros(S, dtype=bool)
    ini[g.init_idx[np.isfinite(g.init_w)]] = True
    fin = np.zeros(S, dtype=bool)
    fin[g.final_idx[np.isfinite(g.final_w)]] = True
    keep = closure(ini, A) & closure(fin, A.T)
    if keep.all():
        return g
    new = np.cumsum(keep) - 1
    ka, ki, kf = keep[g.src] & keep[g.dst], keep[g.init_idx], keep[g.final_idx]
    return dataclasses.replace(g, name=g.name + "_trim", S=int(keep.sum()), init_idx=new[g.init_idx[ki]], init_w=g.init_w[ki],
                               src=new[g.src[ka]], dst=new[g.dst[ka]], w=g.w[ka], final_idx=new[g.final_idx[kf]], final_w=g.final_w[kf],
                               state2pdf=np.asarray(g.state2pdf)[keep].astype(np.int32))


def is_trim(g):
    return trimmed(g) is g


def mixed300(wl):
    """About 300 states with rows of 1 .. 40 and more arcs in both directions: the LF-MMI denominator generator, trimmed.  1400 quads
    per direction: at one wave every KQ up to 21 leaves quads of rows of several quads on virtual lanes."""
    return _memo("q_mixed300", lambda: trimmed(wl.lfmmi_denominator(300, 40, seed=5)))


def mixed300_case(wl):
    g = mixed300(wl)
    return g, emissions(3, 12, g.P, 7100), np.asarray((12, 7, 2), dtype=np.int32)  # (the shortest path has two frames)


def chain_graph(wl, S1, P=24, every=8):
    """A left-to-right chain (wave_cases._chain: self loop, next, the one after; every 8th state initial, the one before it final) of
    S1 - 1 states with exactly S1 quads in EACH direction.  Backward every row has 1 .. 4 arcs: one quad each.  Forward the phony
    final state's row holds n quads (its final arcs and the self loop), so n - 1 of the initial states lose every arc into them --
    rows without a quad; all other rows have one."""
    def make():
        g = _chain(wl, f"qchain{S1}", S1 - 1, np.arange(S1 - 1) % P, P, every=every)
        n = -(-(g.final_idx.size + 1) // 4)
        orphans = np.arange(every, g.S, every)[: n - 1]
        assert orphans.size == n - 1 and np.isin(orphans, g.init_idx).all()
        keep = ~np.isin(g.dst, orphans)
        return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], w=g.w[keep])
    return _memo(("q_chain", S1, P, every), make)


# the quad counts around the register window of one wave: NT * KQ - 1, NT * KQ, NT * KQ + 1, and (KQ = 3) two of the three quads of
# the first virtual lane; KQ = 2 at 129 and KQ = 3 at 193 leave it partly filled as well
VIRTUAL_CASES = [(1, 63), (1, 64), (1, 65), (1, 70), (2, 127), (2, 128), (2, 129), (2, 131), (3, 191), (3, 192), (3, 193), (3, 194), (3, 200)]


def virtual_case(wl, nq):
    g = chain_graph(wl, nq)
    return g, emissions(3, 12, g.P, 7200 + nq), np.asarray((12, 5, 7), dtype=np.int32)  # (the shortest path has 5 frames)


def dense400(wl):
    """400 states of mean degree 90: some 9000 quads per direction, rows of about 23 quads -- beyond the 7680 quads of the register window
    of 8 waves x 15 quads."""
    return _memo("q_dense400", lambda: trimmed(wl.random_fsm(400, 20, 90.0, seed=15, n_init=8)))


def dense400_case(wl):
    g = dense400(wl)
    return g, emissions(2, 8, g.P, 7300), np.asarray((8, 3), dtype=np.int32)


# ---- rows of every kind
HUB_EXTRAS = (0, 1, 2, 3, 4, 5, 8, 9)
HUB_IN, HUB_OUT = 61, 155           # (two and four states before a final state of the chain: 63, 159)


def hub_quads(extra, KQ):
    """Quads of a row that starts a lane (its first quad is q0 = 0 mod KQ) and has `extra` lane ends before its last quad."""
    return (extra + 1) if KQ == 1 else KQ if extra == 0 else KQ * extra + KQ // 2 + 1


def hub_graph(wl, extra, KQ):
    """A chain of 260 states with two hubs: state 61 has 4 n - 1 arcs INTO it, state 155 has 4 n - 1 arcs OUT of it, n =
    hub_quads(extra, KQ).  Each hub has a pdf of its own and is an initial state; the chain's rows have one quad (two where a hub's arc
    is the fifth of a row), so for n > 2 the hubs are the first rows of the forward and of the backward numbering."""
    def make():
        S, P = 260, 32
        n_arcs = 4 * hub_quads(extra, KQ) - 1
        base = _chain(wl, f"qhub{extra}_{KQ}", S, np.arange(S) % (P - 2), P, every=32)
        rng = np.random.default_rng(900 + 10 * extra + KQ)
        arcs = set(zip(base.src.tolist(), base.dst.tolist()))
        plain = np.setdiff1d(np.arange(S), [HUB_IN, HUB_OUT])
        final_idx = np.setdiff1d(base.final_idx, [HUB_OUT])
        have = sum(1 for (i, j) in arcs if j == HUB_IN)
        arcs |= set((int(s), HUB_IN) for s in [s for s in np.roll(plain, -7) if (int(s), HUB_IN) not in arcs][: max(0, n_arcs - have)])
        have = sum(1 for (i, j) in arcs if i == HUB_OUT)
        arcs |= set((HUB_OUT, int(s)) for s in [s for s in np.roll(plain, -19) if (HUB_OUT, int(s)) not in arcs][: max(0, n_arcs - have)])
        key = np.unique(np.array([i * S + j for i, j in arcs], dtype=np.int64))
        src, dst = key // S, key % S
        w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.05, final_idx, rng.random(final_idx.size) + 0.05)
        init_idx = np.union1d(base.init_idx, [HUB_IN, HUB_OUT])
        iw = rng.random(init_idx.size) + 0.1
        s2p = np.asarray(base.state2pdf).copy()
        s2p[HUB_IN], s2p[HUB_OUT] = P - 2, P - 1
        return wl.GraphSpec(f"qhub{extra}_{KQ}", S, init_idx, np.log(iw / iw.sum()), src, dst, w, final_idx, fw, s2p.astype(np.int32), P)
    return _memo(("q_hub", extra, KQ), make)


def hub_case(wl, extra, KQ):
    g = hub_graph(wl, extra, KQ)
    return g, emissions(3, 10, g.P, 7400 + 10 * extra + KQ), np.asarray((10, 6, 2), dtype=np.int32)


def many_finals(wl):
    """A chain of 280 states of which every fourth is final: 71 arcs into the phony final state, 18 quads -- the first row of the
    forward numbering and a long row at KQ = 1 and at KQ = 5.  Its emission is -inf in every frame but the one behind the last, so
    the forward pass skips its long walk in every step but the last.  Backward the phony row is its self loop alone, one quad: the
    long rows the backward pass walks are the out-hubs of hub_graph."""
    return _memo("q_finals", lambda: _chain(wl, "qfinals", 280, np.arange(280) % 24, 24, every=4))


def many_finals_case(wl):
    g = many_finals(wl)
    return g, emissions(3, 10, g.P, 7500), np.asarray((10, 4, 2), dtype=np.int32)


LATE_HUB, LATE_HUB_ARCS, LATE_HUB_KQ = 155, 39, (1, 2)


def late_hub_graph(wl):
    """A long row in the backward pass's GENERIC loop (positions from RPT x NT on, summed through row_total).  Forward a long row is
    always among the first rows; backward the pdfs are ordered by their rows' mean quad count, so the hub comes late if its pdf is
    the lightest: 260 states on 8 pdfs, every sixth state (the hub, state 155, among them) on pdf 7 with arcs to itself and the next
    two states -- one quad --, the others with arcs to themselves and the next five -- two quads --; the hub has 39 arcs out of it, 10
    quads: 9 lane ends at KQ = 1, 4 or 5 at KQ = 2.  At one wave it is the first row of pdf 7, behind some 215 rows."""
    def make():
        S, P = 260, 8
        rng = np.random.default_rng(931)
        s2p = np.where(np.arange(S) % 6 == 5, P - 1, np.arange(S) % (P - 1)).astype(np.int32)
        assert s2p[LATE_HUB] == P - 1
        arcs = set()
        for s in range(S):
            arcs |= set((s, s + k) for k in range(3 if s2p[s] == P - 1 else 6) if s + k < S)
        init_idx = np.union1d(np.arange(0, S, 16), [LATE_HUB])
        final_idx = np.setdiff1d(np.union1d(np.arange(15, S, 16), [S - 2, S - 1]), [LATE_HUB])
        have = sum(1 for (i, j) in arcs if i == LATE_HUB)
        cand = [int(t) for t in np.roll(np.arange(S), -19) if t != LATE_HUB and (LATE_HUB, int(t)) not in arcs]
        arcs |= set((LATE_HUB, t) for t in cand[: LATE_HUB_ARCS - have])
        key = np.unique(np.array([i * S + j for i, j in arcs], dtype=np.int64))
        src, dst = key // S, key % S
        w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.05, final_idx, rng.random(final_idx.size) + 0.05)
        iw = rng.random(init_idx.size) + 0.1
        return wl.GraphSpec("qlatehub", S, init_idx, np.log(iw / iw.sum()), src, dst, w, final_idx, fw, s2p, P)
    return _memo("q_latehub", make)


def late_hub_case(wl):
    g = late_hub_graph(wl)
    return g, emissions(3, 10, g.P, 7450), np.asarray((10, 6, 3), dtype=np.int32)


# ---- the exact fallback
FALLBACK_ROWS = (1, 4, 5, 8, 9)
FALLBACK_ENVS = {"lds": dict(kq=1), "global_fast": dict(kq=1, no_xcsr=True), "global_plain": dict(kq=5)}


def deep_graph(wl):
    """A left-to-right graph of 240 states, initial state 0 alone.  State t of the first half has FALLBACK_ROWS[t % 5] arcs INTO it
    (from t - 1 alone, or from t, t - 1, ..., a self loop included), state s of the second half as many OUT of it (to s + 1 alone, or
    to s, s + 1, ...): rows of 1, 4, 5, 8 and 9 arcs in both directions -- one chunk of the 4-wide walk, one chunk and its clamped
    tail, two chunks, two and a tail.  Final: the last state."""
    def make():
        S, H = 240, 120
        rng = np.random.default_rng(41)
        arcs = set()
        for t in range(S):
            n = FALLBACK_ROWS[t % 5]
            offs = [1] if n == 1 else list(range(n))
            if t < H:
                arcs |= set((t - k, t) for k in offs if t - k >= 0)
            if t >= H - 1:
                arcs |= set((t, t + k) for k in offs if t + k < S)
        key = np.unique(np.array([i * S + j for i, j in arcs], dtype=np.int64))
        src, dst = key // S, key % S
        final_idx = np.array([S - 1])
        w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.2, final_idx, np.full(1, 0.3))
        return wl.GraphSpec("qdeep", S, np.array([0]), np.array([0.0]), src, dst, w, final_idx, fw, (np.arange(S) % 30).astype(np.int32), 30)
    return _memo("q_deep", make)


def deep_case(wl):
    """(graph, V [4, 16, 30], lens).  deep_graph with every 12th state initial (from state 0 alone no path of 16 frames reaches the final
    state), under N(0, 1) emissions times 12: the paths of one frame differ by tens of nats and a frame's vector spans far more than
    the 62 nats of the linear sums -- rows that are alive and underflowed --, while forward the states further than n arcs from an
    initial state, and backward the many states further than the remaining frames from the final state, are dead."""
    g0 = deep_graph(wl)
    def make():
        init_idx = np.arange(0, g0.S, 12)
        return dataclasses.replace(g0, name="qdeep12", init_idx=init_idx, init_w=np.full(init_idx.size, -np.log(init_idx.size)))
    g = _memo("q_deep12", make)
    V = (12.0 * np.random.default_rng(7600).standard_normal((4, 16, g.P))).astype(np.float32)
    return g, V, np.asarray((16, 16, 9, 3), dtype=np.int32)


def sharp_case(wl):
    """mixed300 under sharp emissions consistent with a path of the graph (workloads.path_consistent_emissions, sigma = 150: the pdfs off
    the path lie some 150 nats below it)."""
    g = mixed300(wl)
    V = wl.path_consistent_emissions(g, 4, 14, 150.0, seed=3)
    return g, V, np.asarray((14, 14, 14, 14), dtype=np.int32)


# ---- the pdf count
P_EDGES_ONE_WAVE = (7, 8, 9, 63, 64, 65, 127, 128, 129, 200)
P_EDGES_TWO_WAVES = (127, 128, 129)
PDF_SIZES = (1, 8, 9, 17)      # states of the pdfs 0 .. 3; pdf 4 has none
EMPTY_PDF = 4


def pdf_edge_graph(wl, P):
    """A lexicon graph of 300 states (two hubs) on P pdfs: pdf 0 holds 1 state, pdf 1 8, pdf 2 9, pdf 3 17 (pdf_sums: 8 lanes per pdf --
    less than one pass, one pass, one more, two passes and one more), pdf 4 none; the other states are dealt to the pdfs P - 1,
    P - 2, ..., 5 in turn, so the last pdfs have states whatever P."""
    def make():
        g = trimmed(wl.lexicon_fsm(300, max(P, 8), seed=600 + P, hubs=2))
        first = np.repeat(np.arange(4), PDF_SIZES)
        rest = P - 1 - np.arange(g.S - first.size) % (P - 5)
        s2p = np.concatenate([first, rest])[np.random.default_rng(601).permutation(g.S)]
        return dataclasses.replace(g, name=f"qpedge{P}", state2pdf=s2p.astype(np.int32), P=P)
    return _memo(("q_pedge", P), make)


def pdf_edge_case(wl, P):
    """(graph, V [3, 11, P], lens): pdf P - 1, the first pdf of the last 64-lane pass and the pdfs 0 .. 3 lie 3 nats above the others'
    mean."""
    g = pdf_edge_graph(wl, P)
    V = emissions(3, 11, P, 7700 + P)
    V[..., P - 1] += 3.0
    V[..., last_pass_pdf(P)] += 3.0
    V[..., :4] += 3.0
    return g, V, np.asarray((11, 6, 2), dtype=np.int32)


def last_pass_pdf(P):
    """The first pdf of the last 64-lane pass of the emission staging and of finish_frame that holds a real pdf (5 at the least: the
    pdfs below have their fixed sizes)."""
    return max(5, 64 * ((P - 1) // 64))


# ---- the wave count
WAVE_CASES = [(9, 1), (9, 2), (9, 3), (9, 12), (9, 16), (15, 8)]   # (MM_KQ, MM_NWAVES): fin_wave 0 / 2, the priority branch from 12 on


def big_graph(wl):
    """About 2000 states, 9000 quads per direction: enough rows for 16 waves at two rows per thread."""
    return _memo("q_big", lambda: trimmed(wl.lfmmi_denominator(2000, 84, seed=0)))


def big_case(wl):
    g = big_graph(wl)
    return g, emissions(2, 8, g.P, 7800), np.asarray((8, 5), dtype=np.int32)


# ---- the lengths
LENGTHS_N = 12


def lengths_graph(wl):
    """mixed300 with its first final state made an initial state as well: a path of ONE frame exists, so every length from 1 on has an
    accepting path and the kernel's len == 1 code (a one-step loop with n == len, no frame-2 finish, one half of the pdf sums' ring)
    runs to its end instead of leaving at log Z = -inf."""
    def make():
        g = mixed300(wl)
        f = int(np.setdiff1d(g.final_idx, g.init_idx)[0])
        init_idx = np.append(g.init_idx, f)
        o = np.argsort(init_idx)
        iw = np.append(np.exp(g.init_w) * 0.9, 0.1)
        return dataclasses.replace(g, name="qlengths", init_idx=init_idx[o], init_w=np.log(iw[o]))
    return _memo("q_lengths", make)


LENGTHS_DEAD = (0, 7)


def lengths_case(wl):
    """lengths_graph, one utterance per length 0 .. 5 and N = 12, and an eighth of full length whose frame 6 is -inf for every pdf: no
    accepting path.  Deliberately dead: the length 0 and the eighth (LENGTHS_DEAD); every other length has a path."""
    g = lengths_graph(wl)
    V = emissions(8, LENGTHS_N, g.P, 7900)
    V[7, 6, :] = -np.inf
    return g, V, np.asarray((0, 1, 2, 3, 4, 5, LENGTHS_N, LENGTHS_N), dtype=np.int32)


# state counts that are a multiple of 32: the padded vector length of the packer and of the kernels once differed there
MULT32_S1 = (32, 64, 96, 128, 160, 256)


# ---- the float64 references
def state_posteriors(oracle, graphs_mod, g, V, lens, key):
    """The float64 oracle's posteriors per STATE [B, N, S]: the same graph on the identity state map, every state's emission its pdf's."""
    def make():
        gi = dataclasses.replace(g, state2pdf=np.arange(g.S, dtype=np.int32), P=g.S)
        Vs = np.ascontiguousarray(V[:, :, np.asarray(g.state2pdf)])
        gam, ttl = reference(oracle, graphs_mod, [gi] * V.shape[0], Vs, lens)
        gam = gam.copy()
        gam[~np.isfinite(ttl)] = 0.0
        return gam
    return _memo(("q_state", key), make)


def alpha_beta(oracle, graphs_mod, g, v, n):
    """(alpha, beta) [S + 1, n + 1] in nats of one utterance (v [N, P], n frames) by the float64 oracle."""
    o, oc = oracle
    vh = o.expand(np.ascontiguousarray(v[:n].T, dtype=np.float64), n, o.LOG)
    _, _, A, Bm = oc.single(graphs_mod.to_oracle(o, g), g.state2pdf, g.P, vh, want_ab=True)
    return A, Bm
