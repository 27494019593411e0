"""Fixtures of the Viterbi row-lane tests (tests/test_viterbi_inputs.py without a GPU, tests/test_gpu_viterbi_rows.py on one):
graphs whose weights sit on a grid, so that exact ties are frequent and the tie rule of the back-pointers (the lowest source state
among the maximisers) decides the best path; graphs for every layout of mm_vit_kernel<N4,N2,NJ>, every lane-group width of a row,
the size limits of the form and a back-trace ring that wraps; and a small NumPy max-plus reference whose tie rule can be switched,
which shows that a wrong rule, a forgotten lane or a wrong seam of the ring would change the paths these fixtures give.

All arithmetic is float32 in the kernels' order (one add per arc, a max, one add of the emission).  On the grid every sum is exact,
so scores do not depend on the order of the adds at all."""
import dataclasses
import re

import numpy as np

Q = 0.5  # the grid of the weights; emissions are round(2 * randn) / 2
LENS = [70, 61, 52, 43, 1, 0]  # group 1: B = 6, N = 70
N1 = 70
WIDTHS = (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255)  # arcs of the rows of states 10 + 3 i of `widths`
# R of mm_vit_backtrace_kernel for the ring cases, by the launcher's arithmetic (min(64, room / (2 * row stride))); the GPU test
# asserts these against kernels("tropical") of the batch that ran, the CPU test cuts the seams they imply
RING_R = {"den60": 64, "chain90": 9}
RING_N = {"den60": 131, "chain90": 40}


def ring_lens(name):
    R = RING_R[name]
    return [131, 129, 128, 127, 65, 64, 63, 2] if name == "den60" else [R - 1, R, R + 1, 2 * R, 2 * R + 1, 4 * R + 1, 40]


def quantised(g, q=Q):
    """g with arc, initial and final weights rounded to multiples of q."""
    r = lambda x: np.round(np.asarray(x, dtype=np.float64) / q) * q + 0.0  # (+ 0.0: no negative zeros)
    return dataclasses.replace(g, name=g.name + "_q", w=r(g.w), init_w=r(g.init_w), final_w=r(g.final_w))


def emissions(B, N, P, seed):
    rng = np.random.default_rng(seed)
    return (np.round(rng.standard_normal((B, N, P)) * 2) / 2).astype(np.float32)


def chain_fsm(wl, S, P=20, seed=12, final_every=30):
    """A chain with self loops: every state initial, every `final_every`-th final."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.arange(S), np.arange(S - 1)])
    dst = np.concatenate([np.arange(S), np.arange(1, S)])
    final_idx = np.arange(0, S, final_every)
    w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.05, final_idx, rng.random(final_idx.size) + 0.05)
    iw = rng.random(S) + 0.1
    return wl.GraphSpec(f"chain{S}", S, np.arange(S), np.log(iw / iw.sum()) + np.log(S), src, dst, w, final_idx, fw,
                        rng.integers(0, P, S).astype(np.int32), P)


def widths_fsm(wl, widest=255, S=300, P=20, seed=11):
    """chain_fsm(300) in which state 10 + 3 i has exactly WIDTHS[i] in-arcs: its self loop, the chain's arc and the lowest-numbered
    other states.  `widest`: the arcs of the last of them (256: one more than a one-byte back-pointer can name).  Every state is
    initial (the high lanes of a wide row hold live sources from frame 2 on) and the first final state lies behind the wide rows."""
    g = chain_fsm(wl, S, P, seed)
    rng = np.random.default_rng(seed + 1)
    src, dst = [g.src], [g.dst]
    for i, width in enumerate(WIDTHS[:-1] + (widest,)):
        t = 10 + 3 * i
        extra = np.setdiff1d(np.arange(S), [t - 1, t])[: width - 2]
        src.append(extra), dst.append(np.full(extra.size, t))
    src, dst = np.concatenate(src), np.concatenate(dst)
    # (weights that are NOT normalised per source state: an arc out of a state with 13 successors is as cheap as the chain's, so the
    # many arcs into a wide row compete, from every lane, and the row is worth entering)
    final_idx = np.arange(59, S, 30)
    w, fw, init_w = -3.0 * rng.random(src.size), -3.0 * rng.random(final_idx.size), -3.0 * rng.random(S)
    return dataclasses.replace(g, name=f"widths{widest}", src=src, dst=dst, w=w, init_w=init_w, final_idx=final_idx, final_w=fw)


BUILDERS = {
    "small15": lambda wl: wl.random_fsm(50, 6, 3.0, seed=4),
    "lex15": lambda wl: wl.lexicon_fsm(900, 20),
    "den24": lambda wl: wl.lfmmi_denominator(200, 84),
    "den60": lambda wl: wl.lfmmi_denominator(400, 84),
    "widths": lambda wl: widths_fsm(wl, 255),
    "widths256": lambda wl: widths_fsm(wl, 256),
    # S + 1 = 5760 rows: 90 segments of 64 single-lane rows, every position of every wave.  (Three final states: the phony final
    # state's row of 4 arcs shares a segment.  With more than 4 it takes lanes and a segment of its own, and the largest chain
    # that fits is 64 rows shorter: chain90f.)
    "chain90": lambda wl: chain_fsm(wl, 5759, final_every=1920),
    "chain91": lambda wl: chain_fsm(wl, 5760, final_every=1920),  # one row more than the form holds
    "chain90f": lambda wl: chain_fsm(wl, 5696, final_every=30),   # 89 segments + the phony row's (190 final arcs + 1, 64 lanes)
    "chain91f": lambda wl: chain_fsm(wl, 5697, final_every=30),
}
# what the packer makes of them (asserted on the GPU from kernels("tropical")): N4, N2 of mm_vit_kernel, None = no form
LAYOUT = {"small15": (1, 5), "lex15": (1, 5), "den24": (2, 4), "den60": (6, 0), "widths": (1, 5), "widths256": None,
          "chain90": (1, 5), "chain91": None, "chain90f": (1, 5), "chain91f": None}
# seeds of group 1's emissions: of the first 120, those whose best paths (by the reference) have ties across lanes in the most
# group widths -- den24, den60 in all of theirs, widths in lg 2 .. 6 -- and change most under "highest source among ties"
SEED1 = {"small15": 13, "lex15": 53, "den24": 37, "den60": 29, "widths": 119}
GROUP1 = ["small15", "lex15", "den24", "den60", "widths"]
_graphs = {}


def graph(wl, name, quant=True):
    """The fixture `name`, on the grid (quant) or with the continuous weights its builder ships."""
    if (name, quant) not in _graphs:
        g = BUILDERS[name](wl)
        _graphs[(name, quant)] = quantised(g) if quant else g
    return _graphs[(name, quant)]


def with_pdfs(g, P):
    """g on P pdfs: state s on pdf (P - 1 - s) % P.  (Counted down from P - 1: the 200 states of `den24` then use the LAST pdfs of
    every P, the 256th included, where s % P would leave the pdfs beyond 199 without a state.)"""
    return dataclasses.replace(g, name=f"{g.name}_P{P}", state2pdf=((P - 1 - np.arange(g.S)) % P).astype(np.int32), P=P)


def case1(wl, name, quant=True):
    """Group 1: (graph, V [6, 70, P], lens)."""
    g = graph(wl, name, quant)
    return g, emissions(len(LENS), N1, g.P, SEED1[name]), np.asarray(LENS, dtype=np.int32)


def case_ring(wl, name):
    """(graph, V, lens) of a ring case.  On the chain the cumulated scores of a state and of the one before it keep their order for
    many frames, so neighbouring rows of back-pointers mostly agree and a seam one row off would not show: there the emissions
    carry a bonus of 6 along a trajectory that ends in a final state, stays or advances at random and advances INTO every seam's
    frame -- the row of the seam then says "from the state before", the row after it "from the same state"."""
    g = graph(wl, name)
    lens = np.asarray(ring_lens(name), dtype=np.int32)
    V = emissions(lens.size, RING_N[name], g.P, 31 + sorted(BUILDERS).index(name))
    if name == "chain90":
        rng = np.random.default_rng(32)
        for b, L in enumerate(lens.tolist()):
            steps = rng.integers(0, 2, L)  # steps[n]: the move into frame n (0-based)
            steps[seam_frames(L, RING_R[name])] = 1
            traj = int(g.final_idx[1 + b % 2]) - (np.cumsum(steps[::-1])[::-1] - steps)
            V[b, np.arange(L), np.asarray(g.state2pdf)[traj]] += 6.0
    return g, V, lens


def case_pdfs(wl, name, P):
    """(graph on P pdfs, V [4, 40, P], lens): the last pdf and, where the pdfs outnumber the states, the pdf of the last state (it is in the FIRST
    block of 64) 3 above the others' mean, so that the best paths pass their states."""
    g = with_pdfs(graph(wl, name), P)
    V = emissions(4, 40, P, 77 + P)
    V[..., P - 1] += 3.0
    if P > g.S:
        V[..., int(g.state2pdf[-1])] += 3.0
    return g, V, np.asarray([40, 33, 21, 1], dtype=np.int32)


P_CASES = [("den24", 127), ("den24", 128), ("den24", 255), ("den24", 256), ("lex15", 128), ("den60", 255)]
P_INSTANCE = {("den24", 127): (2, 4, 2), ("den24", 128): (2, 4, 4), ("den24", 255): (2, 4, 4), ("den24", 256): None,
              ("lex15", 128): (1, 5, 4), ("den60", 255): (6, 0, 4)}


def instance(kernels):
    """(N4, N2, NJ, R) of a kernels("tropical") string, None if the row-lane kernels do not run."""
    m = re.search(r"mm_vit_kernel<(\d+),(\d+),(\d+)> \+ mm_vit_backtrace_kernel<csr in LDS, R=(\d+)>", kernels)
    assert (m is not None) == ("mm_vit_kernel" in kernels), kernels
    return tuple(int(x) for x in m.groups()) if m else None


# ---- the reference
def lg_of(width):
    """log2 of the lanes a row of `width` arcs gets in the Viterbi form: at most 4 arcs per lane, at most 64 lanes."""
    lg = 0
    while -(-max(width, 1) // (1 << lg)) > 4 and lg < 6:
        lg += 1
    return lg


class Tables:
    """The rows of T_hat' padded to the widest: SRC / W [S + 1, D] by ascending source (arc number k of a row is its column),
    -inf beyond a row's arcs; the phony final state is row S."""

    def __init__(self, g):
        S = g.S
        src = np.concatenate([g.src, g.final_idx, [S]]).astype(np.int64)
        dst = np.concatenate([g.dst, np.full(g.final_idx.size, S), [S]]).astype(np.int64)
        w = np.concatenate([g.w, g.final_w, [0.0]]).astype(np.float32)
        o = np.lexsort((src, dst))
        src, dst, w = src[o], dst[o], w[o]
        self.deg = np.bincount(dst, minlength=S + 1)
        k = np.arange(src.size) - np.concatenate([[0], np.cumsum(self.deg)])[dst]
        self.D = int(self.deg.max())
        self.SRC = np.zeros((S + 1, self.D), dtype=np.int64)
        self.W = np.full((S + 1, self.D), -np.inf, dtype=np.float32)
        self.SRC[dst, k], self.W[dst, k] = src, w
        self.lg = np.array([lg_of(d) for d in self.deg])
        self.init = np.full(S + 1, -np.inf, dtype=np.float32)
        self.init[g.init_idx] = np.asarray(g.init_w, dtype=np.float32)
        self.pdf = np.concatenate([g.state2pdf, [g.P]]).astype(np.int64)
        self.S = S


_tables = {}


def tables(g):
    if id(g) not in _tables:
        _tables[id(g)] = (g, Tables(g))
    return _tables[id(g)][1]


@dataclasses.dataclass
class Result:
    path: np.ndarray   # [L] states, all -1 where there is no accepting path
    score: np.float32
    bp: np.ndarray     # [L + 1, S + 1] source state of the arc the rule picks (-1: dead), row 0 unused
    tied: np.ndarray   # [L + 1, S + 1] live cell with >= 2 maximisers
    cross: np.ndarray  # ... whose two lowest maximising arc numbers sit in different lanes of the row's group
    live: np.ndarray


def reference(g, V, L, rule="lowest", seams=()):
    """Best path of one utterance (V [N, P], length L).  rule: which maximiser a back-pointer names -- "lowest" source (the
    specification), "highest" source, or "lane0": the first maximum among the arcs of the lane that holds arc 0 (arcs 0, g, 2 g, ...
    of a row on g lanes: a reduction that forgets the other lanes).  seams: rows of bp in whose place the chase reads the row of the
    frame after (a chunk of the back-trace ring copied one row off: the row at its seam is cut out)."""
    t = tables(g)
    S, P, L = t.S, g.P, int(L)
    rows = np.arange(S + 1)
    Vh = np.full((L + 1, P + 1), -np.inf, dtype=np.float32)
    Vh[:L, :P] = V[:L]
    Vh[L, P] = 0.0
    a = t.init + Vh[0][t.pdf]
    shape = (L + 1, S + 1)
    bp, tied, cross, live = np.full(shape, -1, dtype=np.int64), np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    grp = 1 << t.lg
    lane0 = (np.arange(t.D)[None, :] % grp[:, None]) == 0
    for n in range(1, L + 1):
        vals = t.W + a[t.SRC]  # (float32 + float32)
        M = vals.max(axis=1)
        alive = M > -np.inf
        ismax = (vals == M[:, None]) & alive[:, None]
        first = ismax.argmax(axis=1)
        rest = ismax.copy()
        rest[rows, first] = False
        second = rest.argmax(axis=1)
        live[n], tied[n] = alive, rest.any(axis=1)
        cross[n] = tied[n] & (first % grp != second % grp)
        if rule == "lowest":
            k = first
        elif rule == "highest":
            k = t.D - 1 - ismax[:, ::-1].argmax(axis=1)
        else:
            k = np.where(lane0, vals, -np.inf).argmax(axis=1)
        bp[n] = np.where(alive, t.SRC[rows, k], -1)
        a = (M + Vh[n][t.pdf]).astype(np.float32)
    score = a[S] if L >= 1 else np.float32(-np.inf)
    path = np.full(L, -1, dtype=np.int64)
    if score > -np.inf:
        s = S
        for n in range(L, 0, -1):
            s = bp[n + 1 if n in seams else n][s]  # (a seam is never the last frame: n + 1 <= L)
            path[n - 1] = s
    return Result(path, np.float32(score), bp, tied, cross, live)


def seam_frames(L, R):
    """The frames (of the kernel's numbering, 2 .. L + 1, here minus one: rows of `bp`) that are the LAST row of a chunk of the
    back-trace other than the first: chunk c holds the kernel's frames hi - R + 1 .. hi, hi = L + 1 - c R."""
    return [hi - 1 for hi in range(L + 1 - R, 1, -R)]
