"""Fixtures of the stream-kernel tests (tests/test_stream_inputs.py without a GPU, tests/test_gpu_stream_instances.py on one): graphs
and inputs that reach every instance of mm_stream_kernel<NJ,H> (csrc/mm_stream.hip) -- pdf counts on both sides of every step of
mm_stream_nj and at the form's maximum, rows of every lane-group width in both directions and several whole-wave rows per set of a
team, pdfs without states, and a graph whose compiled state count is exactly the form's limit (16-bit LDS byte offsets in the
records: S1 <= 16370).  NumPy only; `wl` is the package's workloads module (GraphSpec, random_fsm).

The properties the GPU tests rest on (the last pdfs carry mass, a lost arc of a grouped row is visible, the states near the limit hold
mass) are asserted from the float64 oracle alone in tests/test_stream_inputs.py."""
import dataclasses

import numpy as np

N = 19
P_LENS = (19, 9, 8, 1)       # group P: 8 and 9 frames straddle the combine kernel's groups of 8 frames
R_LENS = (19, 12, 2)
S_LENS = (5, 3)              # group S: N = 5
P_EDGES = (127, 128, 255, 256, 511, 512, 1023)
S1_LIMIT = 16370             # mm_stream_build: 4 * position <= 65 532 with up to 12 positions of padding
P_MAX = 1023                 # P1 = P + 1 <= 1024
# rows of these lengths exist in each direction of mid_row_graph: the ends of the classes 1 lane (<= 32), 2 lanes (33 .. 64), 4 lanes
# (65 .. 128), a whole wave (> 128)
EDGE_ROWS = (32, 33, 64, 65, 128, 129)
_HUB_ROWS = EDGE_ROWS + (40, 47, 50, 56, 59, 63) + (70, 81, 90, 101, 110, 127) + (150, 200, 260, 300)
EMPTY_PDFS = (0, 7, 8, 9, 31, 63, 64, 65, 100, 127, 128, 150, 191, 192, 200, 255, 256, 257, 280, 290, 298, 299)


def stream_nj(P):
    """NJ of mm_stream_kernel<NJ,H> for P pdfs, as the issue of these tests states it (P1 = P + 1: at most 128 gives 2, 256 gives 4,
    512 gives 8, else 16) -- written down here independently of mm_stream_nj, which the kernels() text reads."""
    P1 = P + 1
    return 2 if P1 <= 128 else 4 if P1 <= 256 else 8 if P1 <= 512 else 16


def last_pass_pdf(P):
    """The first pdf of the last 64-lane staging pass that holds a real pdf: 64 (NJ - 1) where P1 = P + 1 fills its NJ passes (P = 127,
    255, 511, 1023); one step past a boundary of mm_stream_nj (P = 128, 256, 512) the passes beyond pdf P hold nothing, and it is
    64 ((P - 1) // 64)."""
    return min(64 * (stream_nj(P) - 1), 64 * ((P - 1) // 64))


def extended(g):
    """(I, J, W) of T_hat without the phony state's self loop: the arcs, then the final arcs (into state S)."""
    return (np.concatenate([g.src, g.final_idx]).astype(np.int64), np.concatenate([g.dst, np.full(g.final_idx.size, g.S)]).astype(np.int64),
            np.concatenate([g.w, g.final_w]))


def degrees(g):
    """(in-degree, out-degree) [S + 1] of T_hat, the phony final state and its self loop included: the row lengths of the forward
    and of the backward direction's stream form."""
    I, J, _ = extended(g)
    I, J = np.append(I, g.S), np.append(J, g.S)
    return np.bincount(J, minlength=g.S + 1), np.bincount(I, minlength=g.S + 1)


def keep_arcs(g, keep):
    """g with the entries of extended(g) that `keep` selects; nothing is renormalised."""
    n = g.src.size
    ka, kf = keep[:n], keep[n:]
    return dataclasses.replace(g, src=g.src[ka], dst=g.dst[ka], w=g.w[ka], final_idx=g.final_idx[kf], final_w=g.final_w[kf])


def row_positions(g, direction):
    """Per entry of extended(g): (its row, its index within the row) in the row view of `direction` -- 0: the arcs INTO a state by
    ascending source, 1: the arcs OUT of a state by ascending destination (the CSR order the forms are filled in)."""
    I, J, _ = extended(g)
    row, other = (J, I) if direction == 0 else (I, J)
    o = np.lexsort((other, row))
    first = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=g.S + 1))])
    k = np.empty(row.size, dtype=np.int64)
    k[o] = np.arange(row.size) - first[row[o]]
    return row, k


def without_last_arcs(g, lengths, directions=(0, 1)):
    """g without the last arc of every row of a length in `lengths`, in the row view of each of `directions`.  (The phony state's self
    loop is its row's last arc by source; a GraphSpec cannot drop it, so that row loses its last final arc.)"""
    keep = np.ones(g.src.size + g.final_idx.size, dtype=bool)
    deg = degrees(g)
    for d in directions:
        row, k = row_positions(g, d)
        real = deg[d][row] - (row == g.S)  # (entries of the row in extended(g))
        keep &= ~(np.isin(deg[d][row], lengths) & (k == real - 1))
    return keep_arcs(g, keep)


def first_pass_only(g):
    """g with the rows of more than 128 arcs cut to their first 64, in both row views: a whole-wave sum that keeps one pass."""
    keep = np.ones(g.src.size + g.final_idx.size, dtype=bool)
    deg = degrees(g)
    for d in (0, 1):
        row, k = row_positions(g, d)
        keep &= ~((deg[d][row] > 128) & (k >= 64))
    return keep_arcs(g, keep)


def emissions(B, n, P, seed):
    return (1.3 * np.random.default_rng(seed).standard_normal((B, n, P))).astype(np.float32)


# ---- the graphs
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def p_edge_graph(wl, P):
    """A random graph on P pdfs, state s on pdf (P - 1 - s) % P: counted down from P - 1, the last pdfs -- the end of the last 64-lane
    pass of the staging -- have states whatever P; s % P would leave the pdfs beyond the states empty."""
    def make():
        S = 1200 if P >= 512 else 600
        g = wl.random_fsm(S, P, 3.0, seed=1000 + P, n_init=S // 2)
        return dataclasses.replace(g, name=f"pedge{P}", state2pdf=((P - 1 - np.arange(S)) % P).astype(np.int32))
    return _memo(("p", P), make)


def case_p(wl, P):
    """Group P: (graph, V [4, 19, P], lens).  The last pdf and the first pdf of the last staging pass (last_pass_pdf) lie 3 nats above
    the others' mean: both carry posterior mass the comparison can see."""
    g = p_edge_graph(wl, P)
    V = emissions(len(P_LENS), N, P, 2000 + P)
    V[..., P - 1] += 3.0
    V[..., last_pass_pdf(P)] += 3.0
    return g, V, np.asarray(P_LENS, dtype=np.int32)


def mid_row_graph(wl):
    """1200 states on 127 pdfs.  Forty-four hub states: state 100 + 10 k has exactly _HUB_ROWS[k] arcs INTO it, state 105 + 10 k exactly
    _HUB_ROWS[k] arcs OUT of it (k < 22) -- the lengths 32, 33, 64, 65, 128, 129, eight rows in each of the classes 33 .. 64 and
    65 .. 128 and five of more than 128 arcs, per direction.  Every hub is an initial state and has a pdf of its own (the pdfs 83 ..
    126): its posterior is a column of gamma, undiluted by other states."""
    def make():
        S, P, nh = 1200, 127, len(_HUB_ROWS)
        base = wl.random_fsm(S, P - 2 * nh, 3.0, seed=77, n_init=S // 2)
        rng = np.random.default_rng(78)
        hin, hout = 100 + 10 * np.arange(nh), 105 + 10 * np.arange(nh)
        hubs = np.concatenate([hin, hout])
        arcs = set(zip(base.src.tolist(), base.dst.tolist()))
        plain = np.setdiff1d(np.arange(S), hubs)
        final_idx = np.setdiff1d(base.final_idx, hout)  # (an out-hub has no final arc: its row is its arcs)
        for t, width in zip(hin, _HUB_ROWS):   # sources: the lowest-numbered plain states that are not sources yet
            have = sum(1 for (i, j) in arcs if j == t)
            assert have <= width
            arcs |= set((int(s), int(t)) for s in [s for s in plain if (int(s), int(t)) not in arcs][: width - have])
        for t, width in zip(hout, _HUB_ROWS):  # destinations: plain states from the top down
            have = sum(1 for (i, j) in arcs if i == t)
            assert have <= width
            arcs |= set((int(t), int(s)) for s in [s for s in plain[::-1] if (int(t), int(s)) not in arcs][: width - have])
        key = np.unique(np.array([i * S + j for i, j in arcs], dtype=np.int64))
        src, dst = key // S, key % S
        w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.05, final_idx, rng.random(final_idx.size) + 0.05)
        init_idx = np.union1d(base.init_idx, hubs)
        iw = rng.random(init_idx.size) + 0.1
        s2p = np.asarray(base.state2pdf).copy()
        s2p[hubs] = P - 1 - np.arange(2 * nh)
        return wl.GraphSpec("midrows", S, init_idx, np.log(iw / iw.sum()), src, dst, w, final_idx, fw, s2p.astype(np.int32), P)
    return _memo("mid", make)


def mid_hubs():
    nh = len(_HUB_ROWS)
    return 100 + 10 * np.arange(nh), 105 + 10 * np.arange(nh)


def case_r(wl):
    return mid_row_graph(wl), emissions(len(R_LENS), N, 127, 31), np.asarray(R_LENS, dtype=np.int32)


def empty_pdf_graph(wl):
    """320 states on 300 pdfs of which EMPTY_PDFS (the first, the last, both sides of every 64-lane pass, a run of three) have no
    state: the combine kernel's range q0 .. q1 of such a pdf is empty."""
    def make():
        S, P = 320, 300
        g = wl.random_fsm(S, P, 3.0, seed=55, n_init=40)
        used = np.setdiff1d(np.arange(P), EMPTY_PDFS)
        return dataclasses.replace(g, name="emptypdfs", state2pdf=used[np.arange(S) % used.size].astype(np.int32))
    return _memo("empty", make)


def case_e(wl):
    return empty_pdf_graph(wl), emissions(3, N, 300, 56), np.asarray((19, 8, 3), dtype=np.int32)


def limit_graph(wl, S1):
    """A sparse random graph (mean degree 3 and the chain) of S1 - 1 real states -- to_fsm adds the phony final state; the tests read
    the compiled S1 -- on 1000 pdfs.  As many draws of initial states as states (about 63 % of the states are initial) and 30 % final
    states: after one frame the mass sits on states all over the numbering, so on LDS byte offsets all over the 16 bits."""
    def make():
        S = S1 - 1
        return dataclasses.replace(wl.random_fsm(S, 1000, 3.0, seed=S1, n_init=S, p_final=0.3), name=f"limit{S1}")
    return _memo(("limit", S1), make)


def case_s(wl, S1):
    return limit_graph(wl, S1), emissions(len(S_LENS), 5, 1000, 3000 + S1), np.asarray(S_LENS, dtype=np.int32)


def case_b(wl, B):
    """Group B: the 300-state graph of test_stream_kernels' forced case, N = 9, lengths that include 0 and 1."""
    g = _memo("b", lambda: wl.random_fsm(300, 11, 4.0, seed=9))
    lens = np.asarray([(9, 0, 1, 5, 8, 9, 2, 7)[b % 8] for b in range(B)], dtype=np.int32)
    return g, emissions(B, 9, 11, 4000 + B), lens


# ---- the float64 reference, once per case
def reference(oracle, graphs_mod, gs, V, lens, key=None):
    """(gamma [B, N, P] float64, ttl [B]) of a batch by the C oracle, oc.batch_shared per distinct graph; memoised under `key`."""
    def make():
        o, oc = oracle
        g_ref, t_ref = np.zeros(V.shape, dtype=np.float64), np.zeros(V.shape[0])
        for g in {id(g): g for g in gs}.values():
            idx = np.array([b for b, x in enumerate(gs) if x is g])
            gr, tr = oc.batch_shared(graphs_mod.to_oracle(o, g), g.state2pdf, g.P, V[idx], lens[idx], dtype=np.float64, nthreads=4)
            g_ref[idx], t_ref[idx] = gr, tr
        g_ref.setflags(write=False)
        t_ref.setflags(write=False)
        return g_ref, t_ref
    return make() if key is None else _memo(("ref", key), make)
