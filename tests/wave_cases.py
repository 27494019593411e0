"""Fixtures of the wave- and lane-kernel tests (tests/test_wave_lane_inputs.py without a GPU, tests/test_gpu_wave_lane_instances.py on
one): graphs and inputs that reach every instance of mm_wave_kernel<NSEG,NJ,TWO> (csrc/mm_kernel_wave.hip) and of mm_lane_kernel<NS>
(csrc/mm_kernel_lane.hip) at the sizes where each can go wrong -- pdf counts on both sides of every 64-lane pass of the emission
staging, rows of every lane-group width in both directions, pdfs of every group width of the pdf sums, the forms' limits at the value
and one beyond (1023 states, rows of 255 and 256 arcs, a pdf of 256 states, 4 and 8 pdf segments), one utterance per short length, state
counts on both sides of every lane instance, and state maps on exactly 64 pdfs.  NumPy only; `wl` is the package's workloads module.

The properties the GPU tests rest on are asserted from the float64 oracle and the host packers alone in
tests/test_wave_lane_inputs.py."""
import dataclasses

import numpy as np

import stream_cases as sc
from stream_cases import _memo, emissions

P_EDGES = (63, 64, 127, 128, 249)
HUB_ROWS = (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255)   # lane groups of 1, 2, 2, 4, 4, 8, ..., 64, 64 lanes (4 arcs per lane)
PDF_GROUPS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)
WAVE_LENS = tuple(range(13)) + (16, 17)
LANE_LENS = tuple(range(19)) + (24, 25)
LANE_EDGES = (8, 9, 16, 17, 32, 33, 64)
LANE_NS = {8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}


def last_pass_pdf(P):
    """The first pdf of the last 64-lane pass of em_stage / frame_out that holds a real pdf."""
    return 64 * ((P - 1) // 64)


def wave_nj(P):
    """NJ of mm_wave_kernel<NSEG,NJ>: NJ * 64 >= P + 1, 2 or 4 -- stated here independently of the kernels() text."""
    return 2 if P + 1 <= 128 else 4


def pdf_group_lanes(g):
    """Lanes of the pdf sums' segments (mm_engine.hip wave_pdf_table): a pdf with n states takes pow2(ceil(n / 4)) lanes, the phony
    pdf of the final state one; groups are powers of two placed largest first, so they fill ceil(lanes / 64) segments."""
    n = np.bincount(np.asarray(g.state2pdf), minlength=g.P)
    n = n[n > 0]
    return int(sum(1 << int(np.ceil(np.log2(max(1, -(-int(k) // 4))))) for k in n)) + 1


def pdf_segments(g):
    return -(-pdf_group_lanes(g) // 64)


def compile_graph(mm, wl, g):
    return mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))


def wave_segments(mm, wl, g):
    """(NSEG the registers of a compute wave must hold, state segments per direction) by the host packer, None if the graph has no
    wave form: 4 arc slots per segment; 2 pdf segments per wave when the pdf sums need more than 4."""
    cf = compile_graph(mm, wl, g)
    x = np.zeros(cf.S1, dtype=np.float32)
    try:
        st = [cf.wave_product(x, d)[1] for d in (0, 1)]
    except mm.MarkovModelsAMDError:
        return None
    ka = max(int(s[0]) for s in st)
    return max(ka // 4, 2 * (1 if pdf_segments(g) <= 4 else 2)), [int(s[1]) for s in st]


# ---- wave: the pdf count
def pdf_edge_graph(wl, P):
    """A lexicon graph of 300 states (two hubs) on P pdfs, state s on pdf (P - 1 - s) % P: counted down from P - 1, so the last
    pdfs have states whatever P."""
    def make():
        g = wl.lexicon_fsm(300, P, seed=500 + P, hubs=2)
        return dataclasses.replace(g, name=f"wpedge{P}", state2pdf=((P - 1 - np.arange(g.S)) % P).astype(np.int32))
    return _memo(("wp", P), make)


def pdf_edge_case(wl, P, B=3, N=19):
    """(graph, V [B, N, P], lens): pdf P - 1 and the first pdf of the last 64-lane pass lie 3 nats above the others' mean."""
    g = pdf_edge_graph(wl, P)
    V = emissions(B, N, P, 2000 + P + 7 * B)
    V[..., P - 1] += 3.0
    V[..., last_pass_pdf(P)] += 3.0
    lens = np.asarray([(N, N // 2, 1, N - 1, 2)[b % 5] for b in range(B)], dtype=np.int32)
    return g, V, lens


def sparse20(wl):
    """The sparse graph on 20 pdfs of the instance cases: <2,2>."""
    return _memo("sparse20", lambda: wl.lexicon_fsm(120, 20, seed=4, hubs=1))


def sparse20_case(wl, B, N):
    g = sparse20(wl)
    lens = np.asarray([(N, N // 2, 1, N - 1, 2)[b % 5] for b in range(B)], dtype=np.int32)
    return g, emissions(B, N, 20, 2100 + B), lens


def dense_wide(wl):
    """A dense graph of more than 8 state segments per direction: 150 states of mean degree 14 on 12 pdfs (<4,2>)."""
    return _memo("densewide", lambda: wl.random_fsm(150, 12, 14.0, seed=5))


# ---- wave: rows of every lane-group width
def hub_ids():
    nh = len(HUB_ROWS)
    return 20 + 16 * np.arange(nh), 28 + 16 * np.arange(nh)


def hub_graph(wl, widest=255):
    """440 states on 66 pdfs.  State 20 + 16 k has exactly HUB_ROWS[k] arcs INTO it, state 28 + 16 k exactly HUB_ROWS[k] arcs OUT
    of it: lane groups of 1 .. 64 lanes in both directions, both sides of every butterfly level.  Every hub is an initial state
    and has a pdf of its own.  The other ends of a hub's arcs are spread over the plain states (a stride per hub), so that no plain
    row grows wide.  `widest`: the arcs INTO the last in-hub (state 20 + 16 * 12) -- 256 is what 64 lanes of 4 arc slots hold, the
    most the form takes (mm_rows.cpp: a row of more than 64 x seg_stride arcs is refused); 257 is beyond it."""
    def make():
        S, nh = 440, len(HUB_ROWS)
        P = 40 + 2 * nh
        widths = HUB_ROWS[:-1] + (widest,)
        base = wl.random_fsm(S, 40, 1.2, seed=177, n_init=20, p_final=0.08)
        rng = np.random.default_rng(178)
        hin, hout = hub_ids()
        hubs = np.concatenate([hin, hout])
        # (no base arc touches a hub but the chain's: the widths below are met exactly)
        keep = ~(np.isin(base.src, hubs) | np.isin(base.dst, hubs)) | (base.dst == base.src + 1)
        arcs = set(zip(base.src[keep].tolist(), base.dst[keep].tolist()))
        plain = np.setdiff1d(np.arange(S), hubs)
        final_idx = np.setdiff1d(base.final_idx, hout)  # (an out-hub has no final arc: its row is its arcs)
        for k, (t, width) in enumerate(zip(hin, widths)):
            have = sum(1 for (i, j) in arcs if j == t)
            cand = [int(s) for s in np.roll(plain, -31 * k) if (int(s), int(t)) not in arcs]
            arcs |= set((s, int(t)) for s in cand[: width - have])
        for k, (t, width) in enumerate(zip(hout, HUB_ROWS)):
            have = sum(1 for (i, j) in arcs if i == t)
            cand = [int(s) for s in np.roll(plain, -31 * k - 13) if (int(t), int(s)) not in arcs]
            arcs |= set((int(t), s) for s in cand[: width - have])
        key = np.unique(np.array([i * S + j for i, j in arcs], dtype=np.int64))
        src, dst = key // S, key % S
        w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.05, final_idx, rng.random(final_idx.size) + 0.05)
        init_idx = np.union1d(base.init_idx, hubs)
        iw = rng.random(init_idx.size) + 0.1
        s2p = np.asarray(base.state2pdf).copy()
        s2p[hubs] = P - 1 - np.arange(2 * nh)
        return wl.GraphSpec(f"hubs{widest}", S, init_idx, np.log(iw / iw.sum()), src, dst, w, final_idx, fw, s2p.astype(np.int32), P)
    return _memo(("hubs", widest), make)


def hub_case(wl, widest=255):
    g = hub_graph(wl, widest)
    return g, emissions(3, 19, g.P, 41), np.asarray((19, 12, 2), dtype=np.int32)


# ---- wave: pdfs of every group width
def pdf_group_graph(wl, variant="base"):
    """A lexicon graph whose pdfs hold exactly PDF_GROUPS states -- 1 .. 256: groups of 1 .. 64 lanes in wave_pdf_table, 255 group
    lanes with the final state's: exactly 4 pdf segments -- on 17 pdfs of which pdf 0, pdf 8 and pdf 16 have no state.  Variants:
    "pdf257": the largest pdf holds 257 states (no group is that wide: refused); "five": a further pdf of 129 states -- 5 pdf
    segments, two per wave, the <4,.> instances -- on 18 pdfs; "five_p130": the same states on 130 pdfs, the groups spread up
    to pdf 128; "nine": a chain (_chain) with 4 pdfs of 129 states, one of 65 and 225 of one state, 514 group lanes -- more than 8 pdf segments:
    refused; "nine_fits": the same chain, its states spread evenly over the same pdfs -- it fits: the refusal is the pdf sums', not
    the rows'."""
    def make():
        sizes = {"base": PDF_GROUPS, "pdf257": PDF_GROUPS[:-1] + (257,), "five": PDF_GROUPS + (129,), "five_p130": PDF_GROUPS + (129,),
                 "nine": (129,) * 4 + (65,) + (1,) * 225, "nine_fits": (129,) * 4 + (65,) + (1,) * 225}[variant]
        S, n = int(sum(sizes)), len(sizes)
        if variant.startswith("nine"):
            P = n + 3
            ids = np.setdiff1d(np.arange(1, P - 1), [P // 2])
            s2p = np.repeat(ids, sizes) if variant == "nine" else ids[np.arange(S) % n]
            return _chain(wl, f"pdfgroups_{variant}", S, s2p[np.random.default_rng(901).permutation(S)], P, every=16)
        P = 130 if variant == "five_p130" else n + 3
        mid = P // 2
        if variant == "five_p130":  # the groups from pdf 1 up to pdf 128, the widest last
            ids = np.setdiff1d(np.unique(np.linspace(1, P - 2, 2 * n).astype(int)), [mid])[-n:]
            ids[0] = 1
        else:
            ids = np.setdiff1d(np.arange(1, P - 1), [mid])
        assert ids.size == n and ids.max() == P - 2
        g = wl.lexicon_fsm(S, P, seed=900 + n, hubs=4)
        s2p = np.repeat(ids, sizes)[np.random.default_rng(901).permutation(S)]
        return dataclasses.replace(g, name=f"pdfgroups_{variant}", state2pdf=s2p.astype(np.int32))
    return _memo(("pg", variant), make)


def pdf_group_empty(g):
    return np.setdiff1d(np.arange(g.P), np.asarray(g.state2pdf))


def pdf_group_case(wl, variant="base"):
    g = pdf_group_graph(wl, variant)
    return g, emissions(3, 25, g.P, 61), np.asarray((25, 14, 3), dtype=np.int32)


# ---- wave: the state count
LIMIT_S1 = (511, 512, 513, 1023, 1024)   # 1024 rows are 16 full segments: the most the form holds; 1023: the most pick_family's wave-first rule takes


def _chain(wl, name, S, s2p, P, every=0):
    """A left-to-right chain of S states with a self loop, the arc to the next state and the arc over it: rows of at most 3 arcs
    (4 with a final arc), one lane each.  Initial: the first three states; final: the last two -- with `every`, also every
    `every`-th state is initial and the one before it final: mass all along the chain within a few frames."""
    rng = np.random.default_rng(S)
    s = np.arange(S)
    src = np.concatenate([s, s[:-1], s[:-2]])
    dst = np.concatenate([s, s[:-1] + 1, s[:-2] + 2])
    init_idx, final_idx = np.arange(3), np.array([S - 2, S - 1])
    if every:
        init_idx = np.union1d(init_idx, s[::every])
        final_idx = np.union1d(final_idx, s[every - 1 :: every])
    w, fw = wl._normalise_rows(S, src, rng.random(src.size) + 0.2, final_idx, np.full(final_idx.size, 0.3))
    iw = rng.random(init_idx.size) + 0.2
    return wl.GraphSpec(name, S, init_idx, np.log(iw / iw.sum()), src, dst, w, final_idx, fw, np.asarray(s2p, dtype=np.int32), P)


def limit_chain(wl, S1):
    """A left-to-right chain (_chain) of S1 - 1 real states -- the compiled FSM adds the final state: S1 -- so 1023 rows are 16
    segments of 64 lanes.  On 120 pdfs, state s on pdf s % 120."""
    return _memo(("chain", S1), lambda: _chain(wl, f"chain{S1}", S1 - 1, np.arange(S1 - 1) % 120, 120))


def limit_case(wl, S1):
    """N = S1 + 8, B = 2: the full length, and the shortest length with a path (every arc skips: ceil((S - 2) / 2) + 1 frames) + 3."""
    g = limit_chain(wl, S1)
    N = S1 + 8
    return g, emissions(2, N, g.P, 3000 + S1), np.asarray((N, (g.S - 1) // 2 + 4), dtype=np.int32)


def tiny_for_wave(wl):
    """Graphs of fewer segments than an agent has compute waves: the reference's 3-state demo HMM and a 2-state graph."""
    def two():
        lw = np.log(np.array([0.5, 0.3, 0.4, 0.4]))
        return wl.GraphSpec("two", 2, np.array([0]), np.array([0.0]), np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), lw,
                            np.array([0, 1]), np.log(np.array([0.2, 0.2])), np.arange(2, dtype=np.int32), 2)
    return [_memo("l2r3", lambda: wl.l2r_hmm(3)), _memo("two", two)]


# ---- the lengths
def lengths_case(wl, g, lens, seed):
    """One utterance per length of `lens`, on one graph: (V [len(lens), max(lens), P], lens)."""
    lens = np.asarray(lens, dtype=np.int32)
    return emissions(lens.size, int(lens.max()), g.P, seed), lens


def four_segment(wl):
    """A sparse graph whose waves need the 4-segment instance: 700 lexicon states on 20 pdfs."""
    return _memo("lex700", lambda: wl.lexicon_fsm(700, 20, seed=6, hubs=2))


def path_lengths(g, nmax):
    """has[L] (L <= nmax): an accepting path of exactly L frames exists."""
    S = g.S
    A = np.zeros((S, S), dtype=bool)
    A[g.src, g.dst] = True
    fin = np.zeros(S, dtype=bool)
    fin[g.final_idx[np.isfinite(g.final_w)]] = True
    cur = np.zeros(S, dtype=bool)
    cur[g.init_idx[np.isfinite(g.init_w)]] = True
    has = [False]
    for _ in range(nmax):
        has.append(bool((cur & fin).any()))
        cur = (A.T.astype(np.int32) @ cur.astype(np.int32)) > 0
    return np.asarray(has)


# ---- lane: the graphs
def lane_dense(wl, S):
    return _memo(("ld", S), lambda: wl.dense_ergodic(S, seed=S))


def lane_sparse(wl, S, P=None):
    """random_fsm on P pdfs (default: min(S, 12) -- a many-to-one map from S = 16 on)."""
    P = P or min(S, 12)
    return _memo(("ls", S, P), lambda: wl.random_fsm(S, P, 3.0, seed=300 + S + P, n_init=3))


def lane_case(wl, g, B=4, N=21, seed=0):
    return emissions(B, N, g.P, 5000 + seed), np.asarray([(N, 9, 1, N - 1, 8, 2)[b % 6] for b in range(B)], dtype=np.int32)


PERM64 = (63 - (np.arange(64) * 27 + 0) % 64).astype(np.int32)  # state 0 on pdf 63, 27 odd: a permutation; no fixed order


def perm64(wl):
    """64 states on 64 pdfs through a permutation that is not the identity; state 0 -- always initial -- holds pdf 63."""
    def make():
        g = wl.random_fsm(64, 64, 4.0, seed=640, n_init=8)
        return dataclasses.replace(g, name="perm64", state2pdf=PERM64.copy())
    return _memo("perm64", make)


def many_to_one_64(wl):
    """40 states on 64 pdfs: pdf 63 holds the states 0, 1 and 2 (state 0 is initial), pdf 0 none, the others the pdfs 5, 7, 9, ...
    and 62 -- the pdfs 1 .. 4, the even ones up to 60 and a few more hold no state."""
    def make():
        g = wl.random_fsm(40, 64, 4.0, seed=641, n_init=6)
        s2p = np.concatenate([[63, 63, 63], 5 + 2 * np.arange(29), [62] * 8]).astype(np.int32)
        assert s2p.size == 40
        return dataclasses.replace(g, name="m2o64", state2pdf=s2p)
    return _memo("m2o64", make)


def empty_last_64(wl):
    """50 states on 64 pdfs, state s on pdf (3 s + 1) % 63: pdf 63 has no state -- its range pdf_ptr[63] .. pdf_ptr[64] is empty, and
    its upper end is entry 64 of the table."""
    def make():
        g = wl.random_fsm(50, 64, 4.0, seed=642, n_init=6)
        return dataclasses.replace(g, name="emptylast64", state2pdf=((3 * np.arange(50) + 1) % 63).astype(np.int32))
    return _memo("emptylast64", make)


def map64_case(wl, g):
    """(V [4, 21, 64], lens); pdf 63 lies 3 nats above the others' mean."""
    V, lens = lane_case(wl, g, seed=64)
    V[..., 63] += 3.0
    return V, lens


# ---- lane: an input the float64 linear recursion cannot hold
REDO_S = 64


def redo_case(wl):
    """(graph, V [4, 64, 64], lens): the 64-state left-to-right HMM, 64 frames.  Utterance 0: every frame's emission is 0 for state 0
    and -250 nats for every other state -- the one path of 64 frames has left state 0 after the first frame, and state k's forward
    value lies 360 k log2 below state 0's: beyond a double's range from state 3 on.  Utterance 1: N(0, 1.3) emissions at full
    length; 2: one frame short of any path; 3: utterance 0's input, 63 frames -- no path."""
    g = _memo("l2r64", lambda: wl.l2r_hmm(REDO_S))
    V = emissions(4, 64, 64, 77)
    V[0] = -250.0
    V[0, :, 0] = 0.0
    V[3] = V[0]
    return g, V, np.asarray((64, 64, 63, 63), dtype=np.int32)


def lane_forward_emulated(g, V, n):
    """The lane kernel's forward recursion in numpy float64, its range included: linear domain, emissions 2^(e - E) relative to the
    frame's maximum, every vector divided by the power of two of the last vector's maximum, values below 2^-1022 flushed to zero.
    Returns (Z = sum_i alpha_n(i) omega_i in that scaling, the number of states whose value was flushed on the way)."""
    S = g.S
    T = np.zeros((S, S))
    np.add.at(T, (g.src, g.dst), np.exp(g.w))
    a = np.zeros(S)
    a[g.init_idx] = np.exp(g.init_w)
    om = np.zeros(S)
    om[g.final_idx] = np.exp(g.final_w)
    e2 = V[:n][:, np.asarray(g.state2pdf)].astype(np.float64) * np.log2(np.e)
    tiny, flushed = 2.0 ** -1022, 0
    v = None
    for t in range(n):
        x = a if t == 0 else T.T @ v
        K = 0 if t == 0 or v.max() == 0 else int(np.floor(np.log2(v.max())))
        with np.errstate(under="ignore"):
            nv = np.ldexp(x * np.exp2(e2[t] - e2[t].max()), -K)
        lost = (nv < tiny) & (x > 0)
        flushed += int(lost.sum())
        nv[nv < tiny] = 0.0
        v = nv
    return float(v @ om), flushed


# ---- the float64 reference, once per case
def reference(oracle, graphs_mod, gs, V, lens, key=None):
    """(gamma [B, N, P] float64, ttl [B]) of a batch by the C oracle, oc.batch_shared per distinct graph, every graph on the P pdfs of V
    (a batch's graphs share P; a graph with fewer pdfs of its own leaves the others without a state); memoised under `key`.  The
    oracle's gamma of an utterance without a path (ttl = -inf) is 0 / 0: not a number."""
    def make():
        o, oc = oracle
        lens_ = np.full(V.shape[0], V.shape[1], dtype=np.int32) if lens is None else np.asarray(lens, dtype=np.int32)
        g_ref, t_ref = np.zeros(V.shape, dtype=np.float64), np.zeros(V.shape[0])
        for g in {id(g): g for g in gs}.values():
            idx = np.array([b for b, x in enumerate(gs) if x is g])
            gr, tr = oc.batch_shared(graphs_mod.to_oracle(o, g), g.state2pdf, V.shape[2], V[idx], lens_[idx], dtype=np.float64, nthreads=4)
            g_ref[idx], t_ref[idx] = gr, tr
        g_ref.setflags(write=False)
        t_ref.setflags(write=False)
        return g_ref, t_ref
    return make() if key is None else _memo(("wref", key), make)
