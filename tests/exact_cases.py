"""Graphs, shapes, emissions and environments of the exact tier's instance tests: tests/test_gpu_exact_instances.py runs them on
the GPU, tests/test_exact_inputs.py checks from the float64 oracle alone that they are what those tests take them for.

The exact tier: the wide-exponent pair kernels (mm_kernel_wpair.hip: mm_fbw_kernel, as teams mm_fbws_kernel) and the float64 pair
kernels (mm_kernel_dpair.hip: mm_fbd_kernel, as teams mm_fbds_kernel).  NJ is the number of 64-lane passes of the service wave over
the pdfs (mm_pair_nj of mm_internal.h: 2 up to P + 1 = 128, 4 up to 250, 8 up to 506; teams of 8 run 5 passes up to 314), H the
number of workgroups of a team."""
import dataclasses
import os

import numpy as np

import graphs
from test_gpu_exact import peaky
from test_gpu_pair_pdfsums import SHAPES, _holes

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the switches (all under MM_DEBUG=1, read when the batch is created)
ENV_WIDE = {"MM_DEBUG": "1", "MM_EXACT_FIRST": "1", "MM_NO_FALLBACK": "1"}  # the wide kernels alone (where the batch fits them)
ENV_F64 = dict(ENV_WIDE, MM_NO_WPAIR="1")  # the float64 kernels alone
ENV_BEHIND = {"MM_DEBUG": "1", "MM_EXACT_FIRST": "0", "MM_NO_FALLBACK": "1"}  # the float64 kernels behind the float32 kernels
# the float32 kernels alone: marks are counted, nothing runs behind them (MM_EXACT_FIRST=0: nor in front of them after a call with marks)
ENV_F32 = {"MM_DEBUG": "1", "MM_NO_REDO": "1", "MM_EXACT_FIRST": "0"}
TIER_ENV = {"wide": ENV_WIDE, "f64": ENV_F64}


def with_empty_pdf(g, name):
    """g with one more pdf than its states use (an odd P, as test_gpu_pair_pdfsums._holes gets its own)."""
    return dataclasses.replace(g, name=name, P=g.P + 1)


def boundary_graph(wl, P1):
    """A 600-state graph with P + 1 = P1 (lfmmi_denominator takes an even P: an odd one gets a pdf without a state)."""
    P = P1 - 1
    if P % 2 == 0:
        return wl.lfmmi_denominator(600, P, seed=5)
    return with_empty_pdf(wl.lfmmi_denominator(600, P - 1, seed=5), f"lfmmi_600_{P}")


def wsj_den(wl):
    return wl.load_npz_graph(os.path.join(HERE, "golden", "den_fsm_wsj.npz"))


GRAPHS = {
    # group A: one workgroup per utterance (pair), at the shapes of test_gpu_pair_pdfsums
    "nj2": lambda wl: wl.lfmmi_denominator(600, 40, seed=5),
    "nj4": lambda wl: wl.lfmmi_denominator(600, 200, seed=5),
    "nj8": lambda wl: wl.lfmmi_denominator(600, 400, seed=5),
    "loop": lambda wl: wl.lfmmi_denominator(600, 10, seed=5),  # 60 states per pdf
    "holes": _holes,  # 41 pdfs: the last without a state, pdf 3 with one
    "small": lambda wl: wl.random_fsm(100, 12, 20.0, seed=5),  # a vector shorter than one pass of the scans (MM_KERNEL=pair)
    # the pdf-count boundaries of mm_pair_nj on a 600-state graph
    **{f"p1_{P1}": (lambda wl, P1=P1: boundary_graph(wl, P1)) for P1 in (128, 129, 250, 251, 506, 507)},
}
EXTRA_ENV = {"small": {"MM_KERNEL": "pair"}}

# group A: graph -> {tier: NJ}; a tier that is absent does not take the graph (mm_wpair_fits: up to 250 pdfs)
GROUP_A = {
    "nj2": {"wide": 2, "f64": 2},
    "nj4": {"wide": 4, "f64": 4},
    "nj8": {"f64": 8},
    "loop": {"wide": 2, "f64": 2},
    "holes": {"wide": 2, "f64": 2},
    "small": {"wide": 2, "f64": 2},
}
BOUNDARIES = {128: {"wide": 2, "f64": 2}, 129: {"wide": 4, "f64": 4}, 250: {"wide": 4, "f64": 4}, 251: {"f64": 8}, 506: {"f64": 8}}
BOUNDARY_SHAPE = (3, 6, (6, 4, 1))
# the float32 kernels alone need plain inputs that they leave unmarked (test_gpu_pair_pdfsums.py on why short utterances on these
# graphs are often marked): the first seed offset k of case_seed() whose batch of BOUNDARY_SHAPE has no mark.  Of k = 0 .. 39 that
# held for 24 (P + 1 = 128), 23 (129), 12 (250) and all 40 (251, 506: three pdfs in four without a state).
F32_SEED = {128: 0, 129: 1, 250: 1, 251: 0, 506: 0}
# group B: utterance 1 is fixed (plain, 6 frames), utterance 0 is one of six partners
PARTNER_GRAPHS = {2: "nj2", 4: "nj4"}
PARTNERS = ["plain", "sharp", "minus_inf_forward", "minus_inf_backward", "one_frame", "no_frame"]
PARTNER_N = 6
MINUS_INF_PDF = 5
# group C: the float64 kernels behind the float32 kernels
BEHIND_GRAPHS = {2: "nj2", 4: "nj4", 8: "nj8"}
BEHIND_SHAPE = (3, 6, (6, 5, 2))
# (the same choice: of k = 0 .. 39 the plain batch of BEHIND_SHAPE had no mark for 37 (40 pdfs), 8 (200 pdfs) and 40 (400 pdfs))
BEHIND_SEED = {2: 0, 4: 4, 8: 0}
# group D: the teams.  name -> (graph, NJ, H, does the wide tier take it (mm_wpair_fits: teams of 2, up to 250 pdfs))
TEAMS = {
    "wsj_den": (2, 2, True),
    "wsj_size_200": (4, 2, True),
    "wsj_size_400": (8, 2, False),
    "lfmmi_3400_84": (2, 4, False),
    "lfmmi_3600_200": (4, 4, False),
    "lfmmi_3600_400": (8, 4, False),
    "lfmmi_5000_100": (2, 8, False),
    "lfmmi_5000_200": (4, 8, False),
    "lfmmi_6000_300": (5, 8, False),
}
TEAM_SHAPES = [(3, 6, (6, 4, 1)), (2, 3, (3, 2)), (1, 2, (2,))]
GRAPHS["wsj_den"] = wsj_den
GRAPHS["wsj_size_200"] = lambda wl: wl.lfmmi_denominator(3032, 200)  # (the WSJ denominator has 3032 states)
GRAPHS["wsj_size_400"] = lambda wl: wl.lfmmi_denominator(3032, 400)
for _S, _P in ((3400, 84), (3600, 200), (3600, 400), (5000, 100), (5000, 200), (6000, 300)):
    GRAPHS[f"lfmmi_{_S}_{_P}"] = lambda wl, S=_S, P=_P: wl.lfmmi_denominator(S, P)


def kernel_name(tier, nj, H=1):
    """What kernels() prints for phase A of the instance."""
    stem = {"wide": "mm_fbw", "f64": "mm_fbd", "f32": "mm_fbp"}[tier]
    if H == 1:
        return f"{stem}_kernel<{nj},A>"
    return f"{stem[:-1]}s_kernel<{nj},A,{H}>" if tier == "f32" else f"{stem}s_kernel<{nj},A,{H}>"


def env_of(gname, env):
    return dict(env, **EXTRA_ENV.get(gname, {}))


def plain(seed, B, N, P):
    return np.random.default_rng(seed).standard_normal((B, N, P)).astype(np.float32)


def sharp(seed, B, N, P):
    """The inputs the tier exists for: log-softmax of 25 N(0,1), 300 nats down."""
    return peaky(np.random.default_rng(seed), (B, N, P), 25.0) - np.float32(300.0)


def emissions(kind, seed, B, N, P):
    return {"plain": plain, "sharp": sharp}[kind](seed, B, N, P)


def case_seed(kind, B, N, k=0):
    return 1000 * k + 100 * B + N + (50000 if kind == "sharp" else 0)


def shape_case(g, kind, B, N, lens, k=0):
    """(V, lens) of a case of group A, the boundaries or group D."""
    return emissions(kind, case_seed(kind, B, N, k), B, N, g.P), np.asarray(lens, dtype=np.int32)


def all_cases():
    """Every (graph name, key, inputs(g) -> (V, lens)) the GPU tests compare with the oracle: what tests/test_exact_inputs.py walks."""
    out = []
    for kind in ("plain", "sharp"):
        for gname in GROUP_A:
            out += [(gname, (kind, B, N), lambda g, s=(kind, B, N, lens): shape_case(g, *s)) for B, N, lens in SHAPES]
        for gname in [f"p1_{P1}" for P1 in (*BOUNDARIES, 507)] + list(TEAMS):
            shapes = TEAM_SHAPES if gname in TEAMS else [BOUNDARY_SHAPE]
            out += [(gname, (kind, B, N), lambda g, s=(kind, B, N, lens): shape_case(g, *s)) for B, N, lens in shapes]
    for P1 in BOUNDARIES:
        B, N, lens = BOUNDARY_SHAPE
        out.append((f"p1_{P1}", ("f32", B, N), lambda g, s=("plain", B, N, lens, F32_SEED[P1]): shape_case(g, *s)))
    for gname in PARTNER_GRAPHS.values():
        out += [(gname, ("partner", p), lambda g, p=p: partner_case(g, p)[:2]) for p in PARTNERS]
    for nj, gname in BEHIND_GRAPHS.items():
        out += [(gname, ("behind", k), lambda g, k=k, nj=nj: behind_case(g, k, BEHIND_SEED[nj])[1:]) for k in range(3)]
    return out


def partner_case(g, partner, k=0):
    """(V, lens, the (frame, pdf) at -inf or None) of group B: utterance 1 the same in every case."""
    N, P = PARTNER_N, g.P
    V = plain(case_seed("plain", 2, N, k), 2, N, P)
    lens = np.array([N, N], dtype=np.int32)
    hole = None
    if partner == "sharp":
        V[0] = sharp(case_seed("sharp", 1, N, k), 1, N, P)[0]
    elif partner == "minus_inf_forward":  # (a frame of the forward agent's phase B)
        hole = (1, MINUS_INF_PDF)
    elif partner == "minus_inf_backward":  # (and one of the backward agent's)
        hole = (N - 2, MINUS_INF_PDF)
    elif partner == "one_frame":
        lens[0] = 1
    elif partner == "no_frame":
        lens[0] = 0
    if hole:
        V[0, hole[0], hole[1]] = -np.inf
    return V, lens, hole


def behind_case(g, k, seed_k):
    """(V plain, V with utterance k sharp, lens) of group C."""
    B, N, lens = BEHIND_SHAPE
    V = plain(case_seed("plain", B, N, seed_k), B, N, g.P)
    W = V.copy()
    W[k] = sharp(case_seed("sharp", 1, N, k), 1, N, g.P)[0]
    return V, W, np.asarray(lens, dtype=np.int32)


def compiled(cache, mm, wl, gname, table=GRAPHS):
    """(graph, compiled FSM): once per graph and module (`cache` is the module's)."""
    if gname not in cache:
        g = table[gname](wl)
        cache[gname] = (g, mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P)))
    return cache[gname]


_oracle_fsms = {}


def oracle_fsm(oracle, g):
    """The oracle's FSM of g, built once per graph object."""
    if id(g) not in _oracle_fsms:
        _oracle_fsms[id(g)] = (g, graphs.to_oracle(oracle[0], g))
    return _oracle_fsms[id(g)][1]


def oracle64(oracle, g, V, lens):
    return oracle[1].batch_shared(oracle_fsm(oracle, g), g.state2pdf, g.P, V, np.asarray(lens, dtype=np.int32), dtype=np.float64, nthreads=4)


def reference(cache, oracle, g, key, V, lens):
    """The float64 oracle's (gamma, ttl) of a case, computed once per module and left unchanged."""
    if key not in cache:
        g_ref, t_ref = oracle64(oracle, g, V, lens)
        g_ref.setflags(write=False)
        t_ref.setflags(write=False)
        cache[key] = (g_ref, t_ref)
    return cache[key]
