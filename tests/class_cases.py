"""Fixtures of the arc-class tests (tests/test_class_inputs.py without a GPU, tests/test_gpu_class_entries.py on one): class layouts
that reach the parts of the class pass (csrc/mm_kernel_arcclass.hip, class_pass), of the term loop and of the score / cost row
staging (csrc/mm_kernel_scored.hip, mm_kernel_classcost.hip) that the entries' own test files leave alone -- every width of the class
pass with class sizes chosen against its stride, the two thresholds between the widths, rank counts at the block size and at the
term loop's unroll, class counts around the block size, and classes of their own for the arcs of the 70 000-state graph that only a
32-bit row or column index reaches.  NumPy only; `wl` is the package's workloads module, `f` an FSM of wl.to_fsm.

The properties the GPU tests rest on (a dropped rank, a dropped lane share, a class pointer off by one, a clamped or zeroed last
class and a 16-bit index are each visible to the comparisons they use) are asserted from the float64 references alone in
tests/test_class_inputs.py."""
import numpy as np

import arc_reference as ar
import graphs

NT = 512                    # the block of the three entries on the base graph: 8 waves (item_plan caps them at 8)
NT_TWO_WAVES = 128          # ... under MM_DEBUG=1 MM_NWAVES=2
N = 30
LENS = (30, 19)
UNROLL = 8                  # MM_CLASS_UNROLL: the records a thread of the term loop has in flight
LANES = (1, 8, 64)
SHAPE_C = {1: 549, 8: 69, 64: 13}
SHAPE_BIG = {1: 300, 8: 600, 64: 3000}
SHAPE_SEED = 0              # the layouts the GPU tests run; tests/test_class_inputs.py asserts the conditions on them
PHONY_VARIANTS = ("own", "large", "none")
THRESHOLD_C = 40
HIGH = 65536                # the first state index that does not fit 16 bits
HIGH_C = 82


def lanes_for(M, C):
    """The lanes that sum one class, as the issue of these tests states the plan's rule (the mean class size M / C: 64 from 32, 8
    from 2, else 1) -- written down here independently of mm_batch_set_arc_classes, whose choice the kernels() text names."""
    return 64 if M >= 32 * C else 8 if M >= 2 * C else 1


def lanes_text(*lanes):
    return "; class sums on " + ", ".join(str(x) for x in sorted(set(lanes))) + " lanes"


def base_graph(wl):
    """lfmmi_denominator(600, 40, seed=5): 9 704 entries, 60 / 63 packed items -- 8 waves, 512 threads."""
    return wl.lfmmi_denominator(600, 40, seed=5)


def base_inputs(g):
    """Two utterances of 30 frames (lengths 30 and 19), V as the entries' instance tests draw it."""
    return np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32), np.array(LENS, dtype=np.int32)


def phony_entry(f):
    """The final -> final self-loop that to_fsm adds (ClassDev::cphony is its class): it fills the frames t >= len."""
    i, j, _ = ar.fsm_entries(f)
    fs = f.colptr.size - 2
    k = np.flatnonzero((i == fs) & (j == fs))
    assert k.size == 1
    return int(k[0])


def ranked_entries(f):
    """The entries that get a rank when classified, in entry order, the phony self-loop left out: both ends reach the final state,
    and are reached from an initial state (the engine keeps a few unreached states; none of them is picked here).  An entry of a
    state the item forms drop has no slot, and the plan gives it no rank."""
    i, j, w = ar.fsm_entries(f)
    S1 = f.colptr.size - 1
    ok = np.isfinite(w)

    def closure(start, src, dst):
        seen = np.zeros(S1, dtype=bool)
        seen[start] = True
        while True:
            new = seen.copy()
            new[dst[ok & seen[src]]] = True
            if (new == seen).all():
                return seen
            seen = new

    reach = closure(np.asarray(f.alpha_idx, dtype=np.int64), i, j)
    coreach = closure(np.array([S1 - 1]), j, i)
    useful = reach & coreach
    keep = useful[i] & useful[j] & ok
    keep[phony_entry(f)] = False
    return np.flatnonzero(keep)


def edge_sizes(lanes):
    """The class sizes chosen against the stride st = lanes of the class pass and its four-way unrolled loop."""
    st = lanes
    return sorted({0, 1, st - 1, st, st + 1, 4 * st - 1, 4 * st, 4 * st + 1, 5 * st, 8 * st + 3})


def shape_layout(f, lanes, seed, phony="own"):
    """(cls [nnz], C, facts) whose plan sums a class on `lanes` lanes.  Class 0 is empty (the size 0 of edge_sizes); the classes
    1, 2, ... have the other sizes of edge_sizes(lanes) in ascending order; then the large class, then a class for the phony
    self-loop (empty unless phony == "own"; "large": the phony entry is a member of the large class, "none": it has no class); for
    one lane per class every third of the remaining classes holds one entry; the last class is empty.  The members are the first
    entries of a seeded permutation of ranked_entries(f).  facts: `edge` {class: size} of the non-empty edge classes, `large`,
    `phony_class`, `M`."""
    assert lanes in LANES and phony in PHONY_VARIANTS
    C = SHAPE_C[lanes]
    pool = np.random.default_rng([seed, lanes]).permutation(ranked_entries(f))
    cls = np.full(f.nnz, -1, dtype=np.int32)
    sizes = edge_sizes(lanes)
    assert sizes[0] == 0
    at, edge = 0, {}
    for c, n in enumerate(sizes):
        cls[pool[at : at + n]] = c
        at += n
        if n:
            edge[c] = n
    large = len(sizes)
    cls[pool[at : at + SHAPE_BIG[lanes]]] = large
    at += SHAPE_BIG[lanes]
    phony_class = large + 1
    kp = phony_entry(f)
    if phony != "none":
        cls[kp] = phony_class if phony == "own" else large
    if lanes == 1:
        for c in range(phony_class + 1, C - 1):
            if c % 3 == 0:
                cls[pool[at]] = c
                at += 1
    assert at <= pool.size and phony_class < C - 1
    M = int((cls >= 0).sum())
    return cls, C, {"edge": edge, "large": large, "phony_class": phony_class, "M": M}


def threshold_layout(f, C, M):
    """M ranked entries spread evenly over the graph, in the classes pick % C (the construction of test_term_row_placement): for M on
    either side of 2 C and of 32 C."""
    pool = ranked_entries(f)
    pick = pool[np.round(np.linspace(0, pool.size - 1, M)).astype(np.int64)]
    assert np.unique(pick).size == M
    cls = np.full(f.nnz, -1, dtype=np.int32)
    cls[pick] = pick % C
    return cls


def threshold_values(C):
    return (2 * C - 1, 2 * C, 32 * C - 1, 32 * C)


def rank_layout(f, M):
    """5 classes over M ranked entries: M at the block size and at MM_CLASS_UNROLL blocks, for the term loop's two loops."""
    return threshold_layout(f, 5, M)


def rank_values(nt):
    return (nt - 1, nt, nt + 1, UNROLL * nt - 1, UNROLL * nt, UNROLL * nt + 1)


COUNT_MOVED = (11, 1203, 2404, 3605, 4806, 6007, 7208, 8409, 9610)  # ranks into ranked_entries(f): entries moved into the last classes


def count_layout(f, C):
    """Every entry (the phony self-loop too) in the class k 7919 mod C, with a fixed handful of entries moved into the classes
    C - 3 .. C - 1: C around the block size is every residue of C + 1 mod 4 (mm_scored_urow) and both sides of `tid < C` and
    `C > NT` (stage_score_ahead, stage_arow_ahead)."""
    cls = ((np.arange(f.nnz, dtype=np.int64) * 7919) % C).astype(np.int32)
    pool = ranked_entries(f)
    for q, r in enumerate(COUNT_MOVED):
        cls[pool[r % pool.size]] = C - 1 - q % 3
    return cls


def count_values(nt):
    return tuple(range(nt - 2, nt + 3))


def high_layout(g, f):
    """The 70 000-state graph: class = destination pdf + 41 [a real state >= 65 536 at either end], C = 82 -- the arcs that only a
    full 32-bit row or column index reaches have class rows of their own.  (The phony final state is no real state.)"""
    i, j, _ = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    high = ((i >= HIGH) & (i < g.S)) | ((j >= HIGH) & (j < g.S))
    return (s2p[j] + (g.P + 1) * high).astype(np.int32), 2 * (g.P + 1)


def dst_layout(g, f, C=None):
    """Destination-pdf classes (test_gpu_arcclassposteriors._dst_pdf), in C classes when a batch shares its class count."""
    _, j, _ = ar.fsm_entries(f)
    return ar._s2p_full(g)[j].astype(np.int32), (g.P + 1 if C is None else C)


# ---- what the float64 reference says of single entries: xi is the sum of its members' posteriors
def entry_posteriors(oracle, g, f, V, L, n_frames, cut=None):
    """x [nnz, N] and log Z: the posterior of every entry at every transition (float64; the terms of arcclass_reference.reference
    before they are summed by class), frames >= L: the phony self-loop alone.  cut = "row" / "col": what a term record whose row /
    column index is reduced mod 65 536 would give instead."""
    o, oc = oracle
    Vhat = ar.expand_log(V, L, n_frames)
    _, _, A, Bm = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, Vhat, dtype=np.float64, want_ab=True)
    i, j, w = ar.fsm_entries(f)
    i, j = (i % HIGH if cut == "row" else i), (j % HIGH if cut == "col" else j)
    lhs = Vhat[ar._s2p_full(g)]
    with np.errstate(invalid="ignore"):
        logZ = float(ar._lse(A[:, 0] + Bm[:, 0]))
        t = A[i, :n_frames] + w[:, None] + lhs[j, 1 : n_frames + 1] + Bm[j, 1 : n_frames + 1] - logZ
    x = np.exp(np.where(np.isnan(t), -np.inf, t))
    x[:, L:] = 0.0
    x[phony_entry(f), L:] = 1.0
    return x, logZ


def class_sums(x, cls, C):
    xi = np.zeros((C, x.shape[1]))
    m = cls >= 0
    np.add.at(xi, cls[m], x[m])
    return xi


def structural(cls, C, f, L, n_frames):
    """arcclass_reference.reference's mask of the exact values: the empty classes and the frames >= L."""
    exact = np.zeros((C, n_frames), dtype=bool)
    exact[np.bincount(cls[cls >= 0], minlength=C) == 0] = True
    exact[:, L:] = True
    return exact
