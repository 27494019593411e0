"""mm_viterbi_f32 on the row-lane kernels (mm_vit_kernel<N4,N2,NJ> + mm_vit_backtrace_kernel) at every instance, every
lane-group width of a row, the limits of the form and a back-trace ring that wraps -- on graphs whose weights sit on a grid, so that
the tie rule of the back-pointers decides the paths (tests/viterbi_cases.py; tests/test_viterbi_inputs.py shows without a GPU that a
wrong rule, a forgotten lane, a lost pdf or a wrong seam of the ring would change them).

Every comparison is bit exact against the float32 C oracle, for every utterance: the path with its -1 beyond the length, the score,
and for the same call with return_backpointers=True (the item kernel: its tie rule sees the same fixtures) the whole int32 table,
with a path and a score identical to the compact call's.  Each case asserts the instance that ran, and where it matters R, from
kernels("tropical") of its batch."""
import numpy as np
import pytest

import graphs
import viterbi_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_compiled, _oracle = {}, {}


def compiled(mm, wl, g, P=None):
    """The tropical compiled FSM of a fixture, once (P: the pdfs of the batch where its graphs differ in theirs)."""
    P = g.P if P is None else P
    key = (id(g), P)
    if key not in _compiled:
        _compiled[key] = (g, mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, P)))
    return _compiled[key][1]


def oracle_of(oracle, key, gs, V, lens):
    """[(path, score, bp)] of the float32 C oracle for every utterance, once per `key`."""
    if key not in _oracle:
        o, oc = oracle
        P = V.shape[2]
        _oracle[key] = [oc.viterbi(graphs.to_oracle(o, g, "tropical", np.float32), g.state2pdf, P, V[b], int(L), dtype=np.float32)
                        for b, (g, L) in enumerate(zip(gs, lens))]
    return _oracle[key]


def batch_of(mm, wl, gs, P):
    return mm.batch(*[compiled(mm, wl, g, P) for g in gs])


def assert_exact(bf, gs, V, lens, refs, table=True):
    """The compact call and the call that asks for the table, both against the oracle.  Returns kernels("tropical")."""
    lens = np.asarray(lens, dtype=np.int32)
    path2, score2 = bf.viterbi(V, lens)
    k = bf.kernels("tropical")
    off = 0
    if table:
        path, score, bp = bf.viterbi(V, lens, return_backpointers=True)
        assert np.array_equal(path, path2) and np.array_equal(score, score2), k
    for b, (g, L) in enumerate(zip(gs, lens)):
        pr, sr, bpr = refs[b]
        assert np.array_equal(path2[b], pr), (k, b, int(L), np.flatnonzero(path2[b] != pr)[:8], path2[b], pr)
        assert (path2[b, int(L):] == -1).all()
        assert score2[b] == sr, (k, b, score2[b], sr)
        if table:
            assert np.array_equal(bp[:, off : off + g.S + 1], bpr), (k, b)
        off += g.S + 1
    return k


def run_case(mm, wl, oracle, key, gs, V, lens, table=True):
    gs = list(gs) if isinstance(gs, (list, tuple)) else [gs] * len(lens)
    bf = batch_of(mm, wl, gs, V.shape[2])
    return assert_exact(bf, gs, V, lens, oracle_of(oracle, key, gs, V, lens), table), bf


# ---- 1 and 8: the layouts, on the grid and with the continuous weights
@pytest.mark.parametrize("name", vc.GROUP1)
def test_layouts_and_ties(mm, wl, oracle, torch, name):
    g, V, lens = vc.case1(wl, name)
    k, bf = run_case(mm, wl, oracle, ("case1", name), g, V, lens)
    print(name, k)
    assert vc.instance(k) == vc.LAYOUT[name] + (2, 64), k
    path, score = bf.viterbi(V, lens)
    assert lens[5] == 0 and score[5] == -np.inf and (path[5] == -1).all()
    assert np.isfinite(score[:4]).all()


@pytest.mark.parametrize("name", ["den24", "den60"])
def test_layouts_with_continuous_weights(mm, wl, oracle, torch, name):
    """What test_viterbi_bit_exact checks for 1 x 4 + 5 x 2, for the two layouts it never ran."""
    g, V, lens = vc.case1(wl, name, quant=False)
    k, _ = run_case(mm, wl, oracle, ("case1c", name), g, V, lens)
    assert vc.instance(k) == vc.LAYOUT[name] + (2, 64), k


# ---- 2: a row of 255 arcs has a one-byte back-pointer, a row of 256 has not
@pytest.mark.parametrize("name", ["widths", "widths256"])
def test_rows_of_255_and_256_arcs(mm, wl, oracle, torch, name):
    g = vc.graph(wl, name)
    _, V, lens = vc.case1(wl, "widths")
    k, _ = run_case(mm, wl, oracle, ("w", name), g, V[:4, :40], np.minimum(lens[:4], 40))
    print(name, k)
    assert vc.instance(k) == ((1, 5, 2, 64) if name == "widths" else None), k


# ---- 3: NJ and the limits of P
@pytest.mark.parametrize("name,P", vc.P_CASES)
def test_pdf_counts(mm, wl, oracle, torch, name, P):
    g, V, lens = vc.case_pdfs(wl, name, P)
    k, _ = run_case(mm, wl, oracle, ("P", name, P), g, V, lens)
    print(name, P, k)
    want = vc.P_INSTANCE[(name, P)]
    assert vc.instance(k) == (want + (64,) if want else None), k


# ---- 4: the ring of the back-trace wraps
@pytest.mark.parametrize("name", sorted(vc.RING_R))
def test_back_trace_ring(mm, wl, oracle, torch, name):
    """den60: R = 64 and N = 131: one, two and three chunks, the first (the last one chased) of 1 or 2 frames.  chain90: the widest
    row of back-pointers leaves R = 9: up to five chunks in 40 frames."""
    g, V, lens = vc.case_ring(wl, name)
    k, _ = run_case(mm, wl, oracle, ("ring", name), g, V, lens)
    print(name, k)
    assert vc.instance(k) == vc.LAYOUT[name] + (2, vc.RING_R[name]), k


# ---- 5: the largest form and one row more
@pytest.mark.parametrize("name", ["chain90", "chain91", "chain90f", "chain91f"])
def test_size_limits(mm, wl, oracle, torch, name):
    g = vc.graph(wl, name)
    assert g.S + 1 == {"chain90": 5760, "chain91": 5761, "chain90f": 5697, "chain91f": 5698}[name]
    V, lens = vc.emissions(3, 24, g.P, 61), np.asarray([24, 11, 1], dtype=np.int32)
    k, _ = run_case(mm, wl, oracle, ("size", name), g, V, lens)
    print(name, k)
    inst = vc.instance(k)
    assert (inst[:3] if inst else None) == (vc.LAYOUT[name] + (2,) if vc.LAYOUT[name] else None), k
    assert inst is None or inst[3] == 9  # (a row of 5888 bytes)


# ---- 6: different graphs in one batch
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_mixed_graphs_of_one_layout(mm, wl, oracle, torch, order):
    """small15, lex15 and widths (50, 900 and 300 states: rows of 256, 1024 and 512 bytes against ONE stride), twice each."""
    names = ["small15", "lex15", "widths"] * 2
    names = names[::-1] if order == "reverse" else names
    gs = [vc.graph(wl, n) for n in names]
    V, lens = vc.emissions(6, vc.N1, 20, 71), np.asarray(vc.LENS if order == "forward" else vc.LENS[::-1], dtype=np.int32)
    k, _ = run_case(mm, wl, oracle, ("mixed", order), gs, V, lens)
    assert vc.instance(k) == (1, 5, 2, 64), k


def test_mixed_layouts_run_the_item_kernel(mm, wl, oracle, torch):
    gs = [vc.graph(wl, n) for n in ("small15", "den60", "den60", "small15")]
    V, lens = vc.emissions(4, 40, 84, 72), np.asarray([40, 31, 1, 17], dtype=np.int32)
    k, _ = run_case(mm, wl, oracle, ("mixedlayouts",), gs, V, lens)
    assert vc.instance(k) is None, k


# ---- 7: one batch over many calls, strided inputs, what is never read
def test_call_history(mm, wl, oracle, torch):
    """N = 131, 20, 131 on one batch, calls that ask for the table in between: the workspace changes its meaning (byte rows, int32
    rows) and its size; every call gives the oracle's result, which is what a fresh batch gives (test_back_trace_ring)."""
    g, V, lens = vc.case_ring(wl, "den60")
    gs = [g] * len(lens)
    bf = batch_of(mm, wl, gs, g.P)
    long_refs = oracle_of(oracle, ("ring", "den60"), gs, V, lens)
    Vs, ls = np.ascontiguousarray(V[:, :20]), np.minimum(lens, 20)
    short_refs = oracle_of(oracle, ("ring20", "den60"), gs, Vs, ls)
    Vt, Vst = torch.from_numpy(V).cuda(), torch.from_numpy(Vs).cuda()
    seen = {}
    for step, (which, table) in enumerate([("long", False), ("short", True), ("long", True), ("short", False), ("long", False), ("short", False)]):
        Vx, lx, refs = (Vt, lens, long_refs) if which == "long" else (Vst, ls, short_refs)
        out = bf.viterbi(Vx, torch.from_numpy(lx).cuda(), return_backpointers=table)
        path, score = out[0].cpu().numpy(), out[1].cpu().numpy()
        for b in range(len(lens)):
            assert np.array_equal(path[b], refs[b][0]) and score[b] == refs[b][1], (step, which, table, b)
        if table:
            bp = out[2].cpu().numpy()
            assert all(np.array_equal(bp[:, b * (g.S + 1) : (b + 1) * (g.S + 1)], refs[b][2]) for b in range(len(lens))), (step, which)
        if which in seen:
            assert np.array_equal(seen[which][0], path) and np.array_equal(seen[which][1], score)
        seen[which] = (path, score)


@pytest.mark.parametrize("name", ["den24", "chain90"])
def test_strides_and_what_is_never_read(mm, wl, oracle, torch, name):
    """V as a view of a larger buffer (batch and frame strides beyond the shape, NaN everywhere else), and the frames beyond an
    utterance's length set to NaN or +inf: the same paths, scores and table."""
    if name == "den24":
        g, V, lens = vc.case1(wl, name)
        key = ("case1", name)
    else:
        g, V, lens = vc.case_ring(wl, name)
        key = ("ring", name)
    gs = [g] * len(lens)
    refs = oracle_of(oracle, key, gs, V, lens)
    bf = batch_of(mm, wl, gs, g.P)
    B, N, P = V.shape
    lt = torch.from_numpy(lens).cuda()
    for fill in (float("nan"), float("inf")):
        big = torch.full((B, N + 3, P + 5), float("nan"), device="cuda")
        view = big[:, 1 : N + 1, 2 : P + 2]
        view.copy_(torch.from_numpy(V))
        for b, L in enumerate(lens):
            view[b, int(L):, :] = fill
        assert view.stride(2) == 1 and view.stride(1) == P + 5 and view.stride(0) == (N + 3) * (P + 5)
        for table in (False, True):
            out = bf.viterbi(view, lt, return_backpointers=table)
            path, score = out[0].cpu().numpy(), out[1].cpu().numpy()
            for b in range(B):
                assert np.array_equal(path[b], refs[b][0]) and score[b] == refs[b][1], (name, fill, table, b)
            if table:
                bp = out[2].cpu().numpy()
                assert all(np.array_equal(bp[:, b * (g.S + 1) : (b + 1) * (g.S + 1)], refs[b][2]) for b in range(B)), (name, fill)
