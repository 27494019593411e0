"""The item-form kernel instances and row shapes that no other test runs, on the MI355X against the float64 references the
entries already have (tests/arc_reference.py, tests/cost_reference.py, tests/sample_reference.py, the C oracle):

  A. the streamed-only instances (NI = 0) on small graphs, selected with MM_DEBUG=1 MM_NITEMS=0 at batch creation;
  B. a graph of 70 000 states -- beyond the 16-bit state indices of the resident items, the production route to NI = 0 -- alone
     and in one batch with a 40-state graph;
  C. the two sides of the 16-bit boundary (65 530 / 65 531 states) and of each entry's LDS boundary (the last graph whose state
     vectors live in the LDS and the graph of one more state), the boundary taken from kernels();
  D. rows of hundreds of arcs in both directions (the two-pass long-row branches, the lane groups beyond 16 lanes), resident
     and streamed.

Every case asserts by name, through kernels() of the batch that ran, the instance it claims to run.  No comparison here has a bar of its own: they are
arc_reference.check, cost_reference.check (GRAD_ABS_A as it stands), check_gamma, the Bernstein rule and the comparisons of
test_alpha_beta_export, test_tropical_beta_and_maxstateposteriors and test_viterbi_bit_exact.

The input builders (`case_*`) and the conditions on them (`high_state_mass`, `row_counts`) are module-level and need no GPU:
tests/test_itemform_inputs.py runs the references alone on them, tools/measure_cost_floor.py the float32 floor of the cost cases."""
import numpy as np
import pytest

import arc_reference as ar
import cost_reference as cr
import graphs
import sample_reference as sr
from test_gpu_arcposteriors import _check_batch as _arc_check
from test_gpu_arcposteriors import _scrambled_csr_run
from test_gpu_expectedcost import _check_batch as _cost_check
from test_gpu_expectedcost import case_distinct, case_random40
from test_gpu_parity import _with_env, check_gamma
from test_gpu_samplepaths import _exact_tiny_run, _size_check

pytestmark = pytest.mark.gpu

STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
ITEM = {"MM_DEBUG": "1", "MM_KERNEL": "item"}  # pdfposteriors on the item kernel whatever family the graph would get
HIGH = 65536  # the first state index that does not fit 16 bits

# the LDS boundaries predicted from lds_plan / cost_lds_plan / mm_launch_arcs at P = 40: the last S of random_fsm(S, 40, ...)
# whose vectors live in the LDS.  The engine's own answer (kernels()) decides; a mismatch is printed, not failed.
PREDICTED_LDS_BOUNDARY = {"log": 10186, "sample": 10186, "arcs": 10178, "cost": 5062}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# ---- the inputs: (graphs, V, cost, lens, utterances checked against the reference), as tests/test_gpu_expectedcost.py
def case_lfmmi600(wl):
    g = wl.lfmmi_denominator(600, 40)
    N = 60
    V = np.random.default_rng(21).standard_normal((3, N, g.P)).astype(np.float32)
    cost = np.random.default_rng(22).standard_normal((3, N, g.P)).astype(np.float32)
    return [g] * 3, V, cost, np.array([60, 41, 17], dtype=np.int32), None


def case_random_big(wl, S=70000):
    """random_fsm(S, 40, 3.0, seed=3), two utterances of 24 frames (lengths 24 and 13): S = 70 000 is the graph of group B,
    65 530 / 65 531 the two sides of the 16-bit boundary, ~10 000 / ~5 000 the LDS boundaries."""
    g = wl.random_fsm(S, 40, 3.0, seed=3)
    N = 24
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    cost = np.random.default_rng(14).standard_normal((2, N, g.P)).astype(np.float32)
    return [g, g], V, cost, np.array([24, 13], dtype=np.int32), None


def case_mixed(wl, big_first):
    """The 70 000-state graph and a 40-state one (both P = 40) in one batch, in either order."""
    big, small = wl.random_fsm(70000, 40, 3.0, seed=3), wl.random_fsm(40, 40, 3.0, seed=1)
    N = 24
    V = np.random.default_rng(4).standard_normal((2, N, 40)).astype(np.float32)
    cost = np.random.default_rng(14).standard_normal((2, N, 40)).astype(np.float32)
    return ([big, small] if big_first else [small, big]), V, cost, np.array([24, 13], dtype=np.int32), None


def case_wide(wl, name):
    """Rows of hundreds of arcs: `wide` one state of in-degree 650 and one of out-degree 642; `ergodic300` every row 300 wide
    (P = 300); `lexicon` hubs of degree ~140 (lane groups of 17 to 64 lanes)."""
    g, N, lens = {"wide": lambda: (wl.wide_row_fsm(seed=1), 30, (30, 19)),
                  "ergodic300": lambda: (wl.dense_ergodic(300), 20, (20, 13)),
                  "lexicon": lambda: (wl.lexicon_fsm(3000, 50, seed=2), 30, (30, 19))}[name]()
    V = np.random.default_rng(31).standard_normal((2, N, g.P)).astype(np.float32)
    cost = np.random.default_rng(32).standard_normal((2, N, g.P)).astype(np.float32)
    return [g, g], V, cost, np.array(lens, dtype=np.int32), None


# ---- the conditions on the inputs, from the float64 reference alone
def high_state_mass(oracle, g, V, L, N, first=HIGH):
    """Per frame 0 .. L-1: the posterior mass on the real states numbered `first` or higher (float64 oracle)."""
    o, oc = oracle
    _, z, A, Bm = oc.single(graphs.to_oracle(o, g), g.state2pdf, g.P, ar.expand_log(V, L, N), dtype=np.float64, want_ab=True)
    with np.errstate(invalid="ignore"):
        post = np.exp(A[first:g.S, :L] + Bm[first:g.S, :L] - z)
    return np.where(np.isfinite(post), post, 0.0).sum(axis=0)


def assert_high_states_carry_mass(oracle, case):
    """At least 1e-2 of the mass on states >= 65 536 in at least half of the frames of each utterance: a state index cut to 16
    bits would otherwise be invisible."""
    gs, V, _, lens, _ = case
    for b, g in enumerate(gs):
        if g.S <= HIGH:
            continue
        m = high_state_mass(oracle, g, V[b].astype(np.float64), int(lens[b]), V.shape[1])
        print(f"utterance {b}: mass on states >= {HIGH} per frame: min {m.min():.3g}, max {m.max():.3g}, "
              f"{int((m >= 1e-2).sum())} of {m.size} frames at 1e-2 or more")
        assert 2 * int((m >= 1e-2).sum()) >= m.size, (b, m)


def row_counts(mm, wl, oracle, g, V, L, N):
    """The widest-in and widest-out real state of g (phony final state excluded) with their degrees, and the expected count the
    float64 reference puts through the arcs into the one and out of the other; the reference's counts and initial counts."""
    o, oc = oracle
    f = wl.to_fsm(mm, g)
    c, init, z = ar.reference(o, oc, g, f, V, L, N)
    i, j, _ = ar.fsm_entries(f)
    real = (i < g.S) & (j < g.S)
    din, dout = np.bincount(j[real], minlength=g.S), np.bincount(i[real], minlength=g.S)
    s_in, s_out = int(np.argmax(din)), int(np.argmax(dout))
    # ... and through all the rows of more than 64 arcs (lane groups beyond a 16-lane row) of either direction
    wide_in, wide_out = real & (din[np.minimum(j, g.S - 1)] > 64), real & (dout[np.minimum(i, g.S - 1)] > 64)
    return {"in": (s_in, int(din[s_in]), float(c[real & (j == s_in)].sum())),
            "out": (s_out, int(dout[s_out]), float(c[real & (i == s_out)].sum())),
            "in64": (int((din > 64).sum()), float(c[wide_in].sum())), "out64": (int((dout > 64).sum()), float(c[wide_out].sum())),
            "counts": c, "init": init, "logz": z}


def assert_wide_rows_carry_counts(name, rc, b):
    """`wide`: the widest-in and the widest-out state each carry an expected count of at least 0.5.  For the other two graphs
    that condition is replaced by a weaker one, the rows of more than 64 arcs TOGETHER carry at least 0.5 in each direction:
    the four hubs of `lexicon` share the traffic (its short utterance puts 0.16 through the widest-in hub), and every row of
    `ergodic300` is 300 wide, so all N transitions pass one while a single state sees N / 300.  A long-row branch that drops arcs would otherwise lose nothing the bars can see."""
    print(f"{name}, utterance {b}: widest-in state {rc['in'][0]} ({rc['in'][1]} arcs) carries {rc['in'][2]:.3g}, widest-out state "
          f"{rc['out'][0]} ({rc['out'][1]} arcs) carries {rc['out'][2]:.3g}; the {rc['in64'][0]} / {rc['out64'][0]} rows of more than "
          f"64 arcs carry {rc['in64'][1]:.3g} in / {rc['out64'][1]:.3g} out")
    if name == "wide":
        assert rc["in"][2] >= 0.5 and rc["out"][2] >= 0.5, (rc["in"], rc["out"])
    assert rc["in"][1] > 64 and rc["out"][1] > 64 and rc["in64"][1] >= 0.5 and rc["out64"][1] >= 0.5, (rc["in64"], rc["out64"])


# ---- helpers
def _make_batch(mm, wl, gs, semiring="log"):
    cache = {}
    for g in gs:
        if id(g) not in cache:
            cache[id(g)] = mm.compile(wl.to_fsm(mm, g, semiring), mm.statemap(g.state2pdf, g.P))
    return mm.batch(*[cache[id(g)] for g in gs])


def _arcs_are(k, NI, where):
    mem = "state vectors in LDS" if where == "lds" else "state vectors in global memory"
    assert f"mm_log_kernel<MODE_FB,{NI},1>" in k and f"mm_arc_kernel<{NI}>" in k and mem in k, k


def _sample_is(k, NI, where):
    assert f"mm_log_kernel<MODE_FB,{NI},1>" in k and f"mm_sample_kernel<{where}>" in k, k


def _cost_is(k, NI, where):
    assert f"mm_cost_fwd_kernel<{NI},{where}>" in k and f"mm_cost_bwd_kernel<{NI},{where}>" in k, k


def _item_fb_name(NI, where):
    return (f"mm_log_kernel<MODE_FB,0,0,{where}>" if NI == 0 else f"mm_log_kernel<MODE_FB,8,1,{where}> (forward) + mm_log_kernel<MODE_FB,8,2,{where}>")


def _pdf_check(mm, wl, oracle, case, env):
    """pdfposteriors of a batch created under env: check_gamma and ttl, each utterance against its own float64 reference.
    Returns kernels("log") of the batch that ran."""
    o, oc = oracle
    gs, V, _, lens, _ = case

    def run():
        bf = _make_batch(mm, wl, gs)
        return bf.pdfposteriors(V, lens) + (bf.kernels("log"),)

    gam, ttl, k = _with_env(env, run)
    for b, g in enumerate(gs):
        g_ref, t_ref = oc.batch_shared(graphs.to_oracle(o, g), g.state2pdf, g.P, V[b : b + 1], lens[b : b + 1], dtype=np.float64)
        worst = check_gamma(gam[b : b + 1], g_ref, lens[b : b + 1])
        print(f"utterance {b}: len {int(lens[b])}, worst log-posterior error / bar {worst:.3g}")
        assert np.allclose(ttl[b], t_ref[0], rtol=1e-5, atol=1e-4), (b, ttl[b], t_ref[0])
    return k


def _three_entries(mm, wl, oracle, case, env, NI, where, marginals=True):
    """arcposteriors, expectedcost (with gamma) and samplepaths of the case under env, each against its reference, each on the
    instance <NI> with its vectors `where` ("lds" / "global") by the kernels() of the batch that ran."""
    gs, V, cost, lens, idx = case
    _arcs_are(_with_env(env, lambda: _arc_check(mm, wl, oracle, gs, V, lens, check_idx=idx, want_batch=True))[2].kernels("arcs"), NI, where)
    _cost_is(_with_env(env, lambda: _cost_check(mm, wl, oracle, case))[0].kernels("cost"), NI, where)
    _sample_is(_with_env(env, lambda: _size_check(mm, wl, oracle, gs, V, lens, marginals=marginals))[0].kernels("sample"), NI, where)


def _export_check(mm, wl, oracle, g, V, lens, env):
    """alpha / beta export of a log batch against the oracle's want_ab matrices: the comparison of test_alpha_beta_export.
    Returns kernels("export") of the batch that ran."""
    o, oc = oracle
    N, S1 = V.shape[1], g.S + 1

    def run():
        bf = _make_batch(mm, wl, [g] * len(lens))
        return bf.alpharecursion(V, lens), bf.betarecursion(V, lens), bf.kernels("export")

    A, Bm, k = _with_env(env, run)
    assert A.shape == (len(lens) * S1, N + 1) and Bm.shape == A.shape
    of = graphs.to_oracle(o, g)
    for b, L in enumerate(lens):
        _, _, Ar, Br = oc.single(of, g.state2pdf, g.P, ar.expand_log(V[b].astype(np.float64), int(L), N), dtype=np.float64, want_ab=True)
        for got, ref in ((A[b * S1:(b + 1) * S1], Ar), (Bm[b * S1:(b + 1) * S1], Br)):
            assert np.array_equal(np.isneginf(got), np.isneginf(ref))
            m = np.isfinite(ref)
            assert np.allclose(got[m], ref[m], rtol=1e-5, atol=1e-4)
    return k


def _viterbi_check(mm, wl, oracle, g, V, lens, env):
    """Item-form Viterbi (the int32 back-pointers asked for), bit exact against the float32 C oracle: test_viterbi_bit_exact.
    Returns the paths and kernels("tropical") of the batch that ran."""
    o, oc = oracle
    S1 = g.S + 1

    def run():
        bf = _make_batch(mm, wl, [g] * len(lens), "tropical")
        return bf.viterbi(V, np.asarray(lens, dtype=np.int32), return_backpointers=True) + (bf.kernels("tropical"),)

    path, score, bp, k = _with_env(env, run)
    of = graphs.to_oracle(o, g, "tropical", np.float32)
    for b, L in enumerate(lens):
        pr, sc, bpr = oc.viterbi(of, g.state2pdf, g.P, V[b], int(L), dtype=np.float32)
        assert np.array_equal(path[b], pr), (b, path[b], pr)
        assert score[b] == sc
        assert np.array_equal(bp[:, b * S1:(b + 1) * S1], bpr)
    return path, k


def _maxstate_check(mm, wl, oracle, g, V, lens, env, with_reference):
    """Tropical beta and the max-marginals: the comparisons of test_tropical_beta_and_maxstateposteriors (the NumPy oracle's
    generic recursions where with_reference; always mu <= 0, every frame's maximum 0, mu = 0 along the Viterbi path).  Returns
    kernels("tropical") and kernels("export") of the batch that ran."""
    o, _ = oracle
    K, S1, N = o.TROPICAL, g.S + 1, V.shape[1]

    def run():
        bf = _make_batch(mm, wl, [g] * len(lens), "tropical")
        path, score = bf.viterbi(V, np.asarray(lens, dtype=np.int32))
        return (bf.alpharecursion(V, lens), bf.betarecursion(V, lens), bf.maxstateposteriors(V, lens), path, score,
                (bf.kernels("tropical"), bf.kernels("export")))

    A, Bm, mu, paths, scores, k = _with_env(env, run)
    if with_reference:
        of = graphs.to_oracle(o, g, "tropical")
        Co = o.statemap(g.state2pdf, g.P, K)
    for b, L in enumerate(lens):
        if with_reference:
            lhs = o.spmm_csc(Co, o.expand(V[b].T.astype(np.float64), int(L), K), K)
            Ar = o.alpharecursion(of.alpha_hat, of.T_hat.transpose(), lhs, K)
            Br = o.betarecursion(of.T_hat, lhs, K)
            for got, ref in ((A[b * S1:(b + 1) * S1], Ar), (Bm[b * S1:(b + 1) * S1], Br)):
                assert np.array_equal(np.isneginf(got), np.isneginf(ref))
                m = np.isfinite(ref)
                assert np.allclose(got[m], ref[m], rtol=1e-5, atol=1e-4)
        m_b = mu[b * S1:(b + 1) * S1]
        assert np.isfinite(scores[b])
        assert (m_b <= 1e-4).all()
        assert np.allclose(m_b.max(axis=0), 0.0, atol=1e-4)  # some best path passes every frame
        for n, s in enumerate(paths[b, : int(L)]):  # ... and the Viterbi path is one of them
            assert abs(m_b[s, n]) <= 1e-4, (g.name, b, n, s, m_b[s, n])
    return k


# ---- A. the streamed-only instances on small graphs
STREAMED_CASES = {"rand40": case_random40, "distinct": case_distinct, "lfmmi600": case_lfmmi600}


@pytest.mark.parametrize("name", list(STREAMED_CASES))
def test_streamed_arcposteriors(mm, wl, oracle, torch, name):
    gs, V, _, lens, idx = STREAMED_CASES[name](wl)
    c, ttl, bf = _with_env(STREAMED, lambda: _arc_check(mm, wl, oracle, gs, V, lens, check_idx=idx, want_batch=True))
    _arcs_are(bf.kernels("arcs"), 0, "global")
    if name == "rand40":  # length 0 and the utterance without a path
        assert np.isneginf(ttl[3]) and np.isneginf(ttl[4]) and (c[3] == 0).all() and (c[4] == 0).all()


def test_streamed_arcposteriors_scrambled_csr(mm, wl, oracle, torch):
    _arcs_are(_with_env(STREAMED, lambda: _scrambled_csr_run(mm, wl, oracle, torch)), 0, "global")


@pytest.mark.parametrize("name", list(STREAMED_CASES))
def test_streamed_expectedcost(mm, wl, oracle, torch, name):
    case = STREAMED_CASES[name](wl)
    bf, risk, grad, ttl, gamma = _with_env(STREAMED, lambda: _cost_check(mm, wl, oracle, case))
    _cost_is(bf.kernels("cost"), 0, "global")
    if name == "rand40":
        for b in (3, 4):
            assert np.isneginf(ttl[b]) and risk[b] == 0 and (grad[b] == 0).all() and (gamma[b] == 0).all()


@pytest.mark.parametrize("case", [0, 3])
def test_streamed_samplepaths_exact_distribution(mm, wl, torch, case):
    bf = _with_env(STREAMED, lambda: _exact_tiny_run(mm, wl, case))  # (K_EXACT samples, Bernstein rule, logprob)
    _sample_is(bf.kernels("sample"), 0, "global")


def test_streamed_samplepaths_marginals(mm, wl, oracle, torch):
    gs, V, _, lens, _ = case_lfmmi600(wl)
    bf, _, _ = _with_env(STREAMED, lambda: _size_check(mm, wl, oracle, gs, V, lens))
    _sample_is(bf.kernels("sample"), 0, "global")


def test_streamed_alpha_beta_export(mm, wl, oracle, torch):
    g = wl.random_fsm(25, 5, 3.0, seed=7)
    V = np.random.default_rng(3).standard_normal((2, 14, g.P)).astype(np.float32)
    k = _export_check(mm, wl, oracle, g, V, [14, 9], STREAMED)
    assert "mm_log_kernel<MODE_ALPHA,0,lds>" in k and "mm_log_kernel<MODE_BETA,0,lds>" in k, k


def test_streamed_tropical_beta_and_maxstateposteriors(mm, wl, oracle, torch):
    g = wl.random_fsm(30, 5, 3.0, seed=9)
    V = np.random.default_rng(3).standard_normal((2, 12, g.P)).astype(np.float32)
    kt, kx = _maxstate_check(mm, wl, oracle, g, V, [12, 7], STREAMED, with_reference=True)
    assert "mm_tropical_kernel<0,lds>" in kt and "mm_log_kernel<MODE_BETA,0,lds,TROP>" in kx, (kt, kx)


def test_streamed_viterbi_bit_exact(mm, wl, oracle, torch):
    g = wl.random_fsm(50, 6, 3.0, seed=4)
    V = (np.round(np.random.default_rng(5).standard_normal((3, 37, g.P)) * 2) / 2).astype(np.float32)  # quantised: exact ties
    _, k = _viterbi_check(mm, wl, oracle, g, V, [37, 20, 1], STREAMED)
    assert "mm_tropical_kernel<0,lds>" in k, k


# ---- B. beyond 16-bit state indices
def test_beyond_16_bit_indices_new_entries(mm, wl, oracle, torch):
    case = case_random_big(wl)
    assert_high_states_carry_mass(oracle, case)
    _three_entries(mm, wl, oracle, case, {}, 0, "global")


def test_beyond_16_bit_indices_pdfposteriors_and_export(mm, wl, oracle, torch):
    case = case_random_big(wl)
    gs, V, _, lens, _ = case
    k = _pdf_check(mm, wl, oracle, case, {})
    assert k == _item_fb_name(0, "global") + " (forward and backward in one launch, every item streamed)", k
    k = _export_check(mm, wl, oracle, gs[0], V, lens, {})
    assert "alpha: mm_log_kernel<MODE_ALPHA,0,global>; beta: mm_log_kernel<MODE_BETA,0,global>" == k, k


def test_beyond_16_bit_indices_tropical(mm, wl, oracle, torch):
    gs, V, _, lens, _ = case_random_big(wl)
    path, k = _viterbi_check(mm, wl, oracle, gs[0], V, lens, {})
    assert "mm_tropical_kernel<0,global>" in k, k
    assert (path >= HIGH).any()  # (the best paths themselves pass states beyond 16 bits)
    kt, kx = _maxstate_check(mm, wl, oracle, gs[0], V, lens, {}, with_reference=False)
    assert "mm_tropical_kernel<0,global>" in kt and "mm_log_kernel<MODE_BETA,0,global,TROP>" in kx, (kt, kx)


@pytest.mark.parametrize("big_first", [True, False])
def test_mixed_batch_of_a_graph_beyond_16_bits_and_a_small_one(mm, wl, oracle, torch, big_first):
    case = case_mixed(wl, big_first)
    assert_high_states_carry_mass(oracle, case)
    _three_entries(mm, wl, oracle, case, {}, 0, "global")
    k = _pdf_check(mm, wl, oracle, case, {})
    assert _item_fb_name(0, "global") in k, k


# ---- C. the two sides of each boundary
@pytest.mark.parametrize("S,NI", [(65530, 8), (65531, 0)])
def test_16_bit_boundary(mm, wl, oracle, torch, S, NI):
    case = case_random_big(wl, S)
    _three_entries(mm, wl, oracle, case, {}, NI, "global", marginals=False)
    k = _pdf_check(mm, wl, oracle, case, {})
    assert k.startswith(_item_fb_name(NI, "global")), k


LDS_NAMES = {"log": ("mm_log_kernel<MODE_FB,8,1,lds>", "mm_log_kernel<MODE_FB,8,1,global>"),
             "sample": ("mm_sample_kernel<lds>", "mm_sample_kernel<global>"),
             "arcs": ("state vectors in LDS", "state vectors in global memory"),
             "cost": ("mm_cost_fwd_kernel<8,lds>", "mm_cost_fwd_kernel<8,global>")}


def _says_lds(entry, k):
    lds, glb = LDS_NAMES[entry]
    assert (lds in k) != (glb in k), k
    return lds in k


def lds_boundary(mm, wl, entry):
    """The last S of random_fsm(S, 40, 3.0, seed=3) whose vectors the entry keeps in the LDS, from kernels() of a batch of that
    graph: the predicted value where the engine agrees with it, else by bisection.  (A search only: test_lds_boundary asserts the
    two sides on the batches that run.)"""
    def in_lds(S):
        g = wl.random_fsm(S, 40, 3.0, seed=3)
        return _says_lds(entry, _with_env(ITEM, lambda: _make_batch(mm, wl, [g, g]).kernels(entry)))

    pred = PREDICTED_LDS_BOUNDARY[entry]
    if in_lds(pred) and not in_lds(pred + 1):
        print(f"{entry}: the vectors leave the LDS at S = {pred} -> {pred + 1}, as predicted")
        return pred
    lo, hi = 1000, 20000
    assert in_lds(lo) and not in_lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_lds(mid) else (lo, mid)
    print(f"{entry}: the vectors leave the LDS at S = {lo} -> {lo + 1} (predicted: {pred} -> {pred + 1})")
    return lo


@pytest.mark.parametrize("entry", ["log", "arcs", "sample", "cost"])
def test_lds_boundary(mm, wl, oracle, torch, entry):
    S = lds_boundary(mm, wl, entry)
    for s, in_lds in ((S, True), (S + 1, False)):
        case = case_random_big(wl, s)
        gs, V, _, lens, _ = case
        if entry == "log":
            k = _pdf_check(mm, wl, oracle, case, ITEM)
        elif entry == "arcs":
            k = _with_env(ITEM, lambda: _arc_check(mm, wl, oracle, gs, V, lens, want_batch=True))[2].kernels("arcs")
        elif entry == "sample":
            k = _with_env(ITEM, lambda: _size_check(mm, wl, oracle, gs, V, lens, marginals=False))[0].kernels("sample")
        else:
            k = _with_env(ITEM, lambda: _cost_check(mm, wl, oracle, case))[0].kernels("cost")
        assert _says_lds(entry, k) == in_lds, (s, k)  # adjacency, on the batch that ran: lds at S, global at S + 1


# ---- D. wide rows in both directions
@pytest.mark.parametrize("env", [{}, STREAMED], ids=["resident", "streamed"])
@pytest.mark.parametrize("name", ["wide", "ergodic300", "lexicon"])
def test_wide_rows(mm, wl, oracle, torch, name, env):
    case = case_wide(wl, name)
    gs, V, _, lens, _ = case
    for b in range(len(gs)):
        assert_wide_rows_carry_counts(name, row_counts(mm, wl, oracle, gs[b], V[b].astype(np.float64), int(lens[b]), V.shape[1]), b)
    _three_entries(mm, wl, oracle, case, env, 0 if env else 8, "global" if env else "lds")
