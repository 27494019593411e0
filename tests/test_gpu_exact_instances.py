"""GPU tests of every instance of the exact tier at the smallest shapes at which it can go wrong: the wide-exponent pair kernels
(mm_kernel_wpair.hip: mm_fbw_kernel<NJ>, as teams mm_fbws_kernel<NJ, ., H>) and the float64 pair kernels (mm_kernel_dpair.hip:
mm_fbd_kernel<NJ>, as teams mm_fbds_kernel<NJ, ., H>), against the float64 oracle at the project's bars (check_gamma of
test_gpu_parity.py; ttl within rtol 1e-5 and atol 1e-4 on plain, 1e-3 on sharp emissions, as in test_gpu_exact.py).  Inputs:
tests/exact_cases.py; what they are taken for is checked from the oracle alone in tests/test_exact_inputs.py.

Every test first asserts the instance by name from kernels() of the batch that runs (mm_launch_dpairs / mm_launch_wpairs pick the
instance from the same NJ and H that kernels() prints), and runs with MM_NO_FALLBACK: what the tier computed is what is compared.

  A  the one-workgroup instances at the shapes of test_gpu_pair_pdfsums.py: B = 1, 2, 3 and N = 2 .. 9 (one to five phase-B steps
     per agent, the partner ring wrapping, lengths 0 and 1), on graphs of 40, 200 and 400 pdfs (NJ = 2, 4, 8), of 60 states per pdf,
     with a pdf without a state and one of a single state, and of 100 states; then the pdf counts on either side of every step
     of mm_pair_nj (P + 1 = 128 | 129, 250 | 251, 506 | 507), the float32 pair kernels alone at the same counts included;
  B  the partner in a wide pair: utterance 1 against the oracle, and to the bit on the float64 kernels, whatever utterance 0 holds
     (plain, sharp, an emission of -inf in either agent's phase B, one frame, no frame);
  C  the float64 kernels behind the float32 kernels: one utterance of three is sharp, and the others keep, bit for bit, what the
     float32 kernels alone gave them;
  D  the teams of 2, 4 and 8 workgroups with every NJ their launch tables build: mm_fbws<2,.,2>, <4,.,2>; mm_fbds<2|4|8,.,2>,
     <2|4|8,.,4>, <2|4|5,.,8>.  Every instance of the two launch tables is reached by a graph the planner takes; none is left out.

Only utterances of fewer than 2 frames are left out of a comparison (they have no path: gamma = 0 and ttl = -inf exactly), and every
case has an utterance of the full N frames."""
import numpy as np
import pytest

import exact_cases as ec
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu

_compiled, _refs = {}, {}
TTL_ATOL = {"plain": 1e-4, "sharp": 1e-3}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def batch_of(mm, cf, B, env):
    return _with_env(env, lambda: mm.batch(*([cf] * B)))


def run(bf, V, lens):
    gam, ttl = bf.pdfposteriors(V, lens)
    return np.asarray(gam.cpu() if hasattr(gam, "cpu") else gam), np.asarray(ttl.cpu() if hasattr(ttl, "cpu") else ttl)


def against_oracle(ref, gam, ttl, lens, atol, what, only=None):
    """The bars, on every utterance of 2 or more frames (`only`: on those of them); the others have no path."""
    g_ref, t_ref = ref
    ok = lens >= 2
    assert np.array_equal(np.isfinite(t_ref), ok) and lens.max() == gam.shape[1]
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()
    if only is not None:
        ok = ok & only
    worst = check_gamma(gam[ok], g_ref[ok], lens[ok])
    print(what, "worst log-posterior error / bar:", worst, "ttl error / bar:",
          float((np.abs(ttl[ok] - t_ref[ok]) / (atol + 1e-5 * np.abs(t_ref[ok]))).max()))
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=atol)


def exact_first_counts(bf, lens):
    """The whole batch ran on the exact tier, and nothing of 2 or more frames is left to the log-domain kernels (a pathless
    utterance may stay marked: Z = 0 is what a total underflow would look like)."""
    assert bf.last_exact_first()
    assert bf.last_redo_count() == len(lens)
    assert bf.last_fallback_count() <= int((lens == 1).sum())


def exact_tier_case(mm, wl, oracle, gname, tier, name, kind, shape, extra=None):
    """One case of groups A and D: the instance by name, two calls with the same bits, counts, the oracle."""
    B, N, lens = shape
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    V, lens = ec.shape_case(g, kind, B, N, lens)
    bf = batch_of(mm, cf, B, ec.env_of(gname, ec.TIER_ENV[tier]))
    assert name in bf.kernels(), bf.kernels()
    if tier == "f64":
        assert "mm_fbw" not in bf.kernels(), bf.kernels()
    gam, ttl = run(bf, V, lens)
    exact_first_counts(bf, lens)
    against_oracle(ec.reference(_refs, oracle, g, (gname, kind, B, N), V, lens), gam, ttl, lens, TTL_ATOL[kind],
                   f"{gname} {name} {kind} B={B} N={N} lens={lens.tolist()}")
    gam2, ttl2 = run(bf, V, lens)
    exact_first_counts(bf, lens)
    assert np.array_equal(gam, gam2) and np.array_equal(ttl, ttl2)
    return g, gam


# ---- group A
@pytest.mark.parametrize("kind", ["plain", "sharp"])
@pytest.mark.parametrize("B,N,lens", ec.SHAPES)
@pytest.mark.parametrize("gname,tier", [(gname, tier) for gname, tiers in ec.GROUP_A.items() for tier in tiers])
def test_one_workgroup_instances(mm, wl, oracle, torch, gname, tier, B, N, lens, kind):
    g, gam = exact_tier_case(mm, wl, oracle, gname, tier, ec.kernel_name(tier, ec.GROUP_A[gname][tier]), kind, (B, N, lens))
    if gname == "holes":  # the pdf without a state
        assert (gam[..., g.P - 1] == 0).all()


def test_400_pdfs_do_not_fit_the_wide_kernels(mm, wl, torch):
    """mm_wpair_fits is false beyond 250 pdfs: exact-first without MM_NO_WPAIR names no wide kernel on the 600/400 graph."""
    g, cf = ec.compiled(_compiled, mm, wl, "nj8")
    k = batch_of(mm, cf, 3, ec.ENV_WIDE).kernels()
    assert "mm_fbw" not in k and ec.kernel_name("f64", 8) in k, k


@pytest.mark.parametrize("kind", ["plain", "sharp"])
@pytest.mark.parametrize("P1,tier", [(P1, tier) for P1, tiers in ec.BOUNDARIES.items() for tier in ("wide", "f64")])
def test_pdf_count_boundaries(mm, wl, oracle, torch, P1, tier, kind):
    """P + 1 on either side of every step of mm_pair_nj.  Where the wide tier does not take the graph (251, 506) its environment runs
    the float64 instance, and kernels() names no wide kernel."""
    tiers = ec.BOUNDARIES[P1]
    gname = f"p1_{P1}"
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    assert g.P + 1 == P1 and g.S == 600
    if tier in tiers:
        exact_tier_case(mm, wl, oracle, gname, tier, ec.kernel_name(tier, tiers[tier]), kind, ec.BOUNDARY_SHAPE)
        return
    B, N, lens = ec.BOUNDARY_SHAPE
    V, lens = ec.shape_case(g, kind, B, N, lens)
    bf = batch_of(mm, cf, B, ec.ENV_WIDE)
    assert "mm_fbw" not in bf.kernels() and ec.kernel_name("f64", tiers["f64"]) in bf.kernels(), bf.kernels()
    gam, ttl = run(bf, V, lens)
    exact_first_counts(bf, lens)
    against_oracle(ec.reference(_refs, oracle, g, (gname, kind, B, N), V, lens), gam, ttl, lens, TTL_ATOL[kind], f"{gname} wide environment {kind}")


@pytest.mark.parametrize("P1", list(ec.BOUNDARIES))
def test_pdf_count_boundaries_on_the_float32_kernels_alone(mm, wl, oracle, torch, P1):
    """mm_fbp_kernel<NJ> at the same pdf counts, with nothing behind it (MM_NO_REDO) and nothing marked."""
    gname = f"p1_{P1}"
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    B, N, lens = ec.BOUNDARY_SHAPE
    V, lens = ec.shape_case(g, "plain", B, N, lens, ec.F32_SEED[P1])
    bf = batch_of(mm, cf, B, ec.ENV_F32)
    assert ec.kernel_name("f32", ec.BOUNDARIES[P1]["f64"]) in bf.kernels(), bf.kernels()
    gam, ttl = run(bf, V, lens)
    redo = bf.last_redo_count()
    against_oracle(ec.reference(_refs, oracle, g, (gname, "f32", B, N), V, lens), gam, ttl, lens, 1e-4, f"{gname} float32 alone, marked={redo}")
    assert redo == 0 and not bf.last_exact_first()


@pytest.mark.parametrize("kind", ["plain", "sharp"])
def test_507_pdfs_are_beyond_the_pair_family(mm, wl, oracle, torch, kind):
    g, cf = ec.compiled(_compiled, mm, wl, "p1_507")
    B, N, lens = ec.BOUNDARY_SHAPE
    V, lens = ec.shape_case(g, kind, B, N, lens)
    bf = batch_of(mm, cf, B, ec.ENV_WIDE)
    k = bf.kernels()
    assert g.P + 1 == 507 and not any(s in k for s in ("mm_fbp", "mm_fbs", "mm_fbd", "mm_fbw")), k
    gam, ttl = run(bf, V, lens)
    against_oracle(ec.reference(_refs, oracle, g, ("p1_507", kind, B, N), V, lens), gam, ttl, lens, TTL_ATOL[kind], f"p1_507 {kind}: {k[:40]}")


# ---- group B
@pytest.mark.parametrize("tier", ["wide", "f64"])
@pytest.mark.parametrize("nj", list(ec.PARTNER_GRAPHS))
def test_the_partner_in_a_pair(mm, wl, oracle, torch, nj, tier):
    """Utterance 1 (plain, 6 frames) beside six different utterances 0.  In a wide pair utterance 1's operand carries utterance 0's
    high dword as its low dword (up to 2^-20 relative on a term): the bar holds whatever the partner; on the float64 kernels, one
    utterance per workgroup, utterance 1's bits do not depend on it at all.  An emission of -inf gives a posterior of exactly 0 and
    no NaN; no utterance of 2 or more frames is left to the log-domain kernels."""
    gname = ec.PARTNER_GRAPHS[nj]
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    bf = batch_of(mm, cf, 2, ec.TIER_ENV[tier])
    assert ec.kernel_name(tier, nj) in bf.kernels() and (tier == "wide" or "mm_fbw" not in bf.kernels()), bf.kernels()
    first = None
    for partner in ec.PARTNERS:
        V, lens, hole = ec.partner_case(g, partner)
        gam, ttl = run(bf, V, lens)
        exact_first_counts(bf, lens)
        assert not np.isnan(gam).any() and not np.isnan(ttl).any()
        ref = ec.reference(_refs, oracle, g, (gname, "partner", partner), V, lens)
        atol = TTL_ATOL["sharp" if partner == "sharp" else "plain"]
        against_oracle(ref, gam, ttl, lens, atol, f"{gname} {tier} partner {partner}")
        against_oracle(ref, gam, ttl, lens, 1e-4, f"{gname} {tier} partner {partner}, utterance 1", only=np.array([False, True]))
        if hole:
            assert gam[0, hole[0], hole[1]] == 0 and ref[0][0, hole[0], hole[1]] == 0
        if first is None:
            first = (gam[1].copy(), ttl[1].copy())
        elif tier == "f64":
            assert np.array_equal(gam[1], first[0]) and np.array_equal(ttl[1], first[1]), partner


# ---- group C
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("nj", list(ec.BEHIND_GRAPHS))
def test_float64_kernels_behind_the_float32_kernels(mm, wl, oracle, torch, nj, k):
    """Three utterances of 6, 5 and 2 frames that the float32 kernels leave unmarked; then utterance k -- the first of the pair, its
    partner, the utterance of the copy pair -- is sharp.  The float64 kernels run for the marked utterances only: the workgroups of
    the others leave at once, and their outputs keep the bits that the float32 kernels alone (MM_NO_REDO) gave them.  Which
    utterances the float32 kernels mark is read from them one utterance at a time (a mark is a matter of the utterance's own
    frames), and the count of the batch must agree."""
    gname = ec.BEHIND_GRAPHS[nj]
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    V, W, lens = ec.behind_case(g, k, ec.BEHIND_SEED[nj])
    B = len(lens)
    alone = batch_of(mm, cf, B, ec.ENV_F32)
    one = batch_of(mm, cf, 1, ec.ENV_F32)
    assert ec.kernel_name("f32", nj) in alone.kernels()
    run(alone, V, lens)
    assert alone.last_redo_count() == 0  # (the plain batch: nothing marked)
    g32, t32 = run(alone, W, lens)
    marked_n = alone.last_redo_count()
    marked = np.zeros(B, dtype=bool)
    for b in range(B):
        run(one, W[b : b + 1], lens[b : b + 1])
        marked[b] = one.last_redo_count() == 1
    assert marked[k] and marked_n == marked.sum(), (marked, marked_n)
    bf = batch_of(mm, cf, B, ec.ENV_BEHIND)
    assert ec.kernel_name("f32", nj) in bf.kernels() and ec.kernel_name("f64", nj) in bf.kernels(), bf.kernels()
    gam, ttl = run(bf, W, lens)
    assert not bf.last_exact_first() and bf.last_redo_count() == marked_n and bf.last_fallback_count() == 0
    for b in np.flatnonzero(~marked):
        assert np.array_equal(gam[b], g32[b]) and np.array_equal(ttl[b], t32[b]), b
    ref = ec.reference(_refs, oracle, g, (gname, "behind", k), W, lens)
    against_oracle(ref, gam, ttl, lens, 1e-3, f"{gname} behind float32, utterance {k} sharp, marked {marked.astype(int)}", only=marked)
    against_oracle(ref, gam, ttl, lens, 1e-4, f"{gname} behind float32, the unmarked", only=~marked)


# ---- group D
@pytest.mark.parametrize("kind", ["plain", "sharp"])
@pytest.mark.parametrize("B,N,lens", ec.TEAM_SHAPES)
@pytest.mark.parametrize("gname,tier", [(gname, tier) for gname, t in ec.TEAMS.items() for tier in (("wide", "f64") if t[2] else ("f64",))])
def test_team_instances(mm, wl, oracle, torch, gname, tier, B, N, lens, kind):
    nj, H, wide = ec.TEAMS[gname]
    g, cf = ec.compiled(_compiled, mm, wl, gname)
    if not wide:  # (mm_wpair_fits: teams of 2 and up to 250 pdfs -- without MM_NO_WPAIR the batch names no wide kernel either)
        assert "mm_fbw" not in batch_of(mm, cf, B, ec.ENV_WIDE).kernels()
    exact_tier_case(mm, wl, oracle, gname, tier, ec.kernel_name(tier, nj, H), kind, (B, N, lens))
