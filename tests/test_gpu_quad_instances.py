"""Every instance of the quad kernels on a GPU: mm_fbq_kernel<KQ,RPT,PASS> (csrc/mm_kernel_quad.hip; 18 KQ x RPT 2, 3 x the forward and
the backward pass, instances in csrc/mm_quad_tu.hip), and the data-dependent branches inside them -- quads on virtual lanes at both
sides of the register window, rows of 0 .. 9 extra lane ends (row_short, row_long) in both passes, the rows of the generic loop, the
three bodies of the exact fallback on rows of 1, 4, 5, 8 and 9 arcs, pdf counts on both sides of every 64-lane pass, every wave count
with a branch of its own, the short lengths, and the second pass behind the row kernels.

Every case forces MM_DEBUG=1 MM_KERNEL=quad (and MM_KQ, MM_NWAVES, MM_NO_XCSR) around the creation of its batch, asserts the instance
by name from kernels() -- the name tests/quad_cases.py derives from the graph's degrees --, checks EVERY utterance against the float64
C oracle through check_gamma, ttl at rtol 1e-5 / atol 1e-4 (5e-4 on the deep and the sharp inputs: the bars of test_gpu_parity.py),
exact zeros and ttl = -inf where the reference has no path, and identical bits on a second call (the kernel has no atomics).
tests/test_quad_inputs.py shows without a GPU that these inputs can fail."""
import numpy as np
import pytest

import exact_cases as ec
import graphs
import quad_cases as qc
from test_gpu_parity import _with_env
from test_gpu_wave_lane_instances import check_against_oracle, compiled, make_batch

pytestmark = pytest.mark.gpu
REDO_TEXT = "then for marked utterances only "


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def run_case(mm, wl, oracle, key, gs, V, lens, kq=None, nwaves=None, no_xcsr=False, atol=1e-4, also=()):
    """One batch with every assertion of this file's header.  Returns (gamma, ttl, the batch)."""
    bf = make_batch(mm, wl, gs, V.shape[2], qc.quad_env(kq, nwaves, no_xcsr))
    kernels = bf.kernels()
    print(f"{key}: {kernels}")
    for w in qc.instances(gs, kq, nwaves) + list(also):
        assert w in kernels, (w, kernels)
    assert "mm_log_kernel" not in kernels and REDO_TEXT not in kernels, kernels
    gam, ttl = bf.pdfposteriors(V, lens)
    check_against_oracle(key, gam, ttl, *qc.reference(oracle, graphs, gs, V, lens, key), lens, atol)
    g2, t2 = bf.pdfposteriors(V, lens)
    assert np.array_equal(g2, gam) and np.array_equal(t2, ttl)
    return gam, ttl, bf


# ---- 1: every KQ, both passes, both RPT
@pytest.mark.parametrize("nwaves", [None, 1])
@pytest.mark.parametrize("kq", qc.KQ_ALL)
def test_every_kq_instance(mm, wl, oracle, torch, kq, nwaves):
    """<KQ,2,.> at the engine's wave count and <KQ,3,.> at one wave (rows in the generic loop; quads on virtual lanes up to KQ = 21)."""
    g, V, lens = qc.mixed300_case(wl)
    rpt = 2 if nwaves is None else 3
    run_case(mm, wl, oracle, "Q1", [g] * len(lens), V, lens, kq, nwaves, also=[f"mm_fbq_kernel<{kq},{rpt},0>", f"mm_fbq_kernel<{kq},{rpt},1>"])


# ---- 2: virtual lanes
@pytest.mark.parametrize("kq,nq", qc.VIRTUAL_CASES)
def test_virtual_lanes_at_the_register_window(mm, wl, oracle, torch, kq, nq):
    g, V, lens = qc.virtual_case(wl, nq)
    run_case(mm, wl, oracle, ("Q2", nq), [g] * len(lens), V, lens, kq, 1, also=[" x 1 waves"])


def test_virtual_lanes_on_eight_waves(mm, wl, oracle, torch):
    g, V, lens = qc.dense400_case(wl)
    run_case(mm, wl, oracle, "Q2_dense", [g] * len(lens), V, lens, 15, also=["mm_fbq_kernel<15,2,0> x 8 waves", "mm_fbq_kernel<15,2,1> x 8 waves"])


# ---- 3: rows of every kind
@pytest.mark.parametrize("kq", [1, 5])
@pytest.mark.parametrize("extra", qc.HUB_EXTRAS)
def test_rows_of_every_number_of_lane_ends(mm, wl, oracle, torch, extra, kq):
    g, V, lens = qc.hub_case(wl, extra, kq)
    run_case(mm, wl, oracle, ("Q3", extra, kq), [g] * len(lens), V, lens, kq)


@pytest.mark.parametrize("kq", [1, 5])
def test_the_phony_final_row_as_a_long_row(mm, wl, oracle, torch, kq):
    g, V, lens = qc.many_finals_case(wl)
    run_case(mm, wl, oracle, "Q3_finals", [g] * len(lens), V, lens, kq)


@pytest.mark.parametrize("kq", qc.LATE_HUB_KQ)
def test_a_long_row_in_the_backward_generic_loop(mm, wl, oracle, torch, kq):
    """A long row beyond the register-carried rows of the backward pass (one wave): row_total in the generic loop takes the long walk."""
    g, V, lens = qc.late_hub_case(wl)
    run_case(mm, wl, oracle, "Q3_late", [g] * len(lens), V, lens, kq, 1, also=[f"mm_fbq_kernel<{kq},3,1> x 1 waves"])


# ---- 4: the exact fallback
@pytest.mark.parametrize("which", ["deep", "sharp"])
@pytest.mark.parametrize("body", list(qc.FALLBACK_ENVS))
def test_exact_fallback_bodies(mm, wl, oracle, torch, body, which):
    """exact_row_lds (KQ = 1, the CSR in LDS), exact_row<true> (KQ = 1, MM_NO_XCSR) and exact_row<false> (KQ = 5) on a deep graph with
    rows of 1, 4, 5, 8 and 9 arcs, and on a shallow graph under sharp emissions: rows that are dead next to rows that are alive and
    below the range of the linear sums (tests/test_quad_inputs.py)."""
    g, V, lens = qc.deep_case(wl) if which == "deep" else qc.sharp_case(wl)
    e = qc.FALLBACK_ENVS[body]
    where = "(fallback CSR in LDS)" if body == "lds" else "(fallback CSR in global memory)"
    run_case(mm, wl, oracle, f"Q4_{which}", [g] * len(lens), V, lens, e["kq"], None, e.get("no_xcsr", False), atol=5e-4, also=[where])


# ---- 5: the pdf count
@pytest.mark.parametrize("P,nwaves", [(P, 1) for P in qc.P_EDGES_ONE_WAVE] + [(P, 2) for P in qc.P_EDGES_TWO_WAVES])
def test_pdf_count_at_every_pass(mm, wl, oracle, torch, P, nwaves):
    g, V, lens = qc.pdf_edge_case(wl, P)
    gam, _, _ = run_case(mm, wl, oracle, ("Q5", P), [g] * len(lens), V, lens, None, nwaves, also=[f" x {nwaves} waves"])
    assert (gam[:, :, qc.EMPTY_PDF] == 0).all()


# ---- 6: the wave count
@pytest.mark.parametrize("kq,nwaves", qc.WAVE_CASES)
def test_every_wave_count(mm, wl, oracle, torch, kq, nwaves):
    g, V, lens = qc.big_case(wl)
    run_case(mm, wl, oracle, "Q6", [g] * len(lens), V, lens, kq, nwaves, also=[f"mm_fbq_kernel<{kq},{2 if nwaves == 16 else 3},1> x {nwaves} waves"])


# ---- 7: the lengths
@pytest.mark.parametrize("nwaves", [None, 1])
def test_every_short_length(mm, wl, oracle, torch, nwaves):
    """Lengths 0 .. 5 and N in one batch, each from 1 on with an accepting path (the one-step loop of length 1, the two-frame ring of
    the pdf sums, the lag of the posteriors, the frame-2 finish), an utterance of full length without a path, and one call without
    lengths."""
    g, V, lens = qc.lengths_case(wl)
    _, ttl, _ = run_case(mm, wl, oracle, "Q7", [g] * 8, V, lens, None, nwaves)
    assert np.isneginf(ttl[list(qc.LENGTHS_DEAD)]).all() and np.isfinite(ttl[1:7]).all()
    run_case(mm, wl, oracle, "Q7_none", [g] * 7, V[:7], None, None, nwaves)


# ---- 8: FSMs on different pdf counts in one batch
def test_binding_refuses_different_pdf_counts(mm, wl, torch):
    """fb_exact keeps the caller's emissions (no mm_shift_em_kernel) when the FSMs of a batch differ in P1; the Python binding never
    builds such a batch -- it refuses it --, so that path has no case here."""
    a, b = qc.chain_graph(wl, 70), qc.pdf_edge_graph(wl, 9)
    with pytest.raises(mm.DimensionMismatch):
        _with_env(qc.FORCE_QUAD, lambda: mm.batch(compiled(mm, wl, a, a.P), compiled(mm, wl, b, b.P)))


# ---- 9: the second pass behind the row kernels
def test_second_pass_behind_the_row_kernels(mm, wl, oracle, torch):
    """MM_KERNEL=row on exact_cases' batch of three utterances of which one is sharp: the row kernels mark it, the quad kernels compute
    it again and it matches the oracle; the others keep the bits they have in the batch where nothing is marked."""
    cache = {}
    g, cf = ec.compiled(cache, mm, wl, "nj2")
    env = {"MM_DEBUG": "1", "MM_KERNEL": "row"}
    bf = _with_env(env, lambda: mm.batch(cf, cf, cf))
    kernels = bf.kernels()
    print(kernels)
    assert "mm_fbr_kernel" in kernels and REDO_TEXT + "mm_fbq_kernel<" in kernels, kernels
    for k in range(3):
        V, W, lens = ec.behind_case(g, k, ec.BEHIND_SEED[2])
        g0, t0 = bf.pdfposteriors(V, lens)
        assert bf.last_redo_count() == 0
        g1, t1 = bf.pdfposteriors(W, lens)
        assert bf.last_redo_count() == 1  # (the others' inputs are those of the plain batch: the marked one is k)
        g_ref, t_ref = ec.reference(cache, oracle, g, ("behind", k), W, lens)
        check_against_oracle(f"Q9_{k}", g1, t1, g_ref, t_ref, lens, 5e-4)
        others = [b for b in range(3) if b != k]
        assert np.array_equal(g1[others], g0[others]) and np.array_equal(t1[others], t0[others])
        g2, t2 = bf.pdfposteriors(W, lens)
        assert np.array_equal(g2, g1) and np.array_equal(t2, t1)


# ---- MM_KQ values without an instance
@pytest.mark.parametrize("kq", qc.OFF_TABLE_KQ)
def test_kq_without_an_instance_is_ignored(mm, wl, oracle, torch, kq):
    """MM_KQ = 4, 8, 12, ... has no kernel instance: the batch keeps the geometry it would have without the switch (it used to name a
    quad instance and run the item kernel), and kernels() says so."""
    g, V, lens = qc.mixed300_case(wl)
    _, _, bf = run_case(mm, wl, oracle, "Q1", [g] * len(lens), V, lens, kq)
    plain = make_batch(mm, wl, [g] * len(lens), g.P, qc.FORCE_QUAD)
    assert bf.kernels() == plain.kernels() and f"mm_fbq_kernel<{kq}," not in bf.kernels()
