"""Every instance of the stream kernels on a GPU: mm_stream_kernel<NJ,H> for NJ in {2, 4, 8, 16} passes over the pdfs and teams of
H in {1, 2, 4} workgroups (csrc/mm_stream.hip), with mm_stream_combine_kernel and mm_stream_finish_kernel behind it, at the sizes
where each can go wrong -- both sides of every step of NJ, the most pdfs (1023) and states (S1 = 16370) the form holds and one more
of each, rows of every lane-group width and several whole-wave rows per set of a team, pdfs without states, lengths around the
combine kernel's groups of 8 frames, batch sizes at every step of the team size and on both sides of the one-grid / two-launch cut,
a strided V inside a buffer of NaN.

Every case asserts the instance by name from kernels() of the batch that ran, a redo count of 0 (an utterance handed to the item
kernel would hide a wrong stream result), the float64 C oracle through check_gamma, ttl at rtol 1e-5 / atol 1e-3 (the bars of
test_stream_kernels), identical bits on a second call, and -- for teams -- np.allclose(rtol=2e-5, atol=1e-7) with the lone
workgroup's result on the same input.  tests/test_stream_inputs.py shows without a GPU that these inputs can fail.

Batches of graphs with different numbers of pdfs are refused by BatchedFSM (DimensionMismatch): no such case here."""
import numpy as np
import pytest

import graphs
import stream_cases as sc
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu
HS = (1, 2, 4)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_compiled, _results = {}, {}


def compiled(mm, wl, g):
    if id(g) not in _compiled:
        _compiled[id(g)] = (g, mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P)))
    return _compiled[id(g)][1]


def instance(kernels):
    """(NJ, H) of a kernels() string, None if the stream kernels do not run."""
    import re

    m = re.search(r"mm_stream_kernel<(\d+),(\d+)>", kernels)
    assert (m is not None) == ("mm_stream_kernel" in kernels), kernels
    return (int(m.group(1)), int(m.group(2))) if m else None


def check_against_oracle(what, gam, ttl, g_ref, t_ref, lens):
    ok = np.isfinite(t_ref)
    worst = check_gamma(gam[ok], g_ref[ok], lens[ok])
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=1e-3), (ttl, t_ref)
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()  # (no frame: no path)
    print(f"{what}: worst log-posterior error at {worst:.3g} of its bar")
    return worst


def run_stream(mm, wl, oracle, key, gs, V, lens, H, nj, force=True, call=None):
    """One batch on mm_stream_kernel<nj,H> (H None: the engine's team size, no MM_STREAM_H; force False: no MM_KERNEL either -- the
    engine picks the family) with every assertion of this file's header; memoised under (key, H); returns (gamma, ttl)."""
    if (key, H) in _results:
        return _results[(key, H)]
    env = {"MM_DEBUG": "1"}
    if force:
        env["MM_KERNEL"] = "stream"
    if H is not None:
        assert H == 1 or 2 * len(gs) * H <= 256  # (a forced team that cannot co-run would time out by design)
        env["MM_STREAM_H"] = str(H)
    bf = _with_env(env, lambda: mm.batch(*[compiled(mm, wl, g) for g in gs]))
    kernels = bf.kernels()
    got = instance(kernels)
    print(f"{key}: {kernels.split(' (')[0]}")
    assert got is not None and got[0] == nj and (H is None or got[1] == H), kernels
    assert f"mm_stream_kernel<{got[0]},{got[1]}>" in kernels and "mm_stream_combine_kernel" in kernels
    assert (f"teams of {got[1]}" in kernels) == (got[1] > 1) and ("teams of" in kernels) == (got[1] > 1), kernels
    gam, ttl = call(bf) if call else bf.pdfposteriors(V, lens)
    assert bf.last_redo_count() == 0
    g_ref, t_ref = sc.reference(oracle, graphs, gs, V, lens, key)
    check_against_oracle(f"{key}, <{got[0]},{got[1]}>", gam, ttl, g_ref, t_ref, lens)
    g2, t2 = call(bf) if call else bf.pdfposteriors(V, lens)  # (float64 sums in a fixed order: the same bits on every run)
    assert np.array_equal(g2, gam) and np.array_equal(t2, ttl) and bf.last_redo_count() == 0
    _results[(key, H)] = (gam, ttl, got)
    return _results[(key, H)]


def run_team_sizes(mm, wl, oracle, key, gs, V, lens, H, nj, force=True):
    gam, ttl, _ = run_stream(mm, wl, oracle, key, gs, V, lens, H, nj, force)
    if H > 1:  # (other sums than the lone workgroup's: not the same bits)
        g1, _, _ = run_stream(mm, wl, oracle, key, gs, V, lens, 1, nj, force)
        assert np.allclose(gam, g1, rtol=2e-5, atol=1e-7)
    return gam, ttl


def run_elsewhere(mm, wl, oracle, key, gs, V, lens):
    """A batch the stream form refuses, with no switch set: it must not name the stream kernel and still match the oracle."""
    bf = mm.batch(*[compiled(mm, wl, g) for g in gs])
    kernels = bf.kernels()
    print(f"{key}: {kernels.split(' (')[0]}")
    assert "mm_stream" not in kernels, kernels
    gam, ttl = bf.pdfposteriors(V, lens)
    check_against_oracle(key, gam, ttl, *sc.reference(oracle, graphs, gs, V, lens, key), lens)


# ---- group P: the pdf count at every step of NJ, and at the form's maximum
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("P", sc.P_EDGES)
def test_pdf_count_at_every_step(mm, wl, oracle, torch, P, H):
    g, V, lens = sc.case_p(wl, P)
    nj = {127: 2, 128: 4, 255: 4, 256: 8, 511: 8, 512: 16, 1023: 16}[P]
    assert nj == sc.stream_nj(P)
    # (more than 506 pdfs are beyond every other fast family: the engine takes the stream kernels by itself, no MM_KERNEL)
    run_team_sizes(mm, wl, oracle, f"P{P}", [g] * len(lens), V, lens, H, nj, force=P <= 506)


def test_one_pdf_more_than_the_form_holds(mm, wl, oracle, torch):
    P = sc.P_MAX + 1
    g, V, lens = sc.case_p(wl, P)
    run_elsewhere(mm, wl, oracle, f"P{P}", [g] * len(lens), V, lens)


# ---- group R: rows of 2 and 4 lanes and whole-wave rows, in both directions and in every set of a team
@pytest.mark.parametrize("H", HS)
def test_row_groups_and_whole_wave_rows(mm, wl, oracle, torch, H):
    g, V, lens = sc.case_r(wl)
    run_team_sizes(mm, wl, oracle, "midrows", [g] * len(lens), V, lens, H, 2)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("first", ["midrows", "pedge127"])
def test_different_graphs_in_one_batch(mm, wl, oracle, torch, first, H):
    """mid_row_graph and p_edge_graph(127): different graphs of different S (1200 and 600 states) in one batch, in both orders."""
    gm, Vm, _ = sc.case_r(wl)
    gp, Vp, _ = sc.case_p(wl, 127)
    gs, V = ([gm, gp], np.stack([Vm[0], Vp[0]])) if first == "midrows" else ([gp, gm], np.stack([Vp[0], Vm[0]]))
    run_team_sizes(mm, wl, oracle, f"mixed_{first}", gs, V, np.asarray([19, 12], dtype=np.int32), H, 2)


# ---- group S: the most states the form holds -- LDS byte offsets that use all 16 bits
@pytest.mark.parametrize("H", HS)
def test_state_count_at_the_limit(mm, wl, oracle, torch, H):
    g, V, lens = sc.case_s(wl, sc.S1_LIMIT)
    assert compiled(mm, wl, g).S1 == sc.S1_LIMIT
    run_team_sizes(mm, wl, oracle, "limit16370", [g] * len(lens), V, lens, H, 16, force=False)


def test_one_state_more_than_the_form_holds(mm, wl, oracle, torch):
    g, V, lens = sc.case_s(wl, sc.S1_LIMIT + 1)
    assert compiled(mm, wl, g).S1 == sc.S1_LIMIT + 1
    run_elsewhere(mm, wl, oracle, "limit16371", [g] * len(lens), V, lens)


# ---- group E: pdfs without states
@pytest.mark.parametrize("H", [1, 4])
def test_pdfs_without_states(mm, wl, oracle, torch, H):
    g, V, lens = sc.case_e(wl)
    gam, _ = run_team_sizes(mm, wl, oracle, "emptypdfs", [g] * len(lens), V, lens, H, 8)
    assert (gam[:, :, list(sc.EMPTY_PDFS)] == 0).all()
    for b, L in enumerate(lens):
        assert np.allclose(gam[b, :L].sum(-1), 1.0, atol=1e-5)


# ---- group B: the team size by the batch size, one grid or a launch per direction
@pytest.mark.parametrize("B,H", [(32, 4), (33, 2), (64, 2), (65, 1), (128, 1), (129, 1)])
def test_batch_size_picks_the_team_and_the_launch_shape(mm, wl, oracle, torch, B, H):
    """mm_stream_pick_h on 256 compute units: 2 B H workgroups must fit the chip -- teams of 4 up to B = 32, of 2 up to 64, then
    lone workgroups, in one grid up to B = 128 and in a launch per direction from 129 on."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the steps of the team size are stated for 256 compute units, this device has {cus}")
    g, V, lens = sc.case_b(wl, B)
    assert {0, 1, 9} <= set(lens.tolist())
    _, _, got = run_stream(mm, wl, oracle, f"B{B}", [g] * B, V, lens, None, 2)
    assert got == (2, H)


# ---- group V: a strided V in a buffer of NaN, lengths on the device
def test_strided_emissions_inside_nan(mm, wl, oracle, torch):
    g, V, lens = sc.case_p(wl, 256)
    B, n, P = V.shape
    buf = torch.full((B, n + 3, P + 5), float("nan"), device="cuda")
    Vd = buf[:, 1 : n + 1, 2 : P + 2]
    Vd.copy_(torch.from_numpy(V))
    for b, L in enumerate(lens):  # the frames beyond the lengths: NaN and +inf in turn
        Vd[b, L:] = float("nan")
        Vd[b, L + 1 :: 2] = float("inf")
    assert not Vd.is_contiguous() and Vd.stride(2) == 1
    ld = torch.from_numpy(lens).cuda()

    def call(bf):
        gam, ttl = bf.pdfposteriors(Vd, ld)
        torch.cuda.synchronize()
        return gam.cpu().numpy(), ttl.cpu().numpy()

    gam, ttl, _ = run_stream(mm, wl, oracle, "P256_view", [g] * B, V, lens, 2, 8, call=call)
    assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, :, :2]).all() and torch.isnan(buf[:, :, P + 2 :]).all()
    # the same input as a plain array: the same bits
    g0, t0, _ = run_stream(mm, wl, oracle, "P256", [g] * B, V, lens, 2, 8)
    assert np.array_equal(gam, g0) and np.array_equal(ttl, t0)
