"""Every instance of the two kernels pick_family tries first, on a GPU: mm_wave_kernel<NSEG,NJ,TWO> (csrc/mm_kernel_wave.hip: <2,2>,
<2,4>, <4,2>, <4,4>, <2,2,two per CU>, <2,4,two per CU>) and mm_lane_kernel<NS> (csrc/mm_kernel_lane.hip: NS = 8, 16, 32, 64), at the
sizes where each can go wrong -- pdf counts on both sides of every 64-lane pass, one utterance per length 0, 1, 2, ... (the time
split, the requests ahead, the rings, the posteriors' lag), the forms' limits at the value and one beyond, rows and pdfs of every
lane-group width, graphs of fewer segments than waves, different graphs in one batch, state counts on both sides of every lane
instance, state maps on exactly 64 pdfs, and the lane kernel's hand-off of marked utterances to the wave and to the item kernel.

Every case asserts the instance by name from kernels() of the batch that ran, EVERY utterance against the float64 C oracle through
check_gamma, ttl at rtol 1e-5 / atol 5e-4 (wave) or 1e-3 (lane) -- the bars these kernels have in test_gpu_parity.py and
test_gpu_exact.py --, exact zeros and ttl = -inf where the reference has no path, and identical bits on a second call.
tests/test_wave_lane_inputs.py shows without a GPU that these inputs can fail."""
import numpy as np
import pytest

import graphs
import wave_cases as wc
from test_gpu_parity import GAMMA_FLOOR, RTOL_LOGPOST, _with_env, check_gamma
from test_wave_lane_inputs import float32_over_bars

pytestmark = pytest.mark.gpu
FORCE_WAVE = {"MM_DEBUG": "1", "MM_KERNEL": "wave"}
REDO_TEXT = "then for marked utterances only "


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def n_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


_compiled = {}


def compiled(mm, wl, g, P):
    if (id(g), P) not in _compiled:
        _compiled[(id(g), P)] = (g, mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, P)))
    return _compiled[(id(g), P)][1]


def make_batch(mm, wl, gs, P, env=None):
    return _with_env(env or {}, lambda: mm.batch(*[compiled(mm, wl, g, P) for g in gs]))


def check_gamma_scaled(g, g_ref, lens, a_bar, l_bar):
    """check_gamma with its absolute bar times a_bar and its log-posterior bar times l_bar (the long chains alone: 4 times what
    the oracle's own float32 mode loses there, test_wave_lane_inputs.py::test_float32_on_the_long_chains); everything else as there.
    Returns the worst log-posterior error over the UNSCALED bar."""
    g = np.asarray(g, dtype=np.float64)
    assert np.isfinite(g).all()
    for b, L in enumerate(lens):
        assert (g[b, L:] == 0).all() and np.allclose(g[b, :L].sum(-1), 1.0, atol=1e-5)
    a = np.abs(g - g_ref).max() / 2e-5
    m = g_ref > GAMMA_FLOOR
    assert (g[m] > 0).all()
    lg, lr = np.log(g[m]), np.log(g_ref[m])
    l = float(np.max(np.abs(lg - lr) / (RTOL_LOGPOST * np.maximum(np.abs(lr), 1.0))))
    print(f"abs criterion at {a:.3g} of check_gamma's bar (allowed: {a_bar:.3g}), log-posterior criterion at {l:.3g} (allowed: {l_bar:.3g})")
    assert a <= a_bar and l <= l_bar, (a, a_bar, l, l_bar)
    return l


def check_against_oracle(what, gam, ttl, g_ref, t_ref, lens, atol, bars=None):
    """Every utterance; returns check_gamma's worst log-posterior error over its bar."""
    lens = np.full(len(ttl), gam.shape[1], dtype=np.int32) if lens is None else lens
    ok = np.isfinite(t_ref)
    if bars:
        worst = check_gamma_scaled(gam[ok], g_ref[ok], lens[ok], *bars)
    else:
        worst = check_gamma(gam[ok], g_ref[ok], lens[ok]) if ok.any() else 0.0
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=atol), (ttl, t_ref)
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()  # (no path: exact zeros)
    print(f"{what}: {int(ok.sum())} of {len(ok)} utterances have a path; worst log-posterior error at {worst:.3g} of its bar")
    return ok


def run_case(mm, wl, oracle, key, gs, V, lens, want, family="wave", env=None, absent=(), redo=None, bars=None):
    """One batch with every assertion of this file's header: `want` (substrings) in kernels(), `absent` not; for the lane kernel the
    redo count -- `redo` if given, else the utterances of at least one frame without a path (Z = 0 is what an underflow would look like
    too: the kernel behind looks at them again).  Returns (gamma, ttl, the batch)."""
    bf = make_batch(mm, wl, gs, V.shape[2], env)
    kernels = bf.kernels()
    print(f"{key}: {kernels.split(' (')[0]}")
    for w in [want] if isinstance(want, str) else want:
        assert w in kernels, (w, kernels)
    for w in absent:
        assert w not in kernels, (w, kernels)
    gam, ttl = bf.pdfposteriors(V, lens)
    g_ref, t_ref = wc.reference(oracle, graphs, gs, V, lens, key)
    ok = check_against_oracle(key, gam, ttl, g_ref, t_ref, lens, 1e-3 if family == "lane" else 5e-4, bars)
    if family == "lane":
        n_lens = np.full(len(gs), V.shape[1]) if lens is None else lens
        count = bf.last_redo_count()
        assert count == redo if isinstance(redo, int) else redo(count) if redo else count == int((~ok & (n_lens >= 1)).sum()), count
    g2, t2 = bf.pdfposteriors(V, lens)
    assert np.array_equal(g2, gam) and np.array_equal(t2, ttl)
    return gam, ttl, bf


def run_elsewhere(mm, wl, oracle, key, gs, V, lens, absent, env=None, bars=None):
    """A batch the family refuses: it must not name the family's kernel and still match the oracle (ttl at the looser of the bars)."""
    bf = make_batch(mm, wl, gs, V.shape[2], env)
    kernels = bf.kernels()
    print(f"{key}: {kernels.split(' (')[0]}")
    assert absent not in kernels, kernels
    gam, ttl = bf.pdfposteriors(V, lens)
    check_against_oracle(key, gam, ttl, *wc.reference(oracle, graphs, gs, V, lens, key), lens, 1e-3, bars)


# =============================================== the wave kernel
# ---- W1: the six instances
@pytest.mark.parametrize("graph,nj", [("sparse20", 2), ("pedge128", 4)])
@pytest.mark.parametrize("size", ["three", "n_cus", "n_cus_plus_1"])
def test_wave_two_segment_instances(mm, wl, oracle, torch, n_cus, graph, nj, size):
    """<2,2> and <2,4>, and their builds of which two workgroups fit a compute unit: taken from one utterance more than the device has
    compute units, not at exactly as many."""
    B, N = {"three": (3, 19), "n_cus": (n_cus, 9), "n_cus_plus_1": (n_cus + 1, 9)}[size]
    g, V, lens = wc.sparse20_case(wl, B, N) if graph == "sparse20" else wc.pdf_edge_case(wl, 128, B, N)
    two = size == "n_cus_plus_1"
    want = f"mm_wave_kernel<2,{nj},two per CU>" if two else f"mm_wave_kernel<2,{nj}>"
    run_case(mm, wl, oracle, f"W1_{graph}_{size}", [g] * B, V, lens, want, absent=() if two else ("two per CU",))


@pytest.mark.parametrize("which,want", [("five", "<4,2>"), ("five_p130", "<4,4>"), ("densewide", "<4,2>")])
def test_wave_four_segment_instances(mm, wl, oracle, torch, which, want):
    """<4,.>: five pdf segments (two per wave) at P <= 127 and at P >= 128, and a dense graph of more than 8 state segments."""
    if which == "densewide":
        g = wc.dense_wide(wl)
        V, lens = wc.emissions(3, 19, g.P, 88), np.asarray((19, 10, 1), dtype=np.int32)
    else:
        g, V, lens = wc.pdf_group_case(wl, which)
    gam, _, _ = run_case(mm, wl, oracle, f"W1_{which}", [g] * len(lens), V, lens, "mm_wave_kernel" + want)
    assert (gam[:, :, wc.pdf_group_empty(g)] == 0).all()


# ---- W2: the pdf count
@pytest.mark.parametrize("P", wc.P_EDGES)
def test_wave_pdf_count_at_every_pass(mm, wl, oracle, torch, P):
    g, V, lens = wc.pdf_edge_case(wl, P)
    run_case(mm, wl, oracle, f"W2_P{P}", [g] * len(lens), V, lens, ["mm_wave_kernel<", f",{wc.wave_nj(P)}>"])


def test_wave_250_pdfs_run_elsewhere(mm, wl, oracle, torch):
    """P1 <= 250 is the engine's choice: 250 pdfs (P1 = 251) do not get the wave kernel."""
    g, V, lens = wc.pdf_edge_case(wl, 250)
    run_elsewhere(mm, wl, oracle, "W2_P250", [g] * len(lens), V, lens, "mm_wave_kernel")


def test_wave_forced_at_the_launch_limit_of_pdfs(mm, wl, oracle, torch):
    """Asked for by name, the kernel takes what its launch holds: 255 pdfs (P1 = 256) on <.,4>; 256 pdfs run no wave kernel."""
    g, V, lens = wc.pdf_edge_case(wl, 255)
    run_case(mm, wl, oracle, "W2_P255", [g] * len(lens), V, lens, ["mm_wave_kernel<", ",4>"], env=FORCE_WAVE)
    g, V, lens = wc.pdf_edge_case(wl, 256)
    run_elsewhere(mm, wl, oracle, "W2_P256", [g] * len(lens), V, lens, "mm_wave_kernel", env=FORCE_WAVE)


# ---- W3: one utterance per length
@pytest.mark.parametrize("which,want", [("wave2", "mm_wave_kernel<2,2>"), ("wave4", "mm_wave_kernel<4,2>")])
def test_wave_every_short_length(mm, wl, oracle, torch, which, want):
    """Lengths 0, 1, 2, ..., 12, 16, 17 in one batch -- the time split m = NF / 2 at both parities, fewer frames than the four steps
    the emissions are requested ahead and than the ring of 8 partner offsets, the posteriors' tail of two frames -- and one call
    without lengths."""
    g = wc.sparse20(wl) if which == "wave2" else wc.four_segment(wl)
    V, lens = wc.lengths_case(wl, g, wc.WAVE_LENS, 70)
    run_case(mm, wl, oracle, ("lengths", which), [g] * len(lens), V, lens, want)
    run_case(mm, wl, oracle, ("lengths_none", which), [g] * len(lens), V, None, want)


# ---- W4: the state count
@pytest.mark.parametrize("S1", wc.LIMIT_S1)
def test_wave_state_count_up_to_the_limit(mm, wl, oracle, torch, S1):
    """Chains of S1 = 511, 512, 513, 1023 (the most pick_family's wave-first rule takes) and 1024 states (16 full segments, the most
    the form holds: a deep chain gets there through pick_family's second wave rule), N = S1 + 8 frames.  At 519 .. 1032 dependent
    steps float32 itself misses check_gamma's bars -- the oracle's recursion in float32 against float64: 5.4 .. 14 times the absolute
    bar, 1.7 .. 3.4 times the log-posterior bar --, so these cases alone allow 4 times what the float32 oracle loses (for the
    different order of the kernel's roundings).  The kernel measured 0.74, 1.1, 1.3, 6.7 times the absolute bar at 511, 512, 513,
    1023 and 0.49 .. 3.2 times the log-posterior bar: less than the float32 oracle everywhere."""
    g, V, lens = wc.limit_case(wl, S1)
    assert compiled(mm, wl, g, g.P).S1 == S1
    a32, l32 = float32_over_bars(oracle, g, V, lens, f"W4_chain{S1}")
    run_case(mm, wl, oracle, f"W4_chain{S1}", [g] * 2, V, lens, "mm_wave_kernel<2," if S1 <= 512 else "mm_wave_kernel<4,",
             bars=(max(1.0, 4 * a32), max(1.0, 4 * l32)))


def test_wave_one_state_more_than_the_form_holds(mm, wl, oracle, torch):
    """1025 states are 17 segments: another family (float32 in the log domain as well: the long chains' bars, see above)."""
    g, V, lens = wc.limit_case(wl, 1025)
    assert compiled(mm, wl, g, g.P).S1 == 1025
    a32, l32 = float32_over_bars(oracle, g, V, lens, "W4_chain1025")
    run_elsewhere(mm, wl, oracle, "W4_chain1025", [g] * 2, V, lens, "mm_wave_kernel", bars=(max(1.0, 4 * a32), max(1.0, 4 * l32)))


def test_wave_graphs_of_fewer_segments_than_waves(mm, wl, oracle, torch):
    """The 3-state demo HMM and a 2-state graph, asked for by name (they are the lane kernel's otherwise): one segment, so three of an
    agent's four compute waves own none and only keep the step."""
    l2r, two = wc.tiny_for_wave(wl)
    gs = [l2r, two, l2r, two, l2r]
    lens = np.asarray((7, 7, 3, 1, 2), dtype=np.int32)
    run_case(mm, wl, oracle, "W4_tiny", gs, wc.emissions(5, 7, 3, 12), lens, "mm_wave_kernel<2,2>", env=FORCE_WAVE)


# ---- W5: rows and pdf groups of every width
@pytest.mark.parametrize("widest", [255, 256])
def test_wave_rows_of_every_group_width(mm, wl, oracle, torch, widest):
    g, V, lens = wc.hub_case(wl, widest)
    run_case(mm, wl, oracle, f"W5_hubs{widest}", [g] * len(lens), V, lens, "mm_wave_kernel<4,2>")


def test_wave_pdf_groups_of_every_width(mm, wl, oracle, torch):
    g, V, lens = wc.pdf_group_case(wl, "base")
    gam, _, _ = run_case(mm, wl, oracle, "W5_pdfgroups", [g] * len(lens), V, lens, "mm_wave_kernel<4,2>")
    assert wc.pdf_group_empty(g).tolist() == [0, 8, 16] and (gam[:, :, [0, 8, 16]] == 0).all()


@pytest.mark.parametrize("which", ["hubs257", "pdf257", "nine"])
def test_wave_refused_shapes_run_elsewhere(mm, wl, oracle, torch, which):
    """A row of 257 arcs, a pdf of 257 states, nine pdf segments: another family, the same answer."""
    g, V, lens = wc.hub_case(wl, 257) if which == "hubs257" else wc.pdf_group_case(wl, which)
    run_elsewhere(mm, wl, oracle, f"W5_{which}", [g] * len(lens), V, lens, "mm_wave_kernel")


# ---- W6: different graphs in one batch
@pytest.mark.parametrize("first", ["small", "large"])
def test_wave_two_and_four_segment_graphs_in_one_batch(mm, wl, oracle, torch, first):
    """A graph whose waves own fewer than NSEG segments next to one that fills them, different S1, lengths 1 and N; both orders."""
    a, b = wc.sparse20(wl), wc.four_segment(wl)
    gs = [a, b, a, b] if first == "small" else [b, a, b, a]
    lens = np.asarray((23, 23, 1, 1), dtype=np.int32)
    run_case(mm, wl, oracle, f"W6_{first}", gs, wc.emissions(4, 23, 20, 66), lens, "mm_wave_kernel<4,2>")


# ---- W7: calling conventions
def test_wave_strided_views_inside_nan(mm, wl, oracle, torch):
    """V and gamma as strided views of buffers filled with NaN, NaN and +inf in V beyond the lengths, the lengths on the device: the
    bits of the plain arrays, and nothing written outside the view."""
    g, V, lens = wc.pdf_edge_case(wl, 128)
    bits = _strided_call(mm, wl, oracle, torch, "W7_view", g, V, lens, "mm_wave_kernel<2,4>", "wave")
    g0, t0, _ = run_case(mm, wl, oracle, "W2_P128", [g] * len(lens), V, lens, "mm_wave_kernel<2,4>")
    assert np.array_equal(bits[0], g0) and np.array_equal(bits[1], t0)


def _strided_call(mm, wl, oracle, torch, key, g, V, lens, want, family):
    B, n, P = V.shape
    vbuf = torch.full((B, n + 3, P + 5), float("nan"), device="cuda")
    Vd = vbuf[:, 1 : n + 1, 2 : P + 2]
    Vd.copy_(torch.from_numpy(V))
    for b, L in enumerate(lens):  # the frames beyond the lengths: NaN and +inf in turn
        Vd[b, L:] = float("nan")
        Vd[b, L + 1 :: 2] = float("inf")
    gbuf = torch.full((B, n + 2, P + 3), float("nan"), device="cuda")
    out = gbuf[:, 1 : n + 1, 1 : P + 1]
    assert not Vd.is_contiguous() and not out.is_contiguous()
    ld = torch.from_numpy(lens).cuda()
    bf = make_batch(mm, wl, [g] * B, P)
    assert want in bf.kernels(), bf.kernels()
    gam, ttl = bf.pdfposteriors(Vd, ld, out=out)
    torch.cuda.synchronize()
    assert gam.data_ptr() == out.data_ptr()
    edge = gbuf.clone()
    edge[:, 1 : n + 1, 1 : P + 1] = float("nan")
    assert torch.isnan(edge).all()  # (nothing outside the view)
    gam, ttl = gam.cpu().numpy(), ttl.cpu().numpy()
    check_against_oracle(key, gam, ttl, *wc.reference(oracle, graphs, [g] * B, V, lens, key), lens, 1e-3 if family == "lane" else 5e-4)
    return gam, ttl


def test_wave_gamma_modes_on_a_four_pass_instance(mm, wl, oracle, torch):
    """mm_batch_set_gamma_mode on <2,4> (test_gpu_lfmmi.py has it on <.,2>): scale alone, accumulate into the caller's buffer -- the
    frames beyond the lengths untouched --, twice the same bits, and the default again."""
    g, V, lens = wc.pdf_edge_case(wl, 249)
    B = len(lens)
    g_ref, t_ref = wc.reference(oracle, graphs, [g] * B, V, lens, "W2_P249")
    assert np.isfinite(t_ref).all()
    bf = make_batch(mm, wl, [g] * B, g.P)
    assert "mm_wave_kernel<2,4>" in bf.kernels(), bf.kernels()
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    g0, t0 = bf.pdfposteriors(Vt, lt)
    check_gamma(g0.cpu().numpy(), g_ref, lens)
    bf.set_gamma_mode(False, -0.5)
    g1, t1 = bf.pdfposteriors(Vt, lt)
    assert torch.equal(g1, -0.5 * g0) and torch.equal(t1, t0)
    X = torch.from_numpy(np.random.default_rng(3).standard_normal(V.shape).astype(np.float32)).cuda()
    outs = []
    for _ in range(2):
        buf = X.clone()
        bf.set_gamma_mode(True, -1.0)
        g2, t2 = bf.pdfposteriors(Vt, lt, out=buf)
        assert g2.data_ptr() == buf.data_ptr() and torch.equal(t2, t0)
        outs.append(buf.clone())
    assert torch.equal(outs[0], outs[1])
    got, x = outs[0].cpu().numpy(), X.cpu().numpy()
    assert np.abs(got - (x.astype(np.float64) - g_ref)).max() <= 3e-5  # (the bar of test_gamma_mode_accumulates_into_the_callers_buffer)
    for b, L in enumerate(lens):
        assert np.array_equal(got[b, L:], x[b, L:])
    bf.set_gamma_mode(False, 1.0)
    assert torch.equal(bf.pdfposteriors(Vt, lt)[0], g0)


# =============================================== the lane kernel
# ---- L1: the four instances, at both sides of every step of NS
@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("S", wc.LANE_EDGES)
def test_lane_state_count_at_every_step(mm, wl, oracle, torch, S, kind):
    g = wc.lane_dense(wl, S) if kind == "dense" else wc.lane_sparse(wl, S)
    V, lens = wc.lane_case(wl, g, seed=S)
    run_case(mm, wl, oracle, f"L1_{kind}{S}", [g] * len(lens), V, lens, f"mm_lane_kernel<{wc.LANE_NS[S]}>", family="lane")


@pytest.mark.parametrize("which", ["dense65", "sparse65", "pdfs65"])
def test_lane_one_more_than_the_form_holds(mm, wl, oracle, torch, which):
    """65 states, or 65 pdfs on 40 states: no lane kernel."""
    g = {"dense65": lambda: wc.lane_dense(wl, 65), "sparse65": lambda: wc.lane_sparse(wl, 65), "pdfs65": lambda: wc.lane_sparse(wl, 40, 65)}[which]()
    assert (g.S, g.P) == {"dense65": (65, 65), "sparse65": (65, 12), "pdfs65": (40, 65)}[which]
    V, lens = wc.lane_case(wl, g, seed=65)
    run_elsewhere(mm, wl, oracle, f"L1_{which}", [g] * len(lens), V, lens, "mm_lane_kernel")


# ---- L2: one utterance per length
@pytest.mark.parametrize("which,want", [("lane16", "mm_lane_kernel<16>"), ("lane64", "mm_lane_kernel<64>")])
def test_lane_every_short_length(mm, wl, oracle, torch, which, want):
    """Lengths 0 .. 18, 24, 25 in one batch -- both parities of the time split, lengths below, at and beyond the MM_LANE_D = 8 frames
    the emissions and the partner rows are requested ahead, and beyond twice that -- on the identity map and on a many-to-one map;
    and one call without lengths."""
    g = wc.lane_dense(wl, 16) if which == "lane16" else wc.lane_sparse(wl, 64)
    V, lens = wc.lengths_case(wl, g, wc.LANE_LENS, 70)
    run_case(mm, wl, oracle, ("lengths", which), [g] * len(lens), V, lens, want, family="lane")
    run_case(mm, wl, oracle, ("lengths_none", which), [g] * len(lens), V, None, want, family="lane")


# ---- L3: state maps on exactly 64 pdfs
@pytest.mark.parametrize("name", ["perm64", "many_to_one_64", "empty_last_64"])
def test_lane_maps_on_64_pdfs(mm, wl, oracle, torch, name):
    """P = 64 and a map that is not the identity: the kernel's pdf -> states table has 65 entries, one more than a wave has lanes
    (entry 64 was never staged: pdf 63's loop ran to whatever the LDS held).  Each case runs twice, each time behind a wave-kernel
    batch that leaves other data all over the LDS: the same bits, and the oracle's posteriors."""
    g = getattr(wc, name)(wl)
    V, lens = wc.map64_case(wl, g)
    gw, Vw, lw = wc.pdf_edge_case(wl, 249)
    other = make_batch(mm, wl, [gw] * len(lw), gw.P)
    assert "mm_wave_kernel" in other.kernels()
    runs = []
    for k in range(2):
        other.pdfposteriors(Vw + np.float32(k), lw)
        runs.append(run_case(mm, wl, oracle, f"L3_{name}", [g] * len(lens), V, lens, "mm_lane_kernel<64>", family="lane")[:2])
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    empty = np.setdiff1d(np.arange(64), g.state2pdf)
    assert (runs[0][0][:, :, empty] == 0).all()


# ---- L4: different graphs in one batch
@pytest.mark.parametrize("order", ["up", "down"])
def test_lane_different_graphs_and_maps_in_one_batch(mm, wl, oracle, torch, order):
    """5, 20 and 64 states, the identity and other maps, all on 64 pdfs in one batch; both orders."""
    gs = [wc._memo("l2r5", lambda: wl.l2r_hmm(5)), wc.lane_sparse(wl, 20, 12), wc.many_to_one_64(wl), wc.lane_dense(wl, 64)]
    gs = gs if order == "up" else gs[::-1]
    assert [g.S for g in gs] in ([5, 20, 40, 64], [64, 40, 20, 5])
    lens = np.asarray((21, 20, 21, 9), dtype=np.int32)
    run_case(mm, wl, oracle, f"L4_{order}", gs, wc.emissions(4, 21, 64, 44), lens, "mm_lane_kernel<64>", family="lane")


# ---- L5: the hand-off of marked utterances
def test_lane_marked_utterances_go_to_the_wave_kernel(mm, wl, oracle, torch):
    """redo_case (tests/test_wave_lane_inputs.py: the float64 recursion flushes the one path of utterance 0, whose reference is finite):
    every graph has its wave forms, so the marked utterances run the wave kernel, and kernels() says so."""
    g, V, lens = wc.redo_case(wl)
    _, t_ref = wc.reference(oracle, graphs, [g] * 4, V, lens, "redo")
    assert np.isfinite(t_ref[:2]).all() and np.isneginf(t_ref[2:]).all()
    _, ttl, bf = run_case(mm, wl, oracle, "redo", [g] * 4, V, lens, ["mm_lane_kernel<64>", REDO_TEXT + "mm_wave_kernel<2,2>"], family="lane",
                          absent=("mm_log_kernel",), redo=lambda n: n in (3, 4))
    # utterance 0 alone, twice: both are marked, and both come back finite
    V2, l2 = np.stack([V[0], V[0]]), np.asarray((64, 64), dtype=np.int32)
    run_case(mm, wl, oracle, "redo_twice", [g] * 2, V2, l2, REDO_TEXT + "mm_wave_kernel<2,2>", family="lane", redo=2)


def test_lane_marked_utterances_go_to_the_item_kernel(mm, wl, oracle, torch):
    """The same utterances next to dense_ergodic(64), whose 4161 arcs exceed the wave form: the batch's marked utterances run the
    item kernel.  (A dense ergodic graph by itself cannot be marked with a finite reference: every state reaches every state, so the
    backward vector is flat within the weights' range and overlaps the forward maximum.)"""
    g, V, lens = wc.redo_case(wl)
    d = wc.lane_dense(wl, 64)
    gs = [g, d, g, d, g]
    V5 = np.concatenate([V[:1], wc.emissions(1, 64, 64, 5), V[1:3], V[:1]])
    l5 = np.asarray((64, 64, 64, 63, 64), dtype=np.int32)
    run_case(mm, wl, oracle, "redo_items", gs, V5, l5, ["mm_lane_kernel<64>", REDO_TEXT + "mm_log_kernel<MODE_FB,0,0"], family="lane",
             absent=("mm_wave_kernel",), redo=lambda n: n in (2, 3))


# ---- L6: calling conventions
def test_lane_strided_views_inside_nan(mm, wl, oracle, torch):
    g = wc.many_to_one_64(wl)
    V, lens = wc.map64_case(wl, g)
    bits = _strided_call(mm, wl, oracle, torch, "L6_view", g, V, lens, "mm_lane_kernel<64>", "lane")
    g0, t0, bf = run_case(mm, wl, oracle, "L3_many_to_one_64", [g] * len(lens), V, lens, "mm_lane_kernel<64>", family="lane")
    assert np.array_equal(bits[0], g0) and np.array_equal(bits[1], t0)
    with pytest.raises(mm.MarkovModelsAMDError) as e:  # (no accumulate mode on the lane kernel)
        bf.set_gamma_mode(True, -1.0)
    assert e.value.code == -4
