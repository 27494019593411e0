"""Windowed best paths (mm_viterbiwindow_f32) on the MI355X against the float32 mode of tests/vitwindow_reference.py, and the
consequences the header states: (a) closed from the FSM's own start = viterbi, (b) finality, (c) re-windowing with the carried state
in place, (d) the level of a frame, (e) bit-identical repeats; the outputs that may be NULL, hipGraph capture, the kernel instances,
more pdfs than threads, error codes, and streaming.OnlineViterbi against viterbi and against its host replay.

The bar throughout is bit equality -- path, score, converged, ncommit, mcommit and state_out of every utterance of every case
against the restatement that performs the kernels' float32 operations in their order -- so there is no tolerance to measure.  The
one exception is stated where it is used: the float64 score along a re-windowed path on unrounded inputs, held to the project's
ttl bar."""
import copy
import ctypes as C

import numpy as np
import pytest

import vitwindow_reference as vr
from test_gpu_parity import _with_env
from test_viterbiwindow import BASE_MODES, case_base, on_grid, references

pytestmark = pytest.mark.gpu
STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}
BIGV = {"MM_DEBUG": "1", "MM_BIGV": "1"}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib").lib


def _batch(mm, wl, gs):
    cache = {}
    for g in gs:
        if id(g) not in cache:
            cache[id(g)] = mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))
    return mm.batch(*[cache[id(g)] for g in gs])


def _seg(bf, so, b):
    return so[int(bf.state_offsets[b]) : int(bf.state_offsets[b + 1])]


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and not np.isnan(a).any()


def _check(bf, out, refs, what=""):
    """Every utterance, every output, bit for bit."""
    path, score, conv, ncommit, mcommit, so = out
    for b, r in enumerate(refs):
        w = (what, b)
        assert np.array_equal(path[b], r.path), (w, path[b], r.path)
        assert _same_bits(score[b], r.score), (w, score[b], r.score)
        assert conv[b] == r.converged and ncommit[b] == r.ncommit, (w, conv[b], r.converged, ncommit[b], r.ncommit)
        assert _same_bits(mcommit[b], r.mcommit), (w, mcommit[b], r.mcommit)
        assert _same_bits(_seg(bf, so, b), r.state_out), (w, _seg(bf, so, b), r.state_out)


def _run_modes(bf, gs, V, lens, what):
    for closed, commit, cc in BASE_MODES:
        out = bf.viterbiwindow(V, lens, closed=closed, commit=commit, commit_converged=cc, want_state=True)
        _check(bf, out, references(gs, V, lens, closed, commit, cc), f"{what}, commit_converged {cc}, closed {closed}")


@pytest.fixture(scope="module")
def base(wl):
    return case_base(wl, rounded=True)


@pytest.fixture(scope="module")
def unrounded(wl):
    return case_base(wl, rounded=False)


def test_base_case_end_modes_and_commits(mm, wl, torch, base):
    gs, V, lens = base
    N = V.shape[1]
    # non-vacuity, on the reference's own values: the full-length live utterances converge beyond half of their frames
    for closed in (0, 1):
        refs = references(gs, V, lens, np.full(6, closed, dtype=np.int32))
        assert all(refs[b].converged >= N / 2 and refs[b].converged < N for b in (0, 5)), [r.converged for r in refs]
        assert np.isneginf(refs[4].score) and refs[4].converged == 0  # dead at frame 4
    bf = _batch(mm, wl, gs)
    k = bf.kernels("vitwindow")
    assert "mm_vitwindow_fwd_kernel<8,lds>" in k and "mm_vitwindow_trace_kernel<lds>" in k, k
    _run_modes(bf, gs, V, lens, "base case")
    # utterance 4 dies at frame 4: commits ahead of the death keep the prefix's state, commits behind it are -inf
    out = bf.viterbiwindow(V, lens, commit=np.array([0, 0, 0, 0, 2, 0], dtype=np.int32), want_state=True)
    assert np.isneginf(out[1][4]) and (out[0][4] == -1).all() and np.isfinite(out[4][4]) and np.isfinite(_seg(bf, out[5], 4)).any()
    out = bf.viterbiwindow(V, lens, commit=np.array([0, 0, 0, 0, 9, 0], dtype=np.int32), want_state=True)
    assert np.isneginf(out[4][4]) and np.isneginf(_seg(bf, out[5], 4)).all()
    # utterance 3: len = 0 -- the start vector passes through
    assert np.isneginf(out[1][3]) and out[2][3] == 0 and out[3][3] == 0 and out[4][3] == 0
    assert np.array_equal(_seg(bf, out[5], 3), vr.system(gs[3]).pi)


def test_unrounded_inputs(mm, wl, torch, unrounded):
    gs, V, lens = unrounded
    _run_modes(_batch(mm, wl, gs), gs, V, lens, "unrounded")


def test_distinct_graphs(mm, wl, torch):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2, n_init=4), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    B, N = 4, 30
    lens = np.array([30, 22, 30, 17], dtype=np.int32)
    V = (2.0 * np.random.default_rng(21).standard_normal((B, N, 5))).astype(np.float32)
    bf = _batch(mm, wl, gs)
    for closed, commit, cc in ((np.array([0, 1, 1, 0], dtype=np.int32), np.array([10, 0, 40, 3], dtype=np.int32), False),
                               (np.array([1, 0, 0, 1], dtype=np.int32), None, True)):
        out = bf.viterbiwindow(V, lens, closed=closed, commit=commit, commit_converged=cc, want_state=True)
        assert np.isfinite(out[1]).all()
        _check(bf, out, references(gs, V, lens, closed, commit, cc), "distinct graphs")


def test_streamed_and_global_vector_instances(mm, wl, torch, base):
    gs, V, lens = base
    bf = _with_env(STREAMED, lambda: _batch(mm, wl, gs))
    assert "mm_vitwindow_fwd_kernel<0,lds>" in bf.kernels("vitwindow"), bf.kernels("vitwindow")
    _run_modes(bf, gs, V, lens, "streamed instance")
    bf = _with_env(BIGV, lambda: _batch(mm, wl, gs))
    assert "mm_vitwindow_fwd_kernel<8,global>" in bf.kernels("vitwindow"), bf.kernels("vitwindow")
    _run_modes(bf, gs, V, lens, "vectors in global memory")
    bf = _with_env({"MM_DEBUG": "1", "MM_NITEMS": "0", "MM_BIGV": "1"}, lambda: _batch(mm, wl, gs))
    assert "mm_vitwindow_fwd_kernel<0,global>" in bf.kernels("vitwindow"), bf.kernels("vitwindow")
    _run_modes(bf, gs, V, lens, "streamed, vectors in global memory")


def test_vectors_global_by_the_plan(mm, wl, torch):
    """12 500 states: four vectors of 4 bytes per state exceed the 160 KB of a compute unit, the plan itself puts them in global
    memory; the trace kernel's two byte vectors still fit."""
    g = wl.random_fsm(12500, 40, 3.0, seed=3)
    V = np.random.default_rng(4).standard_normal((2, 12, g.P)).astype(np.float32)
    lens = np.array([12, 7], dtype=np.int32)
    bf = _batch(mm, wl, [g, g])
    k = bf.kernels("vitwindow")
    assert "mm_vitwindow_fwd_kernel<" in k and ",global>" in k and "mm_vitwindow_trace_kernel<lds>" in k, k
    for closed, commit, cc in ((np.array([1, 0], dtype=np.int32), np.array([5, 7], dtype=np.int32), False), (np.array([0, 1], dtype=np.int32), None, True)):
        out = bf.viterbiwindow(V, lens, closed=closed, commit=commit, commit_converged=cc, want_state=True)
        assert np.isfinite(out[1]).all()
        _check(bf, out, references([g, g], V, lens, closed, commit, cc), "12500 states")


def test_more_pdfs_than_threads(mm, wl, torch):
    """1100 pdfs against at most 1024 threads: the forward kernel stages a frame's emissions in two parts."""
    g = wl.random_fsm(1200, 1100, 3.0, seed=9)
    V = np.random.default_rng(10).standard_normal((3, 14, g.P)).astype(np.float32)
    lens = np.array([14, 9, 2], dtype=np.int32)
    closed, commit = np.array([0, 1, 0], dtype=np.int32), np.array([7, 9, 1], dtype=np.int32)
    bf = _batch(mm, wl, [g] * 3)
    out = bf.viterbiwindow(V, lens, closed=closed, commit=commit, want_state=True)
    _check(bf, out, references([g] * 3, V, lens, closed, commit), "1200 states, 1100 pdfs")


def test_closed_from_the_start_is_viterbi(mm, wl, torch, base, unrounded):
    """(a), against the entry itself."""
    for gs, V, lens in (base, unrounded):
        bf = _batch(mm, wl, gs)
        path0, score0 = bf.viterbi(V, lens)
        path, score, *_ = bf.viterbiwindow(V, lens, closed=np.ones(6, dtype=np.int32))
        assert np.array_equal(path, path0) and _same_bits(score, score0), (score, score0)


def test_finality(mm, wl, torch, unrounded):
    """(b): a 25-frame open window against the 40-frame windows, on the device."""
    gs, V, lens = unrounded
    bf = _batch(mm, wl, gs)
    short = bf.viterbiwindow(V, np.minimum(lens, 25).astype(np.int32))
    checked = 0
    for closed in (0, 1):
        long = bf.viterbiwindow(V, lens, closed=np.full(6, closed, dtype=np.int32))
        for b in range(6):
            if lens[b] > 25 and np.isfinite(long[1][b]):
                k = int(short[2][b])
                assert 1 <= k <= 25 and np.array_equal(short[0][b, :k], long[0][b, :k]), (b, closed, k)
                checked += 1
    assert checked == 6


def test_rewindowing_on_the_device_with_the_state_in_place(mm, wl, torch, base, unrounded):
    """(c): the second window runs from the first one's state_out, read and written in one buffer.  On the 1/16 grid: the first
    window's path behind c and score - mcommit, bit for bit.  Unrounded: both windows bit for bit against their restatements, and
    the float64 score along the concatenated path within the ttl bar (rtol 1e-5, atol 1e-4) of the single window's."""
    closed = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    c = np.array([12, 20, 0, 0, 2, 39], dtype=np.int32)
    for rounded, (gs, V, lens) in ((True, base), (False, unrounded)):
        B, M, P = V.shape
        bf = _batch(mm, wl, gs)
        Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
        first = bf.viterbiwindow(Vt, lt, closed=closed, commit=c, want_state=True)
        state = first[5]
        first_np = [t.cpu().numpy() for t in first]
        refs1 = references(gs, V, lens, closed, c)
        _check(bf, first_np, refs1, "first window")
        V2 = np.zeros_like(V)
        for b in range(B):
            V2[b, : M - c[b]] = V[b, c[b] :]
        lens2 = (lens - np.minimum(c, lens)).astype(np.int32)
        second = bf.viterbiwindow(torch.from_numpy(V2).cuda(), torch.from_numpy(lens2).cuda(), state=state, closed=closed, want_state=state)
        torch.cuda.synchronize()
        assert second[5] is state
        second_np = [t.cpu().numpy() for t in second]
        _check(bf, second_np, references(gs, V2, lens2, closed, state_in=[r.state_out for r in refs1]), "second window, state in place")
        for b in range(B):
            L, cb = int(lens[b]), int(min(c[b], lens[b]))
            if L == cb or not np.isfinite(first_np[1][b]):
                continue
            if rounded:
                assert np.array_equal(second_np[0][b, : L - cb], first_np[0][b, cb:L]), b
                assert _same_bits(second_np[1][b], first_np[1][b] - first_np[4][b]), (b, second_np[1][b], first_np[1][b], first_np[4][b])
            else:
                whole = np.concatenate([first_np[0][b, :cb], second_np[0][b, : L - cb]])
                s2 = vr.path_score(gs[b], V[b], whole, None, bool(closed[b]))
                s1 = vr.path_score(gs[b], V[b], first_np[0][b, :L], None, bool(closed[b]))
                print(f"utterance {b}: single window {s1:.9g} (float32 {first_np[1][b]:.9g}), re-windowed path {s2:.9g}")
                assert np.isclose(s2, s1, rtol=1e-5, atol=1e-4) and np.isclose(s2, float(first_np[1][b]), rtol=1e-5, atol=1e-4), (b, s1, s2)


def test_the_level_of_a_frame(mm, wl, torch, base):
    """(d): +100 and -150 on one frame: the same paths and convergence points, score moved by the constant (bit for bit: grid)."""
    gs, V, lens = base
    closed, commit, cc = BASE_MODES[0]
    bf = _batch(mm, wl, gs)
    out0 = bf.viterbiwindow(V, lens, closed=closed, commit=commit, commit_converged=cc, want_state=True)
    n = 5
    for shift in (100.0, -150.0):
        Vs = V.copy()
        Vs[:, n] += np.float32(shift)
        out = bf.viterbiwindow(Vs, lens, closed=closed, commit=commit, commit_converged=cc, want_state=True)
        _check(bf, out, references(gs, Vs, lens, closed, commit, cc), f"frame {n} {shift:+g}")
        assert np.array_equal(out[0], out0[0]) and np.array_equal(out[2], out0[2]) and np.array_equal(out[3], out0[3])
        live = np.isfinite(out0[1])
        assert live.sum() == 4 and _same_bits(out[1][live], (out0[1] + np.float32(shift) * (lens > n))[live])


def test_bit_identical_repeats_null_outputs_and_graph_capture(mm, wl, torch, unrounded):
    """(e); path and score do not depend on which optional outputs are asked for; one capture after a first call replays the bits."""
    lib = _lib(mm)
    gs, V, lens = unrounded
    closed, commit, cc = BASE_MODES[1]
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    ct, mt = torch.from_numpy(closed).cuda(), torch.from_numpy(commit).cuda()
    run = lambda: bf.viterbiwindow(Vt, lt, closed=ct, commit=mt, commit_converged=cc, want_state=True)
    out0, out1 = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out0, out1))
    path = torch.full((B, N), 7, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 7.0, device="cuda")
    rc = lib.mm_viterbiwindow_f32(bf._h, Vt.data_ptr(), N * P, P, lt.data_ptr(), N, None, ct.data_ptr(), mt.data_ptr(), 1, None, None, None,
                                  path.data_ptr(), N, score.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(path, out0[0]) and torch.equal(score, out0[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out2 = run()
    for _ in range(2):
        for t in out2:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out0, out2))


def test_capture_before_a_first_call_is_refused(mm, wl, torch):
    """Neither the item forms nor the workspace are made during a capture."""
    g = wl.random_fsm(30, 4, 3.0, seed=5)
    fresh = _batch(mm, wl, [g] * 3)
    V = torch.zeros((3, 20, g.P), device="cuda")
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph0):
        x.add_(1.0)
        with pytest.raises(mm.MarkovModelsAMDError) as ei:
            fresh.viterbiwindow(V, None)
    assert ei.value.code == -1, str(ei.value)
    # ... and the batch works afterwards
    out = fresh.viterbiwindow(V.cpu().numpy(), None, want_state=True)
    _check(fresh, out, references([g] * 3, V.cpu().numpy(), np.full(3, 20)), "after the refused capture")


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    B, N, P = 2, 10, g.P
    V = torch.zeros((B, N, P), device="cuda")
    path = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    score = torch.zeros(B, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, path_ptr=path.data_ptr(), psb=N):
        return lib.mm_viterbiwindow_f32(h, V.data_ptr(), N * P, P, None, N, None, None, None, 0, None, None, None, path_ptr, psb, score.data_ptr(), None, st)

    lb = mm.batch(*([mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(lb._h) == -4
    assert b"tropical" in lib.mm_last_error()
    gl = copy.copy(g)
    gl.w, gl.final_w, gl.init_w = np.exp(g.w), np.exp(g.final_w), np.exp(g.init_w)
    pb = mm.batch(*([mm.compile(wl.to_fsm(mm, gl, "prob", np.float32), mm.statemap(g.state2pdf, g.P))] * B))
    assert call(pb._h) == -4
    tb = _batch(mm, wl, [g] * B)
    assert call(tb._h, path_ptr=None) == -1
    assert call(tb._h, psb=N - 1) == -2
    assert call(tb._h) == 0
    torch.cuda.synchronize()
    for b in (lb, pb):
        with pytest.raises(mm.MarkovModelsAMDError):
            b.kernels("vitwindow")
        with pytest.raises(mm.MarkovModelsAMDError):
            b.viterbiwindow(V, None)


def _chunks(lens, n0, ch, torch):
    return torch.clamp(lens - n0, 0, ch).to(torch.int32)


def test_online_viterbi_with_room_for_every_frame(mm, wl, torch, base):
    """Chunks of 7, max_pending = N, per-utterance lens (0 among them): the concatenated states are viterbi's path, the score
    finish returns is its score exactly (grid), nothing was forced."""
    gs, V, lens = base
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    path0, score0 = bf.viterbi(V, lens)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    dec = mm.OnlineViterbi(bf, N)
    got = [[] for _ in range(B)]
    for n0 in range(0, N + 2, 7):
        ch = min(7, N + 2 - n0)
        Vc = torch.zeros((B, ch, P), device="cuda")
        Vc[:, : max(0, min(ch, N - n0))] = Vt[:, n0 : n0 + ch]
        states, count = dec.push(Vc, _chunks(lt, n0, ch, torch))
        states, count = states.cpu().numpy(), count.cpu().numpy()
        assert states.shape == (B, N + ch)
        for b in range(B):
            assert (states[b, count[b] :] == -1).all()
            got[b].append(states[b, : count[b]])
    assert int(dec.nforced.sum()) == 0
    states, count, total = dec.finish(as_numpy=True)
    for b in range(B):
        whole = np.concatenate(got[b] + [states[b, : count[b]]])
        assert whole.size == lens[b] and np.array_equal(whole, path0[b, : lens[b]]), b
        assert _same_bits(np.float32(total[b]), score0[b]) and total[b] == np.float64(score0[b]), (b, total[b], score0[b])
    assert int(dec.npending.sum()) == 0 and float(dec.score.abs().sum()) == 0


def test_online_viterbi_forced_commits_and_a_masked_finish(mm, wl, torch, base):
    """max_pending = 4: every frame is emitted once, some before they were final; utterance 1 (33 frames) is finished alone while
    the others go on.  States, counts, score and nforced equal the host replay of the policy, bit for bit."""
    gs, V, lens = base
    B, N, P = V.shape
    bf = _batch(mm, wl, gs)
    Vt, lt = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    dec = mm.OnlineViterbi(bf, 4)
    starts = list(range(0, N, 7))
    chunk_lens = [[int(min(7, max(0, lens[b] - n0))) for n0 in starts] for b in range(B)]
    replay = [vr.replay_online(gs[b], V[b], chunk_lens[b], 4) for b in range(B)]
    emitted = np.zeros(B, dtype=np.int64)
    for k, n0 in enumerate(starts):
        ch = min(7, N - n0)
        states, count = dec.push(Vt[:, n0 : n0 + ch], _chunks(lt, n0, ch, torch))
        states, count = states.cpu().numpy(), count.cpu().numpy()
        for b in range(B):
            want = replay[b][0][k] if not (b == 1 and n0 >= 35) else np.zeros(0, dtype=np.int32)
            assert count[b] == want.size and np.array_equal(states[b, : count[b]], want) and (states[b, count[b] :] == -1).all(), (b, k)
            emitted[b] += count[b]
        if n0 == 28:  # utterance 1 has ended (33 frames pushed): finished alone
            mask = np.arange(B) == 1
            st, cnt, total = dec.finish(mask, as_numpy=True)
            assert (cnt[~mask] == 0).all() and np.isneginf(total[~mask]).all()
            assert np.array_equal(st[1, : cnt[1]], replay[1][0][-1]) and total[1] == replay[1][3], (total[1], replay[1][3])
            emitted[1] += cnt[1]
    nforced = dec.nforced.cpu().numpy().copy()
    score = dec.score.cpu().numpy().copy()
    st, cnt, total = dec.finish(np.arange(B) != 1, as_numpy=True)
    for b in range(B):
        if b == 1:
            continue
        assert np.array_equal(st[b, : cnt[b]], replay[b][0][-1]), b
        assert nforced[b] == replay[b][2] and score[b] == replay[b][1], (b, nforced[b], replay[b][2], score[b], replay[b][1])
        assert total[b] == replay[b][3] or (np.isneginf(total[b]) and np.isneginf(replay[b][3])), (b, total[b], replay[b][3])
        emitted[b] += cnt[b]
    assert (emitted == lens).all() and (nforced > 0).any() and max(r[2] for r in replay) > 0
