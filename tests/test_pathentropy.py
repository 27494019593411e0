"""Posterior path entropy and its gradient (mm_pathentropy_f32) without a GPU: the bindings of the new entry, the float64 reference
helper against path enumeration, against central differences and against the identity that builds H from the posteriors, the
properties the definition implies, and the conditions the GPU tests' inputs must meet."""
import json
import math
import os
import re

import numpy as np

import arc_reference as ar
import entropy_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_bound(mm):
    """The library exports the entry (it loads without a GPU), the Python mirror binds it, the host interface is there."""
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert "mm_pathentropy_f32" in mm.SYMBOLS
    assert lib.mm_pathentropy_f32.argtypes is not None and len(lib.mm_pathentropy_f32.argtypes) == 14
    assert callable(mm.pathentropy) and callable(mm.entropy.path_entropy) and callable(mm.entropy.conditional_entropy_loss)
    assert callable(mm.path_entropy) and callable(mm.conditional_entropy_loss)
    assert hasattr(mm.BatchedFSM, "pathentropy")
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_pathentropy_f32(" in hdr and "#define MM_ABI_VERSION 4 " in hdr
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_pathentropy_f32, LIB\)", src) and re.search(r"function pathentropy\(", src)


def _shared_pdf(wl):
    """Four states on two pdfs: states that share a pdf."""
    g = wl.random_fsm(4, 2, mean_deg=2.5, seed=11)
    assert len(set(g.state2pdf)) < g.S
    return g


def _tiny_cases(wl):
    rng = np.random.default_rng(21)
    out = []
    g = wl.l2r_hmm(3)
    out.append(("l2r3 zero emissions", g, np.zeros((5, g.P)), 5, 5))
    out.append(("l2r3 short", g, rng.standard_normal((6, g.P)), 4, 6))
    g = wl.random_fsm(6, 3, mean_deg=2.0, seed=4)
    V = rng.standard_normal((4, g.P))
    V[1, 0] = -np.inf  # a frame with a -inf entry
    out.append(("rand6 -inf entry", g, V, 4, 4))
    out.append(("rand6 one frame", g, rng.standard_normal((4, g.P)), 1, 4))
    g = _shared_pdf(wl)
    out.append(("two states per pdf", g, rng.standard_normal((5, g.P)), 5, 5))
    V = rng.standard_normal((4, g.P))
    V[2, :] = -np.inf  # no accepting path
    out.append(("no path", g, V, 4, 4))
    return out


def test_reference_against_path_enumeration(mm, wl, oracle):
    o, oc = oracle
    seen_no_path = False
    for name, g, V, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        H, grad, gamma, z, mean = er.reference(o, oc, g, f, V, L, N, want_mean=True)
        H_e, grad_e, gamma_e, z_e = er.enumerate_paths(g, f, V, L, N)
        if not np.isfinite(z_e):
            seen_no_path = True
            assert np.isneginf(z) and H == 0 and (grad == 0).all() and (gamma == 0).all(), name
            continue
        assert np.isclose(z, z_e, rtol=1e-10, atol=1e-10), name
        assert abs(H - H_e) <= 1e-10, (name, H, H_e)
        assert np.abs(grad - grad_e).max() <= 1e-10, (name, np.abs(grad - grad_e).max())
        assert np.abs(gamma - gamma_e).max() <= 1e-10, name
        assert (grad[L:] == 0).all() and (gamma[L:] == 0).all(), name
        # the chain rule of entropy: the bracket Hf + Hb - ln q - H has posterior mean zero at every frame (nothing is taken out
        # of the float64 reference's gradient)
        assert mean <= 1e-10, (name, mean)
        assert np.abs(grad.sum(axis=1)).max() <= 1e-10, name
        if name == "l2r3 zero emissions":  # six paths of equal weight
            assert abs(H - math.log(6)) <= 1e-10, H
    assert seen_no_path


def test_reference_float32_mode_agrees(mm, wl, oracle):
    """The float32 mode of the reference is the same recursion: on tiny graphs it misses float64 by float32 rounding only."""
    o, oc = oracle
    for name, g, V, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        ref = er.reference(o, oc, g, f, V, L, N)
        r32 = er.reference(o, oc, g, f, V, L, N, dtype=np.float32)
        if not np.isfinite(ref[3]):
            continue
        assert abs(r32[0] - ref[0]) <= 1e-5 * max(1.0, ref[0]), name
        assert np.abs(r32[1] - ref[1]).max() <= 1e-5 * max(np.abs(ref[1]).max(), 1.0), name


def test_reference_gradient_against_central_differences(mm, wl, oracle):
    """grad = d H / d V (eps = 1e-6; the rounding of an entropy of a few nats over eps is 1e-9)."""
    o, oc = oracle
    eps = 1e-6
    for name, g, V, L, N in _tiny_cases(wl):
        f = wl.to_fsm(mm, g, dtype=np.float64)
        H, grad, gamma, z = er.reference(o, oc, g, f, V, L, N)
        if not np.isfinite(z):
            continue
        for n in range(L):
            for p in range(g.P):
                if not np.isfinite(V[n, p]):
                    assert grad[n, p] == 0
                    continue
                d = []
                for sgn in (1.0, -1.0):
                    V2 = V.copy()
                    V2[n, p] += sgn * eps
                    d.append(er.reference(o, oc, g, f, V2, L, N)[0])
                assert abs((d[0] - d[1]) / (2 * eps) - grad[n, p]) <= 1e-7, (name, n, p)


def test_entropy_from_the_posteriors(mm, wl, oracle):
    """H = log Z - E[ln w(path)] = log Z - sum gamma V - sum (arc counts) ln T_hat - sum (initial counts) ln alpha_hat: the value
    as pdfposteriors and arcposteriors would give it, a difference of large numbers the recursion never forms."""
    o, oc = oracle
    g = wl.lfmmi_denominator(300, 40, seed=2)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L = 200, 187
    V = np.random.default_rng(5).standard_normal((N, g.P))
    H, grad, gamma, z = er.reference(o, oc, g, f, V, L, N)
    counts, init, z2 = ar.reference(o, oc, g, f, V, L, N)
    w = ar.fsm_entries(f)[2]
    e_lnw = float(np.sum(gamma[:L] * V[:L])) + float(np.sum(counts * w)) + float(np.sum(init * np.asarray(f.alpha_val, dtype=np.float64)))
    assert np.isclose(z, z2, rtol=1e-12)
    assert H >= 1.0 and abs(H - (z - e_lnw)) <= 1e-9 * max(1.0, abs(z), abs(e_lnw)), (H, z - e_lnw)
    assert np.abs(grad.sum(axis=1)).max() <= 1e-10
    assert np.abs(gamma[:L].sum(axis=1) - 1.0).max() <= 1e-10


def test_single_path_chain(mm, wl, oracle):
    """One path of positive weight: H = 0, grad = 0."""
    import test_gpu_pathentropy as tg

    o, oc = oracle
    gs, V, lens, _ = tg.case_single_path(wl)
    f = wl.to_fsm(mm, gs[0], dtype=np.float64)
    H, grad, gamma, z = er.reference(o, oc, gs[0], f, V[0].astype(np.float64), int(lens[0]), V.shape[1])
    assert np.isfinite(z) and abs(H) <= 1e-12 and np.abs(grad).max() <= 1e-12
    assert np.abs(gamma.sum(axis=1) - 1.0).max() <= 1e-12 and (gamma.max(axis=1) > 1 - 1e-12).all()


def test_invariance_under_per_frame_shifts(mm, wl, oracle):
    o, oc = oracle
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L = 30, 25
    rng = np.random.default_rng(0)
    V = rng.standard_normal((N, g.P))
    ref = er.reference(o, oc, g, f, V, L, N)
    c = 100.0 * rng.standard_normal((N, 1))
    sh = er.reference(o, oc, g, f, V + c, L, N)
    assert ref[0] >= 1.0 and abs(sh[0] - ref[0]) <= 1e-9 * ref[0]
    assert np.abs(sh[1] - ref[1]).max() <= 1e-9 * np.abs(ref[1]).max()
    assert abs(sh[3] - ref[3] - c[:L].sum()) <= 1e-9 * abs(sh[3])


def test_float32_mode_within_the_bars(mm, wl, oracle):
    """The reference's float32 mode -- the recursion as the kernels run it, in NumPy -- passes the bars the device has to pass."""
    o, oc = oracle
    g = wl.lfmmi_denominator(300, 40, seed=2)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, L = 200, 187
    V = np.random.default_rng(5).standard_normal((N, g.P)).astype(np.float32).astype(np.float64)
    ref = er.reference(o, oc, g, f, V, L, N)
    H32, grad32, _, z32 = er.reference(o, oc, g, f, V, L, N, dtype=np.float32)
    assert er.H_ABS_PER_FRAME > 0 and 0 < er.GRAD_ABS_A <= 1e-4
    er.check(H32, grad32, z32, ref, L, label="float32 mode, lfmmi_denominator(300, 40), N = 200")


def test_gpu_inputs_test_something(mm, wl, oracle):
    """The conditions of the GPU tests' inputs, from the reference alone: every checked utterance of 20 frames or more that has a
    path carries at least a nat of entropy and a gradient (the small inputs here; the long ones assert it when they run)."""
    import test_gpu_pathentropy as tg

    o, oc = oracle
    seen = []
    for name, (gs, V, lens, idx) in (("rand40", tg.case_random40(wl)), ("distinct", tg.case_distinct(wl))):
        for b in (range(len(gs)) if idx is None else idx):
            ref = er.reference(o, oc, gs[b], wl.to_fsm(mm, gs[b]), V[b].astype(np.float64), int(lens[b]), V.shape[1])
            er.assert_inputs_test_something(ref, int(lens[b]))
            if name == "rand40":
                seen.append(ref[0])
    # (27.2 nats with the three -inf entries of utterance 0, 19.6; the single frame of utterance 2 has one initial state to choose
    # from; then the two utterances without a path)
    assert abs(seen[0] - 27.2) < 0.1 and abs(seen[1] - 19.6) < 0.1 and abs(seen[2]) < 1e-12 and seen[3] == 0 and seen[4] == 0, seen


def test_recorded_floor_covers_every_gpu_input(mm, wl):
    """The long inputs of the GPU tests (config 3, both WSJ graphs, 12 500 states) take a minute of reference on the CPU, so their
    conditions are asserted from the record tools/measure_entropy_floor.py left of that very run (profiles/pathentropy_floor.json):
    the record has a row for every checked utterance with a path of every input builder, with the builder's own length, and every
    such utterance of 20 frames or more carries at least a nat of entropy and a gradient.  The bars' constants are its worst rows."""
    import test_gpu_pathentropy as tg

    rec = json.load(open(os.path.join(ROOT, "profiles", "pathentropy_floor.json")))
    rows = {(r["case"], r["utterance"]): r for r in rec["rows"]}
    no_path = {("random40", 3), ("random40", 4)}
    cases = [("random40", tg.case_random40(wl)), ("four distinct graphs", tg.case_distinct(wl)), ("config3 T=1500 randn", tg.case_config3(wl, False)),
             ("config3 T=500 log_softmax(10x)", tg.case_config3(wl, True)), ("wsj den T=700", tg.case_wsj(wl, "den_fsm_wsj")),
             ("wsj num T=700", tg.case_wsj(wl, "num_fsm_wsj")), ("12500 states", tg.case_bigv(wl))]
    seen = 0
    for name, (gs, V, lens, idx) in cases:
        for b in (range(len(gs)) if idx is None else idx):
            if (name, b) in no_path:
                assert (name, b) not in rows
                continue
            r = rows[(name, b)]
            assert r["len"] == int(lens[b]), (name, b)
            if r["len"] >= 20:
                assert r["H"] >= 1.0 and r["G"] > 0, (name, b, r)
            seen += 1
    assert seen == len(rows) == 19
    assert abs(max(r["H_err_per_frame"] for r in rows.values()) - er.H_F32_FLOOR) <= 0.01 * er.H_F32_FLOOR
    assert abs(max(r["grad_err_over_G"] for r in rows.values()) - er.GRAD_F32_FLOOR) <= 0.01 * er.GRAD_F32_FLOOR
