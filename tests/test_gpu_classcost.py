"""Expected arc-class cost and its gradient (mm_classcost_f32) on the MI355X against the float64 reference of
tests/classcost_reference.py: risk, grad and ttl by classcost_reference.check, gamma by check_gamma of test_gpu_parity.  Every
instance and row path, the class cap, the identities with the expected cost, the pdf and the arc-class posteriors of the same
batch, rows beyond the length, and the properties of the entry: bit-identical repeats, optional outputs, strides, hipGraph capture,
relabelling, error codes; the gradients of mbr.expected_class_cost and mpe_loss on a forced alignment.  Every test asserts by name,
from kernels("classcost"), the instance it claims to run, and prints its worst error over the bar.  The shapes are those of
tests/test_gpu_scoredposteriors.py: the smallest at which each instance and row path exists.  A and D are N(0, 1).  The case
functions are what tools/measure_classcost_floor.py measures the float32 floor on (classcost_reference.GRAD_ABS_A comes from there,
not from the kernel)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import arc_reference as ar
import classcost_reference as ccr
import scored_reference as sr
from test_gpu_arcclassposteriors import STREAMED, _batch, _dst_pdf, _lib, _sparse, _src_pdf
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _is(bf, NI, where):
    k = bf.kernels("classcost")
    assert f"mm_classcost_fwd_kernel<{NI},{where}>" in k and f"mm_classcost_bwd_kernel<{NI},{where}>" in k, k
    assert "exceed the cap" not in k and "no classes set" not in k, k
    return k


def _costs(seed, B, N, nc, P):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N, nc)).astype(np.float32), rng.standard_normal((B, N, P)).astype(np.float32)


# ---- the inputs: (name, env, NI, where, gs, clss per utterance, nc, V, lens); A and D come from _costs(seed 40, ...)
def case_random40(mm, wl):
    """A frame with -inf entries, a dead utterance (4), one frame (2) and none (3); three class layouts."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    f = wl.to_fsm(mm, g)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2, N], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((6, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf
    V[4, 4, :] = -np.inf
    layouts = {"entry": (np.arange(f.nnz, dtype=np.int32), f.nnz), "dst": _dst_pdf(g, f), "sparse": _sparse(f)}
    return [(f"random40 {name}", {}, 8, "lds", [g] * 6, [cls] * 6, nc, V, lens) for name, (cls, nc) in layouts.items()]


def case_instance(mm, wl, which):
    if which == "streamed":
        g, N, lens, env, inst = wl.lfmmi_denominator(600, 40, seed=5), 30, np.array([30, 19], dtype=np.int32), STREAMED, (0, "global")
    elif which == "bigv":
        g, N, lens, env, inst = wl.random_fsm(12500, 40, 3.0, seed=3), 40, np.array([40, 29], dtype=np.int32), {}, (8, "global")
    else:
        from test_gpu_itemform import case_wide

        gs, V, _, lens, _ = case_wide(wl, "wide")
        g, N = gs[0], V.shape[1]
        env, inst = (STREAMED, (0, "global")) if which == "wide" else ({}, (8, "lds"))
    f = wl.to_fsm(mm, g)
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    cls, nc = _dst_pdf(g, f)
    return [(which, env, inst[0], inst[1], [g, g], [cls, cls], nc, V, np.asarray(lens, dtype=np.int32)[:2])]


def case_distinct(mm, wl):
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    fs = [wl.to_fsm(mm, g) for g in gs]
    sp = _sparse(fs[2])[0]
    sp[3::5] = 5
    d3 = _dst_pdf(gs[3], fs[3])[0].copy()
    d3[::3] = -1
    clss = [_dst_pdf(gs[0], fs[0])[0], _src_pdf(gs[1], fs[1])[0], sp, d3]
    return [("four distinct graphs", {}, 8, "lds", gs, clss, 6, V, lens)]


def case_cap(mm, wl, cap):
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    f = wl.to_fsm(mm, g)
    cls = ((np.arange(f.nnz) * 7919) % cap).astype(np.int32)
    cls[::9] = -1
    cls[3] = cap - 1
    N = 10
    V = np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)
    return [("C = cap", {}, 8, "lds", [g, g], [cls, cls], cap, V, np.array([10, 6], dtype=np.int32))]


def all_cases(mm, wl, cap):
    """Every input the tests below check against the reference (the floor tool walks them)."""
    out = case_random40(mm, wl)
    for which in ("streamed", "bigv", "wide", "wide resident"):
        out += case_instance(mm, wl, which)
    return out + case_distinct(mm, wl) + case_cap(mm, wl, cap)


def _check(gs, fs, clss, V, A, D, lens, risk, grad, ttl, gamma, what=""):
    """Every utterance against the float64 reference: returns the worst (risk error / bar, gradient error / (a G_b))."""
    N = V.shape[1]
    wr, wg, alive, gref = 0.0, 0.0, [], np.zeros(V.shape)
    for b in range(len(gs)):
        L = int(lens[b])
        Ab, Db = A[b].astype(np.float64), None if D is None else D[b].astype(np.float64)
        ref = ccr.reference(gs[b], fs[b], clss[b], V[b].astype(np.float64), Ab, Db, L, N)
        er, eg = ccr.check(risk[b], grad[b], ttl[b], ref, Ab, Db, L)
        print(f"{what} utterance {b}: len {L}, log Z {ref[3]:.6g}, risk {ref[0]:.6g}, risk error / bar {er:.3g}, "
              f"worst grad error / G_b {eg:.3g} (a = {ccr.GRAD_ABS_A:.3g})")
        wr, wg = max(wr, er), max(wg, eg / ccr.GRAD_ABS_A)
        gref[b] = ref[2]
        if np.isfinite(ref[3]):
            alive.append(b)
        else:
            assert (gamma[b] == 0).all()
    if alive:
        w = check_gamma(gamma[alive], gref[alive], [int(lens[b]) for b in alive])
        print(f"{what}: worst gamma error / bar {w:.3g}")
    assert not np.isnan(risk).any() and not np.isnan(grad).any() and not np.isnan(gamma).any() and not np.isnan(ttl).any()
    return wr, wg


def _run_case(mm, wl, case, with_d=(True, False)):
    name, env, NI, where, gs, clss, nc, V, lens = case

    def run():
        fs, bf = _batch(mm, wl, gs)
        shared = all(g is gs[0] for g in gs)
        assert bf.set_arc_classes(clss[0] if shared else clss, nc) == nc
        _is(bf, NI, where)
        A, D = _costs(40, len(gs), V.shape[1], nc, V.shape[2])
        out = None
        for d in with_d:
            risk, grad, ttl, gamma = bf.classcost(V, A, lens, D=D if d else None, want_gamma=True)
            assert grad.shape == V.shape and gamma.shape == V.shape and risk.shape == (len(gs),)
            _check(gs, fs, clss, V, A, D if d else None, lens, risk, grad, ttl, gamma, f"{name}, D {'given' if d else 'NULL'}")
            out = out or (risk, grad, ttl, gamma)
        return bf, out

    return _with_env(env, run)


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_random_graph_lengths_no_path_one_frame_and_none(mm, wl, torch, layout):
    """<8,lds> on random_fsm(40, 6, 3.0, seed=1), N = 30, lens [30, 25, 1, 0, 28, 30]: one class per entry, the destination's pdf,
    a sparse layout with an empty class; with D and with D NULL."""
    _, (risk, grad, ttl, gamma) = _run_case(mm, wl, case_random40(mm, wl)[layout])
    for b in (3, 4):
        assert risk[b] == 0 and (grad[b] == 0).all() and (gamma[b] == 0).all() and np.isneginf(ttl[b])
    assert np.isfinite(ttl[2]) and (grad[2, 1:] == 0).all()


@pytest.mark.parametrize("which", ["streamed", "bigv", "wide", "wide resident"])
def test_instances(mm, wl, torch, which):
    """<0,global> on the denominator graph and on rows of hundreds of arcs (long streamed rows), <8,global> on a graph whose
    vectors do not fit the LDS, <8,lds> with its long rows streamed beside the class plane.  B = 2 each."""
    _run_case(mm, wl, case_instance(mm, wl, which)[0])


def test_distinct_graphs_with_their_own_classes(mm, wl, torch):
    _run_case(mm, wl, case_distinct(mm, wl)[0])


def test_csr_layout_with_scrambled_entries(mm, wl, torch):
    """An FSM handed over as CSR(T_hat) with the entries of every row in a scrambled order: the classes follow the caller's entry
    order into both class planes.  Through the C ABI."""
    lib = _lib(mm)
    g = wl.random_fsm(50, 4, 3.0, seed=9)
    f = wl.to_fsm(mm, g)
    i, j, w = ar.fsm_entries(f)
    order = np.lexsort((np.random.default_rng(1).random(i.size), i))
    S1 = f.colptr.size - 1
    ptr = np.zeros(S1 + 1, dtype=np.int64)
    np.add.at(ptr, i + 1, 1)
    ptr = np.cumsum(ptr)
    idx = np.ascontiguousarray(j[order], dtype=np.int64)
    val = np.ascontiguousarray(w[order], dtype=np.float32)
    aidx = np.ascontiguousarray(f.alpha_idx, dtype=np.int64)
    aval = np.ascontiguousarray(f.alpha_val, dtype=np.float32)
    s2p = np.ascontiguousarray(list(g.state2pdf) + [g.P], dtype=np.int32)
    h, bh = C.c_void_p(), C.c_void_p()
    assert lib.mm_fsm_create(0, S1, i.size, 1, 8, 0, 4, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, aidx.size,
                             aidx.ctypes.data, aval.ctypes.data, s2p.ctypes.data, g.P + 1, C.byref(h)) == 0
    assert lib.mm_batch_create((C.c_void_p * 2)(h, h), 2, C.byref(bh)) == 0
    try:
        nc = 7
        cls_csc = (np.arange(i.size) % (nc + 1) - 1).astype(np.int32)  # in f's CSC order; -1 for every 8th entry
        cls_caller = np.ascontiguousarray(cls_csc[order])
        assert lib.mm_batch_set_arc_classes(bh, cls_caller.ctypes.data, None, nc) == 0, lib.mm_last_error()
        N = 25
        Vn = np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)
        An, Dn = _costs(3, 2, N, nc, g.P)
        V, A, D = torch.from_numpy(Vn).cuda(), torch.from_numpy(An).cuda(), torch.from_numpy(Dn).cuda()
        lens = torch.tensor([25, 19], dtype=torch.int32, device="cuda")
        grad = torch.full((2, N, g.P), -7.0, device="cuda")
        gamma = torch.full((2, N, g.P), -7.0, device="cuda")
        risk, ttl = torch.empty(2, device="cuda"), torch.empty(2, device="cuda")
        rc = lib.mm_classcost_f32(bh, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, A.data_ptr(), *A.stride(),
                                  D.data_ptr(), D.stride(0), D.stride(1), risk.data_ptr(), grad.data_ptr(), gamma.data_ptr(), *grad.stride(),
                                  ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.mm_last_error()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1024)
        assert lib.mm_batch_kernels(bh, 16, buf, 1024) == 0
        k = buf.value.decode()
        assert "mm_classcost_fwd_kernel<8,lds>" in k and "mm_classcost_bwd_kernel<8,lds>" in k, k
        _check([g, g], [f, f], [cls_csc, cls_csc], Vn, An, Dn, np.array([25, 19]), risk.cpu().numpy(), grad.cpu().numpy(), ttl.cpu().numpy(),
               gamma.cpu().numpy(), "scrambled CSR")
    finally:
        lib.mm_batch_destroy(bh)
        lib.mm_fsm_destroy(h)


def test_identities_with_the_other_entries(mm, wl, torch):
    """lfmmi_denominator(600, 40, seed=5), B = 6, N = 120.  The identities hold within the entry's own bars (classcost_reference.check):
    risk by 1e-4 (sum gamma |D| + sum xi |A|) + 1e-6 L max(|A|, |D|), grad by 1e-4 |grad| + a G_b, ttl as the checks compare it,
    sum_p grad(n, p) = 0 and the constant-cost gradient by a G_b resp. a max |a_t|.  The other side of an identity, the masses and G_b
    of its bar come from the expected-cost / posterior entries' outputs, which existed before this entry."""
    g = wl.lfmmi_denominator(600, 40, seed=5)
    B, N, P = 6, 120, g.P
    fs, bf = _batch(mm, wl, [g] * B)
    f = fs[0]
    V = np.random.default_rng(6).standard_normal((B, N, P)).astype(np.float32)
    lens = np.array([120, 100, 90, 120, 7, 64], dtype=np.int32)
    a = ccr.GRAD_ABS_A
    _, Dp = _costs(41, B, N, 1, P)

    def against_expectedcost(got, want, what):
        (r1, g1, t1), (r0, g0, t0, gam0) = got, want
        worst = 0.0
        for b, L in enumerate(lens):
            c = np.abs(Dp[b, :L].astype(np.float64))
            bar = 1e-4 * float(np.sum(gam0[b, :L] * c)) + 1e-6 * L * float(c.max())
            G = float(np.abs(g0[b]).max())
            err = np.abs(g1[b].astype(np.float64) - g0[b])
            assert abs(float(r1[b]) - float(r0[b])) <= bar, (what, b, r1[b], r0[b], bar)
            assert (err <= 1e-4 * np.abs(g0[b]) + a * G).all(), (what, b, err.max(), G)
            worst = max(worst, abs(float(r1[b]) - float(r0[b])) / bar, float((err / (1e-4 * np.abs(g0[b]) + a * G)).max()))
        assert np.allclose(t1, t0, rtol=1e-5, atol=1e-4)
        print(f"{what}: worst difference / bar {worst:.3g}")

    want = bf.expectedcost(V, Dp, lens, want_gamma=True)
    # source-pdf classes, A = D' (class P: the phony self-loop's, which costs nothing whatever A holds), D NULL
    cls, nc = _src_pdf(g, f)
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds")
    A = np.concatenate([Dp, np.full((B, N, 1), 5.0, dtype=np.float32)], axis=2)
    against_expectedcost(bf.classcost(V, A, lens), want, "source-pdf classes, A = D'")
    # A = 0 with D
    against_expectedcost(bf.classcost(V, np.zeros((B, N, nc), dtype=np.float32), lens, D=Dp), want, "A = 0, D = D'")
    # risk = sum gamma D + sum_{t<len} xi A
    cls, nc = _dst_pdf(g, f)
    bf.set_arc_classes(cls, nc)
    A, D = _costs(42, B, N, nc, P)
    risk, grad, ttl = bf.classcost(V, A, lens, D=D)
    xi, _ = bf.arcclassposteriors(V, lens)
    gam, _ = bf.pdfposteriors(V, lens)
    for b, L in enumerate(lens):
        x = xi[b, :, :L].T.astype(np.float64)
        dot = float(np.sum(gam[b, :L].astype(np.float64) * D[b, :L]) + np.sum(x * A[b, :L]))
        mass = float(np.sum(gam[b, :L] * np.abs(D[b, :L])) + np.sum(x * np.abs(A[b, :L])))
        bar = 1e-4 * mass + 1e-6 * L * max(float(np.abs(A[b, :L]).max()), float(np.abs(D[b, :L]).max()))
        # sum_p grad(n, p) = 0 within a G_b: the backward kernel takes the frame's posterior mean out
        G = float(np.abs(grad[b]).max())
        s = np.abs(grad[b].astype(np.float64).sum(axis=1))
        print(f"utterance {b}: risk {risk[b]:.6g} against sum gamma D + sum xi A {dot:.6g} (difference / bar {abs(float(risk[b]) - dot) / bar:.3g}), "
              f"worst |sum_p grad| / (a G_b) {s.max() / (a * G):.3g}")
        assert abs(float(risk[b]) - dot) <= bar
        assert (s <= a * G).all(), (b, s.max(), G)
    # every entry has a class and A[b, t, c] = a_t: every path pays the same
    a_t = np.random.default_rng(43).standard_normal((B, N)).astype(np.float32)
    risk, grad, ttl = bf.classcost(V, np.repeat(a_t[:, :, None], nc, axis=2), lens)
    for b, L in enumerate(lens):
        want_r = float(a_t[b, :L].astype(np.float64).sum())
        bar = 1e-4 * float(np.abs(a_t[b, :L]).sum()) + 1e-6 * L * float(np.abs(a_t[b, :L]).max())
        print(f"utterance {b}: constant class costs, risk {risk[b]:.6g} against {want_r:.6g} (bar {bar:.3g}), max |grad| {np.abs(grad[b]).max():.3g}")
        assert abs(float(risk[b]) - want_r) <= bar
        assert np.abs(grad[b]).max() <= ccr.GRAD_ABS_A * float(np.abs(a_t[b, :L]).max())


def test_rows_beyond_the_length_are_never_read(mm, wl, torch):
    case = case_random40(mm, wl)[1]
    _, _, _, _, gs, clss, nc, V, lens = case
    fs, bf = _batch(mm, wl, gs)
    bf.set_arc_classes(clss[0], nc)
    _is(bf, 8, "lds")
    A, D = _costs(40, len(gs), V.shape[1], nc, V.shape[2])
    for b, L in enumerate(lens):
        A[b, L:] = 0
        D[b, L:] = 0
    clean = bf.classcost(V, A, lens, D=D, want_gamma=True)
    An, Dn = A.copy(), D.copy()
    for b, L in enumerate(lens):
        An[b, L:] = np.nan
        Dn[b, L:] = np.nan
    dirty = bf.classcost(V, An, lens, D=Dn, want_gamma=True)
    for x, y in zip(clean, dirty):
        assert np.isfinite(y[np.isfinite(x)]).all() and not np.isnan(y).any() and (x == y).all()


def test_class_cap(mm, wl, torch):
    """C = cap classes (most of them empty) run and are checked; C = cap + 1 is refused with the cap in the message while the
    arc-class entry still runs."""
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    fs, bf = _batch(mm, wl, [g, g])
    cap = bf.info(classcost=True)["cost_class_cap"]
    print(f"cost_class_cap {cap}")
    floor = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "classcost_floor.json")))
    assert floor["cap"] == cap, "the float32 floor was measured at another class count: rerun tools/measure_classcost_floor.py"
    assert fs[0].nnz < cap <= 65534, cap
    case = case_cap(mm, wl, cap)[0]
    bf, _ = _run_case(mm, wl, case, with_d=(True,))
    assert f"class cap {cap}" in bf.kernels("classcost")
    V, lens, cls = case[7], case[8], case[5][0]
    bf.set_arc_classes(cls, cap + 1)
    assert "exceed the cap" in bf.kernels("classcost")
    with pytest.raises(mm.MarkovModelsAMDError) as e:
        bf.classcost(V, np.zeros((2, V.shape[1], cap + 1), dtype=np.float32), lens)
    assert e.value.code == -4 and str(cap) in str(e.value)
    x2, _ = bf.arcclassposteriors(V, lens)  # (the arc-class entry has no such cap)
    assert x2.shape == (2, cap + 1, V.shape[1])


def test_bit_identical_optional_outputs_strides_capture_and_relabelling(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    fs, bf = _batch(mm, wl, [g] * 6)
    f = fs[0]
    N, B, P = 120, 6, g.P
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((B, N, P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    cls, nc = _dst_pdf(g, f)
    cls = cls.copy()
    cls[::5] = -1
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds")
    An, Dn = _costs(8, B, N, nc, P)
    A, D = torch.from_numpy(An).cuda(), torch.from_numpy(Dn).cuda()
    r0, g0, t0, m0 = bf.classcost(V, A, lens, D=D, want_gamma=True)
    r1, g1, t1, m1 = bf.classcost(V, A, lens, D=D, want_gamma=True)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and torch.equal(g0, g1) and torch.equal(t0, t1) and torch.equal(m0, m1)
    assert float(g0.abs().sum()) > 0 and float(m0.sum()) > 0
    # optional outputs: gamma and ttl NULL change no bit of the rest
    lib = _lib(mm)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r2, g2 = torch.zeros(B, device="cuda"), torch.full((B, N, P), -7.0, device="cuda")
    rc = lib.mm_classcost_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, A.data_ptr(), *A.stride(), D.data_ptr(), D.stride(0),
                              D.stride(1), r2.data_ptr(), g2.data_ptr(), None, *g2.stride(), None, st())
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(r2, r0) and torch.equal(g2, g0)
    # non-contiguous strides: A with the frames contiguous per class, grad with the frames contiguous per pdf
    At = A.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert At.stride() == (nc * N, 1, N)
    g3 = torch.full((B, P, N), -7.0, device="cuda").permute(0, 2, 1)
    r3 = torch.zeros(B, device="cuda")
    rc = lib.mm_classcost_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, At.data_ptr(), *At.stride(), D.data_ptr(), D.stride(0),
                              D.stride(1), r3.data_ptr(), g3.data_ptr(), None, *g3.stride(), None, st())
    assert rc == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(r3, r0) and torch.equal(g3, g0)
    r4, g4, t4 = bf.classcost(V, At, lens, D=D)
    assert torch.equal(r4, r0) and torch.equal(g4, g0) and torch.equal(t4, t0)
    # hipGraph capture; a replay follows costs overwritten in place
    Ac = A.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc_, gc, tc = bf.classcost(V, Ac, lens, D=D)
    for _ in range(2):
        rc_.zero_()
        gc.zero_()
        tc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rc_, r0) and torch.equal(gc, g0) and torch.equal(tc, t0)
    A2 = torch.from_numpy(_costs(9, B, N, nc, P)[0]).cuda()
    r5, g5, t5 = bf.classcost(V, A2, lens, D=D)
    Ac.copy_(A2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rc_, r5) and torch.equal(gc, g5) and torch.equal(tc, t5) and not torch.equal(rc_, r0)
    # relabelling: class c becomes perm[c], the columns of A move with the labels; risk and grad stay bit for bit
    perm = np.random.default_rng(1).permutation(nc).astype(np.int32)
    pt = torch.from_numpy(perm.astype(np.int64)).cuda()
    bf.set_arc_classes(np.where(cls >= 0, perm[np.maximum(cls, 0)], -1).astype(np.int32), nc)
    Ap = torch.empty_like(A)
    Ap[:, :, pt] = A
    r6, g6, t6 = bf.classcost(V, Ap, lens, D=D)
    torch.cuda.synchronize()
    assert torch.equal(r6, r0) and torch.equal(g6, g0) and torch.equal(t6, t0)


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N, B, P = 10, 2, g.P
    V = torch.zeros((B, N, P), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = wl.to_fsm(mm, g)
    sm = mm.statemap(g.state2pdf, g.P)
    lb = mm.batch(*([mm.compile(f, sm)] * 2))
    nc = 3
    A = torch.ones((B, N, nc), device="cuda")
    gr = torch.zeros((B, N, P), device="cuda")
    r, t = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")

    def call(bf, ap=A.data_ptr(), as_=(N * nc, nc, 1), rp=r.data_ptr(), gp=gr.data_ptr(), gs=(N * P, P, 1), stream=st):
        return lib.mm_classcost_f32(bf._h, V.data_ptr(), N * P, P, None, N, ap, *as_, None, 0, 0, rp, gp, None, *gs, t.data_ptr(), stream)

    assert call(lb) == -1 and b"no classes set" in lib.mm_last_error()
    assert lb.kernels("classcost").endswith("no classes set")
    cls = (np.arange(f.nnz) % nc).astype(np.int32)
    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), sm)] * 2))
    assert call(tb) == -4 and b"log" in lib.mm_last_error()
    cap = C.c_int64()
    assert lib.mm_batch_cost_class_cap(tb._h, C.byref(cap)) == -4 and lib.mm_batch_cost_class_cap(lb._h, None) == -1
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("classcost")
    assert lib.mm_batch_set_arc_classes(lb._h, cls.ctypes.data, None, nc) == 0
    assert call(lb, ap=None) == -1 and b"NULL" in lib.mm_last_error()
    assert call(lb, rp=None) == -1 and call(lb, gp=None) == -1
    assert call(lb, as_=(N * nc, nc - 1, 1)) == -2 and b"a strides" in lib.mm_last_error()  # frames overlap
    assert call(lb, gs=(N * P, P - 1, 1)) == -2 and b"g strides" in lib.mm_last_error()
    with pytest.raises(mm.DimensionMismatch):
        lb.classcost(V, torch.zeros((B, N, nc + 1), device="cuda"))
    with pytest.raises(mm.DimensionMismatch):
        lb.classcost(V, A, D=torch.zeros((B, N, P + 1), device="cuda"))
    with pytest.raises(TypeError):
        lb.classcost(V, torch.zeros((B, N, nc), device="cuda", dtype=torch.float64))
    # a first call under capture is refused: the planes are not on the device yet.  (An expected-cost call first: it puts the item
    # forms on the device and sizes the very workspace, so the refusal is the class planes' and no other.)
    D0 = torch.zeros((B, N, P), device="cuda")
    lb.expectedcost(V, D0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(lb, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"class planes" in lib.mm_last_error() and b"mm_classcost_f32" in lib.mm_last_error(), (rc, lib.mm_last_error())
    assert call(lb) == 0, lib.mm_last_error()
    torch.cuda.synchronize()
    # every entry has a class and costs 1: every path pays its N transitions, and the gradient vanishes
    assert np.allclose(r.cpu().numpy(), N, rtol=1e-5) and float(gr.abs().max()) <= ccr.GRAD_ABS_A


def test_autograd_expected_class_cost(mm, wl, torch):
    """Gradients in V, A and D of mbr.expected_class_cost against the float64 reference: d risk / d V = grad by the gradient's bar,
    d risk / d D = gamma by check_gamma, d risk / d A = xi (the reference's: the derivative of its risk, which is linear in A) by the
    arc-class bar 1e-4 xi + 1e-6, exact zeros for t >= len and for an utterance without a path."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    B, N, P = 3, 24, g.P
    fs, bf = _batch(mm, wl, [g] * B)
    f = fs[0]
    cls, nc = mm.loop_exit_classes(f, g.state2pdf, g.P)
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds")
    Vn = np.random.default_rng(12).standard_normal((B, N, P)).astype(np.float32)
    Vn[2, 5, :] = -np.inf  # no path
    An, Dn = _costs(13, B, N, nc, P)
    lens_n = np.array([24, 17, 24], dtype=np.int32)
    lens = torch.from_numpy(lens_n).cuda()
    V = torch.from_numpy(Vn).cuda().requires_grad_(True)
    A = torch.from_numpy(An).cuda().requires_grad_(True)
    D = torch.from_numpy(Dn).cuda().requires_grad_(True)
    gout = torch.tensor([1.0, -2.0, 3.0], device="cuda")
    total, risk, ttl = mm.expected_class_cost(V, A, bf, lens, D=D)
    assert torch.isneginf(ttl[2]) and float(risk[2].detach()) == 0
    (risk * gout).sum().backward()
    gV, gA, gD = V.grad.cpu().numpy(), A.grad.cpu().numpy(), D.grad.cpu().numpy()
    assert not np.isnan(gV).any() and not np.isnan(gA).any() and not np.isnan(gD).any()
    assert (gV[2] == 0).all() and (gA[2] == 0).all() and (gD[2] == 0).all() and (gA[1, 17:] == 0).all()
    for b in range(2):
        L, s = int(lens_n[b]), float(gout[b])
        ref = ccr.reference(g, f, cls, Vn[b].astype(np.float64), An[b].astype(np.float64), Dn[b].astype(np.float64), L, N)
        ccr.check(float(risk[b].detach()), gV[b] / s, float(ttl[b]), ref, An[b], Dn[b], L)
        check_gamma((gD[b] / s)[None], ref[2][None], [L])
        # d risk / d A: xi of the float64 reference of the arc-class posteriors (no scores)
        _, xr, _, _ = sr.reference(g, f, cls, nc, None, Vn[b].astype(np.float64), L, N)
        xr = xr.T.copy()
        xr[L:] = 0
        err = np.abs(gA[b] / s - xr)
        print(f"utterance {b}: d risk / d A against xi, worst error / bar {(err / (1e-4 * xr + 1e-6)).max():.3g}")
        assert (err <= 1e-4 * xr + 1e-6).all()
    # only what is needed: V alone asks for neither gamma nor xi
    V2 = torch.from_numpy(Vn).cuda().requires_grad_(True)
    total2, risk2, _ = mm.expected_class_cost(V2, A.detach(), bf, lens, D=D.detach())
    total2.backward()
    assert torch.equal(risk2, risk.detach()) and torch.equal(V2.grad[0], V.grad[0]) and torch.equal(V2.grad[1] * -2.0, V.grad[1])


def test_mpe_loss_on_a_forced_alignment(mm, wl, torch):
    """l2r_hmm(5) with loop_exit_classes and emissions that leave one alignment (every other pdf 60 nats below): accuracy[b] is the
    number of transitions whose class equals the reference's.  The reference classes are the alignment's own except at three
    transitions, one entry is < 0 and one lies beyond the length."""
    g = wl.l2r_hmm(5)
    fs, bf = _batch(mm, wl, [g, g])
    f = fs[0]
    cls, nc = mm.loop_exit_classes(f, g.state2pdf, g.P)
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds")
    N = 14
    lens = np.array([14, 12], dtype=np.int32)
    exits = [np.array([2, 4, 7, 8, 13]), np.array([0, 1, 6, 10, 11])]  # the transition at which state s is left
    V = np.full((2, N, g.P), -60.0, dtype=np.float32)
    ref = np.zeros((2, N), dtype=np.int64)
    want = []
    for b in range(2):
        L = int(lens[b])
        state = np.searchsorted(exits[b], np.arange(L))
        V[b, np.arange(L), np.asarray(g.state2pdf)[state]] = 0.0
        true = 2 * np.asarray(g.state2pdf)[state] + np.isin(np.arange(L), exits[b]).astype(np.int64)  # loop: 2 pdf, exit: 2 pdf + 1
        ref[b, :L] = true
        ref[b, 3] = (true[3] + 1) % nc  # a wrong class
        ref[b, 5] = -1                  # no reference: costs nothing
        ref[b, 9] = (true[9] + 2) % nc
        if L < N:
            ref[b, L:] = true[L - 1]    # beyond the length: ignored
        want.append(L - 3)
    Vt = torch.from_numpy(V).cuda().requires_grad_(True)
    loss, acc, ttl = mm.mpe_loss(Vt, ref, bf, torch.from_numpy(lens).cuda())
    print("accuracy", acc.tolist(), "expected", want, "ttl", ttl.tolist())
    assert torch.isfinite(ttl).all()
    assert np.allclose(acc.detach().cpu().numpy(), want, rtol=0, atol=1e-4 * N)
    assert abs(float(loss.detach()) + sum(want)) <= 2e-4 * N
    loss.backward()
    assert torch.isfinite(Vt.grad).all()
