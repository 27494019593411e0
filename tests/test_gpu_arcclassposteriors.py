"""Per-frame arc-class posteriors (mm_arcclassposteriors_f32) on the MI355X against the float64 reference of
tests/arcclass_reference.py, the identities with the arc, pdf and boundary posteriors of the same batch, every instance and
both placements of the term rows, and the properties of the entry: bit-identical repeats, hipGraph capture, relabelling, error
codes.  Every test asserts by name, from kernels("arcclass"), the instance and the term-row placement it claims to run; the
comparisons with the reference print their worst error over the bar of arcclass_reference.check."""
import ctypes as C

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr
from test_gpu_parity import _with_env

pytestmark = pytest.mark.gpu

STREAMED = {"MM_DEBUG": "1", "MM_NITEMS": "0"}  # (test_gpu_itemform.STREAMED: the streamed-only instance at batch creation)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _lib(mm):
    from importlib import import_module

    return import_module(mm.__name__ + "._lib").lib


def _batch(mm, wl, gs):
    """One compiled FSM per distinct graph object: a repeated graph shares its handle (and its class plan)."""
    cache = {}
    fs = [cache.setdefault(id(g), wl.to_fsm(mm, g)) for g in gs]
    cf = {id(g): mm.compile(cache[id(g)], mm.statemap(g.state2pdf, g.P)) for g in gs}
    return fs, mm.batch(*[cf[id(g)] for g in gs])


def _is(bf, NI, where, terms):
    k = bf.kernels("arcclass")
    assert f"mm_log_kernel<MODE_FB,{NI},1>" in k and f"mm_arcclass_kernel<{NI},{where}>" in k, k
    assert k.endswith("terms in LDS" if terms == "lds" else "terms in global memory"), k
    return k


def _dst_pdf(g, f):
    _, j, _ = ar.fsm_entries(f)
    return ar._s2p_full(g)[j].astype(np.int32), g.P + 1


def _src_pdf(g, f):
    i, _, _ = ar.fsm_entries(f)
    return ar._s2p_full(g)[i].astype(np.int32), g.P + 1


def _sparse(f):
    """every 7th entry in class 0, every 11th of the rest in class 2, class 1 empty"""
    cls = np.full(f.nnz, -1, dtype=np.int32)
    cls[::7] = 0
    rest = np.flatnonzero(cls < 0)
    cls[rest[::11]] = 2
    return cls, 3


def _check(oracle, gs, fs, clss, nc, V, lens, xi, ttl, idx=None, what=""):
    o, oc = oracle
    N = V.shape[1]
    worst = 0.0
    for b in (range(len(gs)) if idx is None else idx):
        ref, z, exact = acr.reference(o, oc, gs[b], fs[b], clss[b], nc, V[b].astype(np.float64), int(lens[b]), N)
        w = acr.check(xi[b], ttl[b], ref, z, exact)
        print(f"{what} utterance {b}: len {int(lens[b])}, worst arc-class error / bar {w:.3g}")
        worst = max(worst, w)
    return worst


def _run_shared(mm, wl, oracle, g, B, V, lens, layouts, NI, where, terms, idx=None):
    fs, bf = _batch(mm, wl, [g] * B)
    out = {}
    for name, (cls, nc) in layouts.items():
        assert bf.set_arc_classes(cls, nc) == nc
        _is(bf, NI, where, terms)
        xi, ttl = bf.arcclassposteriors(V, lens)
        assert xi.shape == (B, nc, V.shape[1])
        _check(oracle, [g] * B, fs, [cls] * B, nc, V, lens, xi, ttl, idx, name)
        out[name] = (xi, ttl)
    return fs[0], bf, out


def test_random_graph_lengths_and_no_path(mm, wl, oracle, torch):
    """test_gpu_arcposteriors' inputs: a frame with -inf entries, an utterance of one frame, one of none, one without a path;
    one class per entry, the destination's pdf, a sparse layout with an empty class.  <8,lds>, terms in LDS."""
    g = wl.random_fsm(40, 6, 3.0, seed=1)
    f = wl.to_fsm(mm, g)
    N = 30
    lens = np.array([N, N - 5, 1, 0, N - 2], dtype=np.int32)
    V = np.random.default_rng(0).standard_normal((5, N, g.P)).astype(np.float32)
    V[0, 7, :3] = -np.inf
    V[4, 4, :] = -np.inf
    layouts = {"entry": (np.arange(f.nnz, dtype=np.int32), f.nnz), "dst": _dst_pdf(g, f), "sparse": _sparse(f)}
    _, bf, out = _run_shared(mm, wl, oracle, g, 5, V, lens, layouts, 8, "lds", "lds")
    for xi, ttl in out.values():
        assert np.isneginf(ttl[3]) and np.isneginf(ttl[4]) and (xi[3] == 0).all() and (xi[4] == 0).all()
    xi, _ = out["dst"]
    assert (xi[2, g.P, 1:] == 1).all() and (xi[2, : g.P, 1:] == 0).all()  # behind one frame: the phony loop alone
    assert (out["sparse"][0][:, 1] == 0).all()  # the empty class
    _, t2 = bf.pdfposteriors(V, lens)
    ok = np.isfinite(t2)
    assert np.allclose(out["dst"][1][ok], t2[ok], rtol=1e-5, atol=1e-4)


def test_identities_with_the_other_entries(mm, wl, torch):
    """lfmmi_denominator(600, 40, seed=5), B = 6, N = 120: sum_t xi by class against arcposteriors grouped by class (the count
    bar of arc_reference.check), source-pdf classes against pdfposteriors of the batch on its default path, destination-pdf
    classes against the same gamma one frame on (the bars of arcclass_reference.check)."""
    g = wl.lfmmi_denominator(600, 40, seed=5)
    B, N, P = 6, 120, g.P
    fs, bf = _batch(mm, wl, [g] * B)
    f = fs[0]
    V = np.random.default_rng(6).standard_normal((B, N, P)).astype(np.float32)
    lens = np.array([120, 100, 90, 120, 7, 64], dtype=np.int32)
    counts, _ = bf.arcposteriors(V, lens)
    gamma, tg = bf.pdfposteriors(V, lens)
    gamma = gamma.astype(np.float64).transpose(0, 2, 1)  # [B, P, N]
    worst = {}
    for name, (cls, nc) in {"dst": _dst_pdf(g, f), "src": _src_pdf(g, f), "sparse": _sparse(f)}.items():
        bf.set_arc_classes(cls, nc)
        _is(bf, 8, "lds", "lds")
        xi, ttl = bf.arcclassposteriors(V, lens)
        assert np.allclose(ttl, tg, rtol=1e-5, atol=1e-4)
        xi = xi.astype(np.float64)
        for b in range(B):
            L = int(lens[b])
            by_class = np.zeros(nc)
            np.add.at(by_class, cls[cls >= 0], counts[b, : f.nnz].astype(np.float64)[cls >= 0])
            err, bar = np.abs(xi[b].sum(axis=1) - by_class), 1e-4 * by_class + 1e-6 * L
            worst["counts"] = max(worst.get("counts", 0.0), float((err / bar).max()))
            print(f"{name} utterance {b}: sum over frames against arcposteriors, worst / bar {(err / bar).max():.3g}")
            assert (err <= bar).all(), (name, b, err.max())
            ref = None
            if name == "src":
                ref, got = gamma[b][:, :L], xi[b][:P, :L]
            elif name == "dst":
                ref, got = gamma[b][:, 1:L], xi[b][:P, : L - 1]
            if ref is not None:
                err, bar = np.abs(got - ref), 1e-4 * ref + 1e-6
                fsum = np.abs(got.sum(axis=0) - ref.sum(axis=0))
                w = max(float((err / bar).max()), float(fsum.max() / 1e-4))
                worst[name] = max(worst.get(name, 0.0), w)
                print(f"{name} utterance {b}: against pdfposteriors, worst / bar {w:.3g}")
                assert (err <= bar).all() and (fsum <= 1e-4).all(), (name, b, err.max(), fsum.max())
    print("worst over the bars:", worst)


def _case_instances(wl, which):
    if which == "streamed":
        g = wl.lfmmi_denominator(600, 40, seed=5)
        return g, 30, np.array([30, 19], dtype=np.int32), STREAMED, (0, "global", "lds")
    if which == "bigv":  # (53 608 entries, all with a class: beyond every cap)
        return wl.random_fsm(12500, 40, 3.0, seed=3), 40, np.array([40, 29], dtype=np.int32), {}, (8, "global", "global")
    from test_gpu_itemform import case_wide

    gs, V, _, lens, _ = case_wide(wl, "wide")
    return gs[0], V.shape[1], lens, STREAMED, (0, "global", "lds")


@pytest.mark.parametrize("which", ["streamed", "bigv", "wide"])
def test_instances(mm, wl, oracle, torch, which):
    """<0,global> on the denominator graph and on rows of hundreds of arcs (long streamed rows), <8,global> on a graph whose
    vectors do not fit the LDS; destination-pdf classes (every entry has a class)."""
    g, N, lens, env, (NI, where, terms) = _case_instances(wl, which)
    f = wl.to_fsm(mm, g)
    V = np.random.default_rng(4).standard_normal((2, N, g.P)).astype(np.float32)
    layouts = {"dst": _dst_pdf(g, f)} if which != "streamed" else {"dst": _dst_pdf(g, f), "sparse": _sparse(f)}
    _with_env(env, lambda: _run_shared(mm, wl, oracle, g, 2, V, lens, layouts, NI, where, terms))


def test_wide_rows_resident(mm, wl, oracle, torch):
    """case_wide(wl, "wide") on the default instance: <8,lds> with its long rows streamed."""
    from test_gpu_itemform import case_wide

    gs, V, _, lens, _ = case_wide(wl, "wide")
    f = wl.to_fsm(mm, gs[0])
    _run_shared(mm, wl, oracle, gs[0], 2, V, lens, {"dst": _dst_pdf(gs[0], f)}, 8, "lds", "lds")


@pytest.mark.parametrize("over", [0, 1])
def test_term_row_placement(mm, wl, oracle, torch, over):
    """Exactly cap and cap + 1 classified entries (cap from info()), spread over 5 classes by entry index: terms in LDS, terms in
    global memory.  The cap of lfmmi_denominator(600, 40) (~19 100) exceeds its 9 907 entries: the graph is
    lfmmi_denominator(1200, 40), 19 461 entries against a cap of ~17 950 -- the first of the sizes 1000, 1100, 1200 whose
    entries exceed its cap with some margin."""
    g = wl.lfmmi_denominator(1200, 40)
    fs, bf = _batch(mm, wl, [g, g])
    f = fs[0]
    cap = bf.info()["arcclass_cap"]
    assert 0 < cap + 1 <= f.nnz, (cap, f.nnz)
    M = cap + over
    cls = np.full(f.nnz, -1, dtype=np.int32)
    pick = np.round(np.linspace(0, f.nnz - 1, M)).astype(np.int64)  # M distinct entries over the whole graph
    assert np.unique(pick).size == M
    cls[pick] = pick % 5
    N = 20
    V = np.random.default_rng(8).standard_normal((2, N, g.P)).astype(np.float32)
    lens = np.array([20, 13], dtype=np.int32)
    bf.set_arc_classes(cls, 5)
    assert bf.info() == dict(arcclass_cap=cap, arcclass_max_M=M, arcclass_C=5)
    _is(bf, 8, "lds", "global" if over else "lds")
    xi, ttl = bf.arcclassposteriors(V, lens)
    _check(oracle, [g, g], fs, [cls, cls], 5, V, lens, xi, ttl, None, "cap + 1" if over else "cap")


def test_distinct_graphs_with_their_own_classes(mm, wl, oracle, torch):
    """The four graphs of test_gpu_arcposteriors.test_distinct_graphs_in_their_own_order, a layout of 6 classes each."""
    gs = [wl.random_fsm(60, 5, 3.0, seed=2), wl.l2r_hmm(5), wl.random_fsm(25, 5, 2.0, seed=7), wl.lfmmi_denominator(300, 5, seed=1)]
    N = 40
    V = np.random.default_rng(5).standard_normal((len(gs), N, 5)).astype(np.float32)
    lens = np.array([40, 33, 20, 38], dtype=np.int32)
    fs, bf = _batch(mm, wl, gs)
    sp = _sparse(fs[2])[0]
    sp[3::5] = 5
    d3 = _dst_pdf(gs[3], fs[3])[0].copy()
    d3[::3] = -1
    clss = [_dst_pdf(gs[0], fs[0])[0], _src_pdf(gs[1], fs[1])[0], sp, d3]
    with pytest.raises(mm.MarkovModelsAMDError):
        bf.set_arc_classes(clss[0], 6)  # one array for a batch of several FSMs
    with pytest.raises(mm.DimensionMismatch):
        bf.set_arc_classes([clss[0], clss[1], clss[2], clss[3][:-1]], 6)
    assert bf.set_arc_classes(clss, 6) == 6
    _is(bf, 8, "lds", "lds")
    xi, ttl = bf.arcclassposteriors(V, lens)
    _check(oracle, gs, fs, clss, 6, V, lens, xi, ttl)


def test_csr_layout_with_scrambled_entries(mm, wl, oracle, torch):
    """An FSM handed over as CSR(T_hat) with the entries of every row in a scrambled order (the construction of
    test_gpu_arcposteriors._scrambled_csr_run): the classes follow the caller's entry order.  Through the C ABI, xi laid out
    [B, C, N] by its strides."""
    o, oc = oracle
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
        V = torch.from_numpy(np.random.default_rng(2).standard_normal((2, N, g.P)).astype(np.float32)).cuda()
        lens = torch.tensor([25, 19], dtype=torch.int32, device="cuda")
        xi = torch.full((2, nc, N), -7.0, device="cuda")
        ttl = torch.empty(2, device="cuda")
        rc = lib.mm_arcclassposteriors_f32(bh, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, xi.data_ptr(), xi.stride(0),
                                           xi.stride(2), xi.stride(1), ttl.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.mm_last_error()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1024)
        assert lib.mm_batch_kernels(bh, 14, buf, 1024) == 0
        k = buf.value.decode()
        assert "mm_arcclass_kernel<8,lds>" in k and k.endswith("terms in LDS"), k
        x, t = xi.cpu().numpy(), ttl.cpu().numpy()
        for b, L in enumerate([25, 19]):
            ref, z, exact = acr.reference(o, oc, g, f, cls_csc, nc, V[b].cpu().numpy().astype(np.float64), L, N)
            print(f"scrambled CSR utterance {b}: worst arc-class error / bar {acr.check(x[b], t[b], ref, z, exact):.3g}")
    finally:
        lib.mm_batch_destroy(bh)
        lib.mm_fsm_destroy(h)


def test_bit_identical_capture_relabelling_and_replacement(mm, wl, torch):
    g = wl.lfmmi_denominator(600, 40, seed=5)
    fs, bf = _batch(mm, wl, [g] * 6)
    f = fs[0]
    N = 120
    V = torch.from_numpy(np.random.default_rng(6).standard_normal((6, N, g.P)).astype(np.float32)).cuda()
    lens = torch.tensor([120, 100, 90, 120, 7, 64], dtype=torch.int32, device="cuda")
    cls, nc = _dst_pdf(g, f)
    cls = cls.copy()
    cls[::5] = -1
    bf.set_arc_classes(cls, nc)
    _is(bf, 8, "lds", "lds")
    x0, t0 = bf.arcclassposteriors(V, lens)
    x1, t1 = bf.arcclassposteriors(V, lens)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(t0, t1)
    assert float(x0.sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x2, t2 = bf.arcclassposteriors(V, lens)
    for _ in range(2):
        x2.zero_()
        t2.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(x2, x0) and torch.equal(t2, t0)
    # relabelling: class c becomes perm[c]; the rows move with their labels, bit for bit
    perm = np.random.default_rng(1).permutation(nc).astype(np.int32)
    bf.set_arc_classes(np.where(cls >= 0, perm[np.maximum(cls, 0)], -1).astype(np.int32), nc)
    x3, t3 = bf.arcclassposteriors(V, lens)
    torch.cuda.synchronize()
    assert torch.equal(x3[:, torch.from_numpy(perm.astype(np.int64)).cuda(), :], x0) and torch.equal(t3, t0)
    # replacing the plan takes effect: two classes, the even and the odd entries
    bf.set_arc_classes((np.arange(f.nnz) % 2).astype(np.int32), 2)
    x4, _ = bf.arcclassposteriors(V, lens)
    torch.cuda.synchronize()
    assert x4.shape == (6, 2, N)
    assert torch.allclose(x4.sum(dim=1), torch.ones_like(x4[:, 0]), atol=1e-4)  # every entry has a class: the frames add up to 1


def _word_loop(wl, lengths=(3, 4, 2)):
    """l2r_hmm-style chains (self-loop + forward arc), one per word, joined into a loop: the last state of a word goes on to the
    first state of every word, or ends.  One pdf per state.  Returns (graph, word of every state)."""
    first = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    S = int(sum(lengths))
    word = np.repeat(np.arange(len(lengths)), lengths)
    src, dst = list(range(S)), list(range(S))
    for w, n in enumerate(lengths):
        for s in range(first[w], first[w] + n - 1):
            src.append(s)
            dst.append(s + 1)
        for w2 in range(len(lengths)):
            src.append(first[w] + n - 1)
            dst.append(first[w2])
    src, dst = np.array(src), np.array(dst)
    fin = np.array([first[w] + n - 1 for w, n in enumerate(lengths)])
    tot = np.zeros(S)
    np.add.at(tot, src, 1.0)
    np.add.at(tot, fin, 1.0)
    g = wl.GraphSpec("wordloop", S, first.astype(np.int64), np.full(len(lengths), -np.log(len(lengths))), src, dst, -np.log(tot[src]), fin,
                     -np.log(tot[fin]), np.arange(S, dtype=np.int32), S)
    return g, word


def test_boundary_posteriors_of_a_word_loop(mm, wl, oracle, torch):
    """boundary_classes by word on a 3-word loop: the row of word w is P(an arc enters w from another word at frame t), and over
    the frames it adds up to the expected number of such entries into w that arcposteriors counts."""
    g, word = _word_loop(wl)
    fs, bf = _batch(mm, wl, [g] * 3)
    f = fs[0]
    cls = mm.boundary_classes(f, word)
    i, j, _ = ar.fsm_entries(f)
    # 3 word ends x the 2 OTHER words' starts: a word that follows itself does not leave its group, so it is no boundary
    assert (cls >= 0).sum() == 6 and (cls[cls >= 0] == word[j[cls >= 0]]).all() and (word[i[cls >= 0]] != word[j[cls >= 0]]).all()
    N = 40
    V = np.random.default_rng(12).standard_normal((3, N, g.P)).astype(np.float32)
    lens = np.array([40, 31, 12], dtype=np.int32)
    bf.set_arc_classes(cls, 3)
    _is(bf, 8, "lds", "lds")
    xi, ttl = bf.arcclassposteriors(V, lens)
    _check(oracle, [g] * 3, fs, [cls] * 3, 3, V, lens, xi, ttl, None, "boundaries")
    counts, _ = bf.arcposteriors(V, lens)
    for b in range(3):
        L = int(lens[b])
        for w in range(3):
            want = float(counts[b, : f.nnz].astype(np.float64)[cls == w].sum())
            got = float(xi[b, w].astype(np.float64).sum())
            assert abs(got - want) <= 1e-4 * want + 1e-6 * L, (b, w, got, want)
        assert (xi[b, :, L - 1 :] == 0).all()  # no word starts on the way into the final state or behind it


def test_error_codes(mm, wl, torch):
    lib = _lib(mm)
    g = wl.random_fsm(20, 4, 3.0, seed=1)
    N = 10
    V = torch.zeros((2, N, g.P), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = wl.to_fsm(mm, g)
    sm = mm.statemap(g.state2pdf, g.P)
    lb = mm.batch(*([mm.compile(f, sm)] * 2))
    nc = 3
    x = torch.zeros((2, N, nc), device="cuda")
    call = lambda bf, xp, sb, sn, sc: lib.mm_arcclassposteriors_f32(bf._h, V.data_ptr(), N * g.P, g.P, None, N, xp, sb, sn, sc, None, st)
    assert call(lb, x.data_ptr(), N * nc, nc, 1) == -1 and b"no classes set" in lib.mm_last_error()
    assert lb.kernels("arcclass").endswith("no classes set")
    cls = (np.arange(f.nnz) % nc).astype(np.int32)
    bad = cls.copy()
    bad[5] = nc
    assert lib.mm_batch_set_arc_classes(lb._h, bad.ctypes.data, None, nc) == -1 and b"outside" in lib.mm_last_error()
    bad[5] = -2
    assert lib.mm_batch_set_arc_classes(lb._h, bad.ctypes.data, None, nc) == -1
    assert lib.mm_batch_set_arc_classes(lb._h, cls.ctypes.data, None, 0) == -1 and b"C >= 1" in lib.mm_last_error()
    assert call(lb, x.data_ptr(), N * nc, nc, 1) == -1  # (the refused plans left none behind)
    tb = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), sm)] * 2))
    assert lib.mm_batch_set_arc_classes(tb._h, cls.ctypes.data, None, nc) == -4
    assert call(tb, x.data_ptr(), N * nc, nc, 1) == -4 and b"log" in lib.mm_last_error()
    with pytest.raises(mm.MarkovModelsAMDError):
        tb.kernels("arcclass")
    assert lib.mm_batch_set_arc_classes(lb._h, cls.ctypes.data, None, nc) == 0
    assert call(lb, None, N * nc, nc, 1) == -1
    assert call(lb, x.data_ptr(), N * nc, nc - 1, 1) == -2 and b"strides" in lib.mm_last_error()  # frames overlap
    assert call(lb, x.data_ptr(), N * nc - 1, nc, 1) == -2
    # a capture before the plan is on the device is refused, and so is replacing the plan inside one
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.mm_arcclassposteriors_f32(lb._h, V.data_ptr(), N * g.P, g.P, None, N, x.data_ptr(), N * nc, nc, 1, None,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        with pytest.raises(mm.MarkovModelsAMDError):
            lb.set_arc_classes(cls, nc)
    assert rc == -1, rc
    assert call(lb, x.data_ptr(), N * nc, nc, 1) == 0
    torch.cuda.synchronize()
    assert np.isclose(float(x.sum()), 2 * N, rtol=1e-4)  # every entry has a class
