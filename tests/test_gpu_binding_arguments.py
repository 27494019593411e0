"""What the Python binding (markovmodels.jl_amd/inference.py) refuses before it calls the library, and what it accepts: the kernels
write through the raw pointers and strides this layer hands over, so a wrong ``out``, ``state``, ``closed`` or ``want_state`` that
slipped through would be memory corruption, not an exception.  Every refusal here is raised in Python, ahead of the library; each
case asserts the exception's class (and code -2 of a DimensionMismatch) and the fixed part of its message, then calls the entry
correctly and compares every output, bit for bit, with the result taken before any refusal.

The batch: a left-to-right HMM of 3 states and a random graph of 5 (4 + 6 states with the phony final ones: total_states = 10 is a
multiple of neither, and no [B, S] tensor passes for [total_states]), N = 4 frames, lengths 4 and 2.  The log batch runs with the
deterministic gamma sum and a fixed exact policy, so that ``pdfposteriors`` too returns the same bits on every call (the other
entries have no atomics)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N, P, T = 2, 4, 3, 10
LENS = [4, 2]
# the good call of every entry: each argument the tests replace is given, so that a replaced one is the only change
GOOD = {
    "pdfposteriors": ("log", {}),
    "leakyposteriors": ("log", dict(leak=0.01)),
    "filterposteriors": ("log", dict(state="state", want_state=True)),
    "windowposteriors": ("log", dict(state="state", closed=[1, 0], commit=[3, 1], want_state=True)),
    "segmentposteriors": ("log", dict(state="state", end_mode=[2, 1], end="end", want_end=True)),
    "chunkedposteriors": ("log", dict(chunk=3)),  # (two chunks: both passes run, gamma is written through views of out)
    "weightedposteriors": ("log", {}),
    "viterbi": ("tropical", {}),
    "viterbiwindow": ("tropical", dict(state="state", closed=[1, 0], commit=[3, 1], want_state=True)),
}
WITH_OUT = ["pdfposteriors", "leakyposteriors", "filterposteriors", "windowposteriors", "segmentposteriors", "chunkedposteriors",
            "weightedposteriors"]
# (entry, argument, its name in the messages)
VECTORS_IN = [("filterposteriors", "state", "state"), ("windowposteriors", "state", "state"), ("segmentposteriors", "state", "state"),
              ("viterbiwindow", "state", "state"), ("segmentposteriors", "end", "end")]
# (entry, argument, its name in the messages, the result's position, the input it may alias)
VECTORS_OUT = [("filterposteriors", "want_state", "the state buffer", 3, "state"), ("windowposteriors", "want_state", "the state buffer", 3, "state"),
               ("viterbiwindow", "want_state", "the state buffer", 5, "state"), ("segmentposteriors", "want_end", "the end buffer", 3, "end")]
PER_UTT = [("windowposteriors", "closed"), ("windowposteriors", "commit"), ("viterbiwindow", "closed"), ("viterbiwindow", "commit"),
           ("segmentposteriors", "end_mode")]
BAD_VECTORS = ["float64", "one_more", "two_dims", "strided"]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(mm, wl, torch):
    c = Ctx()
    gs = [wl.l2r_hmm(3), wl.random_fsm(S=5, P=3, seed=1)]
    c.bf = {sem: mm.batch(*[mm.compile(wl.to_fsm(mm, g, semiring=sem), mm.statemap(g.state2pdf, g.P)) for g in gs]) for sem in ("log", "tropical")}
    c.bf["log"].set_deterministic(True).set_exact_policy("f32_first")
    assert all(bf.B == B and bf.P == P and bf.total_states == T for bf in c.bf.values())
    c.Vnp = np.random.default_rng(7).standard_normal((B, N, P)).astype(np.float32)
    c.V = torch.from_numpy(c.Vnp).cuda()
    c.lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    # carried vectors the entries made themselves: the state behind the first frame, the end vector of the whole
    c.vec = {("log", "state"): c.bf["log"].filterposteriors(c.V[:, :1], want_state=True)[3],
             ("tropical", "state"): c.bf["tropical"].viterbiwindow(c.V[:, :1], want_state=True)[5],
             ("log", "end"): c.bf["log"].segmentposteriors(c.V, c.lens, end_mode=[1, 1], want_end=True)[3]}
    assert all(v.shape == (T,) and torch.isfinite(v).any() for v in c.vec.values())
    c.baseline = {}
    return c


def _call(c, entry, **kw):
    sem, good = GOOD[entry]
    args = dict(good, **kw)
    for k in ("state", "end"):
        if isinstance(args.get(k), str):
            args[k] = c.vec[sem, k]
    V, lens = args.pop("V", c.V), args.pop("lens", c.lens)
    return getattr(c.bf[sem], entry)(V, lens=lens, **args)  # (by name: weightedposteriors takes W ahead of lens)


def _bits(res):
    return [None if r is None else (tuple(r.shape), str(r.dtype).replace("torch.", ""), (r.cpu().numpy() if hasattr(r, "cpu") else np.asarray(r)).tobytes())
            for r in res]


def _baseline(c, entry):
    """The good call's result, taken once, before the first refusal of the entry."""
    if entry not in c.baseline:
        c.baseline[entry] = _bits(_call(c, entry))
    return c.baseline[entry]


def _refused(mm, c, entry, exc, text, **kw):
    want = _baseline(c, entry)
    with pytest.raises(exc) as e:
        _call(c, entry, **kw)
    assert type(e.value) is exc and text in str(e.value), (type(e.value), str(e.value))
    if exc is mm.DimensionMismatch:
        assert e.value.code == -2
    assert _bits(_call(c, entry)) == want  # the batch is as it was


def _bad_vector(torch, c, good, kind):
    """(what is wrong with it, the exception, the message after the argument's name)"""
    if kind == "float64":
        return good.double(), TypeError, " must be a float32 tensor on V's device"
    x = {"one_more": torch.zeros(T + 1, device="cuda"), "two_dims": good[None], "strided": torch.zeros(2 * T, device="cuda")[::2]}[kind]
    assert kind != "strided" or (x.shape == (T,) and not x.is_contiguous())
    return x, None, f" must be a contiguous [{T}] vector, got {tuple(x.shape)}"


# ---- out ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float64", "cpu", "numpy"])
@pytest.mark.parametrize("entry", WITH_OUT)
def test_out_of_the_wrong_kind(mm, torch, ctx, entry, kind):
    out = {"float64": lambda: torch.empty((B, N, P), dtype=torch.float64, device="cuda"), "cpu": lambda: torch.empty((B, N, P), dtype=torch.float32),
           "numpy": lambda: np.empty((B, N, P), dtype=np.float32)}[kind]()
    _refused(mm, ctx, entry, TypeError, "out must be a float32 tensor on V's device", out=out)


@pytest.mark.parametrize("shape", [(B, N, P + 1), (B, N + 1, P), (B * N, P)])
@pytest.mark.parametrize("entry", WITH_OUT)
def test_out_of_the_wrong_shape(mm, torch, ctx, entry, shape):
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    _refused(mm, ctx, entry, mm.DimensionMismatch, f"out must be [B={B}, N={N}, P={P}], got {shape}", out=out)


@pytest.mark.parametrize("entry", WITH_OUT)
def test_a_good_out_is_written_and_returned(torch, ctx, entry):
    out = torch.full((B, N, P), 7.0, device="cuda")
    res = _call(ctx, entry, out=out)
    assert res[0] is out and _bits(res) == _baseline(ctx, entry)


def test_out_without_filt_is_refused_before_its_dtype(mm, torch, ctx):
    for dtype in (torch.float64, torch.float32):
        _refused(mm, ctx, "filterposteriors", ValueError, "out given with want_filt=False", out=torch.empty((B, N, P), dtype=dtype, device="cuda"),
                 want_filt=False)


# ---- state, end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BAD_VECTORS)
@pytest.mark.parametrize("entry,arg,name", VECTORS_IN)
def test_carried_vector_in_refused(mm, torch, ctx, entry, arg, name, kind):
    x, exc, text = _bad_vector(torch, ctx, ctx.vec[GOOD[entry][0], arg], kind)
    _refused(mm, ctx, entry, exc or mm.DimensionMismatch, name + text, **{arg: x})


@pytest.mark.parametrize("entry,arg,name", VECTORS_IN)
def test_carried_vector_in_from_numpy_float64(ctx, entry, arg, name):
    good = ctx.vec[GOOD[entry][0], arg]
    x = good.cpu().numpy().astype(np.float64)
    assert x.shape == (T,) and x.dtype == np.float64
    assert _bits(_call(ctx, entry, **{arg: x})) == _baseline(ctx, entry)


# ---- want_state, want_end as the tensor that receives the vector --------------------------------------------------------------
@pytest.mark.parametrize("kind", BAD_VECTORS)
@pytest.mark.parametrize("entry,arg,name,pos,alias", VECTORS_OUT)
def test_carried_vector_out_refused(mm, torch, ctx, entry, arg, name, pos, alias, kind):
    x, exc, text = _bad_vector(torch, ctx, ctx.vec[GOOD[entry][0], alias], kind)
    _refused(mm, ctx, entry, exc or mm.DimensionMismatch, name + text, **{arg: x})


@pytest.mark.parametrize("entry,arg,name,pos,alias", VECTORS_OUT)
def test_carried_vector_out_is_the_tensor_given(torch, ctx, entry, arg, name, pos, alias):
    want = _baseline(ctx, entry)
    buf = torch.full((T,), 7.0, device="cuda")
    res = _call(ctx, entry, **{arg: buf})
    assert res[pos] is buf and _bits(res) == want
    # ... the input itself included (a copy of it: the call overwrites it)
    both = ctx.vec[GOOD[entry][0], alias].clone()
    res = _call(ctx, entry, **{alias: both, arg: both})
    assert res[pos] is both and _bits(res) == want


# ---- closed, commit, end_mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,arg", PER_UTT)
def test_per_utterance_vector_refused(mm, torch, ctx, entry, arg):
    good = GOOD[entry][1][arg]
    _refused(mm, ctx, entry, mm.DimensionMismatch, f"{arg} must be a [{B}] vector, got {(B + 1,)}", **{arg: good + [0]})
    _refused(mm, ctx, entry, mm.DimensionMismatch, f"{arg} must be a [{B}] vector, got {(B, 1)}",
             **{arg: torch.tensor(good, dtype=torch.int32, device="cuda")[:, None]})


@pytest.mark.parametrize("entry,arg", PER_UTT)
def test_per_utterance_vector_accepted_forms(torch, ctx, entry, arg):
    good = GOOD[entry][1][arg]
    want = _baseline(ctx, entry)  # (taken with the Python list)
    for x in (list(good), np.asarray(good, dtype=np.int64), torch.tensor(good, dtype=torch.int64, device="cuda")):
        assert _bits(_call(ctx, entry, **{arg: x})) == want, type(x)


# ---- V, lens --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["pdfposteriors", "viterbi"])
def test_V_and_lens(mm, torch, ctx, entry):
    c = ctx
    _refused(mm, c, entry, TypeError, "V must be a float32 tensor on the HIP device", V=c.V.double())
    for shape in ((B, N, P + 1), (B + 1, N, P)):
        _refused(mm, c, entry, mm.DimensionMismatch, f"V must be [B={B}, N, P={P}], got {shape}", V=torch.zeros(shape, device="cuda"))
    _refused(mm, c, entry, mm.DimensionMismatch, "lens must have B entries", lens=torch.tensor(LENS + [1], dtype=torch.int32, device="cuda"))
    Vt = c.V.transpose(1, 2).contiguous().transpose(1, 2)  # the same values, the frames adjacent in memory
    assert Vt.shape == (B, N, P) and Vt.stride(2) != 1 and torch.equal(Vt, c.V)
    assert _bits(_call(c, entry, V=Vt)) == _baseline(c, entry)


# ---- the module-level entries in pdfposteriors' call shape ----------------------------------------------------------------------
@pytest.mark.parametrize("entry,kw", [("leakyposteriors", dict(leak=0.01)), ("filterposteriors", {}), ("windowposteriors", dict(closed=[1, 0])),
                                      ("chunkedposteriors", dict(chunk=3))])
def test_module_level_entries_on_host_and_device(mm, torch, ctx, entry, kw):
    c, fn, bf = ctx, getattr(mm, entry), ctx.bf["log"]
    Vh = [mm.expand(c.Vnp[b].T, LENS[b]) for b in range(B)]
    Vd = [torch.from_numpy(v).cuda() for v in Vh]
    host = fn(bf, Vh, **kw)
    assert all(isinstance(r, np.ndarray) for r in host) and host[0].shape == (B, P, N) and host[0].flags.c_contiguous
    dev = fn(bf, Vd, seqlengths=LENS, **kw)
    assert all(isinstance(r, torch.Tensor) and r.is_cuda for r in dev) and len(dev) == len(host)
    assert dev[0].shape == (B, P, N) and not dev[0].is_contiguous() and dev[0].transpose(1, 2).is_contiguous()  # a view of [B, N, P]
    assert _bits(dev) == _bits(host)
    # the values are the method's own
    own = getattr(bf, entry)(c.V, lens=c.lens, **kw)
    assert _bits([own[0].transpose(1, 2)] + list(own[1 : len(host)])) == _bits(host)
    # device V_hats without their lengths go to the host, where the phony row gives them
    unasked = fn(bf, Vd, **kw)
    assert all(isinstance(r, np.ndarray) for r in unasked) and unasked[0].flags.c_contiguous and _bits(unasked) == _bits(host)
    with pytest.raises(mm.DimensionMismatch) as e:
        fn(bf, Vd + [Vd[0]], seqlengths=LENS + [1], **kw)
    assert e.value.code == -2 and f"{B + 1} matrices V_hat for a batch of {B} FSMs" in str(e.value)
    assert _bits(fn(bf, Vd, seqlengths=LENS, **kw)) == _bits(host)
