"""Host-side mirror of src/inference.jl: CompiledFSM / compile / batch / expand /
alpha-recursion / beta-recursion / pdfposteriors, plus bestpath
(docs/src/inference.md:4-6).  Every compute entry point is ONE call into the
HIP engine through the C ABI (include/markovmodels_amd.h); there is no CPU
path here.

Two ways in:
  * the reference call shapes -- ``pdfposteriors(fsm, Vhats, Chats)`` with
    ``Vhats`` made by ``expand`` (src/inference.jl:145-161), or the
    prepare-once variant ``pdfposteriors(batch(cfsm...), Vhats)``
    (``pdfposteriors2``, :164-180);
  * the native one the bench uses -- ``BatchedFSM.pdfposteriors(V, lens)`` on
    device-resident ``V[B, N, P]`` log-likelihoods and lengths, no host round
    trips.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict  # noqa: F401
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import SEMIRING_ID, check, lib
from .fsm import FSM, GeneralStateMap, StateMap, split_blocks, statemap

_ZERO = -np.inf
_SEM_ZERO = {"log": -np.inf, "tropical": -np.inf, "prob": 0.0}
_SEM_ONE = {"log": 0.0, "tropical": 0.0, "prob": 1.0}


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("markovmodels_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


# ---- what the BatchedFSM entries check, allocate and pass alike.  The kernels write through the raw pointers and strides this layer
# hands over: a wrong buffer is memory corruption, not an exception.  Functions of the tensor and of the device or shape it must
# match, not of a batch, so that they run on CPU tensors as well.
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _head(h, Vt, lt, N):
    """What the argument list of every entry starts with: the batch, V and its strides, the lengths, N."""
    return h, Vt.data_ptr(), Vt.stride(0), Vt.stride(1), _ptr(lt), N


def _out_buffer(out, shape, device):
    """The ``out`` of a call, a float32 tensor [B, N, P] on V's device with strides of its own, or a fresh buffer."""
    import torch

    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != device:
        raise TypeError("out must be a float32 tensor on V's device")
    if tuple(out.shape) != tuple(shape):
        B, N, P = shape
        raise _lib.DimensionMismatch(-2, f"out must be [B={B}, N={N}, P={P}], got {tuple(out.shape)}")
    return out


def _state_vector(x, name, n, device):
    """A carried vector (``state``, ``end``, or the tensor that receives one): float32, contiguous [n = total_states], on V's device.
    What is not a tensor goes there through NumPy; None passes."""
    import torch

    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
        if device.type == "cuda":  # (the current device: the check below compares it with V's)
            x = x.cuda()
    if x.dtype != torch.float32 or x.device != device:
        raise TypeError(f"{name} must be a float32 tensor on V's device")
    if x.dim() != 1 or x.numel() != n or not x.is_contiguous():
        raise _lib.DimensionMismatch(-2, f"{name} must be a contiguous [{n}] vector, got {tuple(x.shape)}")
    return x


def _want_vector(want, name, n, device):
    """``want_state`` / ``want_end``: the tensor that receives the vector (checked), or whether to make one; None if not wanted."""
    import torch

    if isinstance(want, torch.Tensor):
        return _state_vector(want, name, n, device)
    return torch.empty(n, dtype=torch.float32, device=device) if want else None


def _per_utt(x, name, B, device):
    """A per-utterance argument (``closed``, ``commit``, ``end_mode``) as a contiguous int32 [B] tensor on V's device; None passes."""
    import torch

    if x is None:
        return None
    t = x.to(device=device, dtype=torch.int32) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.int32)).to(device)
    if t.dim() != 1 or t.numel() != B:
        raise _lib.DimensionMismatch(-2, f"{name} must be a [{B}] vector, got {tuple(t.shape)}")
    return t.contiguous()


def _class_scores(U, name, shape, device):
    """the per-frame class scores of an entry: None, or a float32 [B, N, C] tensor on the batch's device"""
    if U is None:
        return None
    torch = _torch()
    Ut = U if isinstance(U, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(U, dtype=np.float32))
    Ut = Ut.to(device=device)
    if Ut.dtype != torch.float32:
        raise TypeError(f"{name} must be float32")
    if tuple(Ut.shape) != tuple(shape):
        raise _lib.DimensionMismatch(-2, f"{name} must be [B={shape[0]}, N={shape[1]}, C={shape[2]}], got {tuple(Ut.shape)}")
    return Ut


def _beam_vector(beam, B, device):
    """The ``beam`` of a lattice call as a contiguous float32 [B] tensor on V's device: a number (every utterance's beam) or a [B]
    tensor / array."""
    import torch

    if isinstance(beam, torch.Tensor):
        t = beam.to(device=device, dtype=torch.float32)
    elif np.ndim(beam) == 0:
        return torch.full((B,), float(beam), dtype=torch.float32, device=device)
    else:
        t = torch.as_tensor(np.asarray(beam, dtype=np.float32)).to(device)
    if t.dim() == 0:
        return t.expand(B).contiguous()
    if t.dim() != 1 or t.numel() != B:
        raise _lib.DimensionMismatch(-2, f"beam must be a number or a [{B}] vector, got {tuple(t.shape)}")
    return t.contiguous()


def _record_cap(max_arcs):
    """``max_arcs`` of a lattice call: None, or a record count >= 0."""
    if max_arcs is None:
        return None
    cap = int(max_arcs)
    if cap < 0:
        raise ValueError(f"max_arcs must be >= 0, got {max_arcs}")
    return cap


class Lattice(NamedTuple):
    """What ``BatchedFSM.lattice`` returns.  ``counts[B, N]`` int32: the kept arcs of every transition; ``offsets[B * N + 1]`` int64:
    their exclusive prefix sum in row-major (b, t) order -- the records of (b, t) are ``offsets[b * N + t] : offsets[b * N + t + 1]``,
    ``offsets[-1]`` the total; ``arc`` int32 / ``score`` float32: per record the stored entry k of the utterance's FSM (ascending
    within a transition) and its through-score relative to the best path (<= 0 up to rounding); ``best[B]``: the best path's
    weight."""

    counts: object
    offsets: object
    arc: object
    score: object
    best: object


class LatticePosteriors(NamedTuple):
    """What ``BatchedFSM.latticeposteriors`` returns.  ``post`` float32, one per record of the lattice: the log posterior of the
    record (<= 0; -inf: no path through it); ``logz[B]``: the log-sum of the lattice's paths (-inf: none); ``gamma[B, N, P]``: the
    pdf occupancies, the gradient of ``logz`` against ``V`` (None when not asked for)."""

    post: object
    logz: object
    gamma: object


class LatticeCost(NamedTuple):
    """What ``BatchedFSM.latticecost`` returns.  ``risk[B]``: the expected cost of the lattice's paths (0: no path); ``diff`` float32,
    one per record: d risk / d extra, the record's posterior times (the expected cost of the paths through it - risk); ``post`` and
    ``logz`` as in ``LatticePosteriors`` (``exp(post)`` is d risk / d cost); ``grad[B, N, P]``: d risk / d V; ``gamma[B, N, P]``: the
    pdf occupancies (either None when not asked for)."""

    risk: object
    diff: object
    post: object
    logz: object
    grad: object
    gamma: object


class LatticeBest(NamedTuple):
    """What ``BatchedFSM.latticebest`` returns.  ``best[B]``: the weight of the lattice's best path (-inf: none); ``score`` float32,
    one per record: the best path through the record minus ``best`` (<= 0 up to rounding; -inf: no path through it); ``rec[B, N]``
    int64: the best path's record of every transition, an index into ``lat.arc``; ``path[B, N]`` int32: the source state of that
    record, ``bestpath``'s convention (both -1 at and behind ``len`` and without a path; None when not asked for)."""

    best: object
    score: object
    rec: object
    path: object


class LatticeSamples(NamedTuple):
    """What ``BatchedFSM.latticesample`` returns.  ``rec[B, K, N]`` int64: sample k's record of every transition, an index into
    ``lat.arc``; ``path[B, K, N]`` int32: the source state of that record, ``bestpath``'s convention (both -1 at and behind ``len``
    and without a path; ``path`` None when not asked for); ``logprob[B, K]``: the log posterior of the sampled record sequence
    among the lattice's paths (-inf without a path; None when not asked for); ``logz[B]``: the lattice's log-sum,
    ``latticeposteriors``' (-inf: no path)."""

    rec: object
    path: object
    logprob: object
    logz: object


def _on_device(x, dtype, device):
    """A member of a lattice (or ``extra``) as a contiguous tensor of ``dtype`` on ``device``: a tensor, or anything NumPy reads."""
    import torch

    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype).contiguous()


def _results(res, as_numpy):
    """The tuple an entry returns: NumPy arrays if V came as NumPy, None members as they are."""
    return tuple(t.cpu().numpy() if t is not None else None for t in res) if as_numpy else res


class CompiledFSM:
    """CompiledFSM{K} (src/inference.jl:3-12): alpha_hat, T_hat, T_hat', C_hat, C_hat'
    prepared once -- here as the packed device forms the kernels stream."""

    def __init__(self, fsm: FSM, C_hat: Union[StateMap, np.ndarray]):
        if not isinstance(C_hat, StateMap):
            C_hat = StateMap.from_matrix(C_hat)
        if C_hat.shape[0] != fsm.S1:
            raise _lib.DimensionMismatch(-2, f"C_hat has {C_hat.shape[0]} rows, the FSM {fsm.S1} states")
        self.fsm = fsm
        self.C_hat = C_hat
        self.semiring = fsm.semiring
        self.S1 = fsm.S1
        self.P1 = C_hat.numpdf + 1
        # K of FSM{K}: the precision of the computation follows the FSM's, like the reference (src/inference.jl:147 converts
        # V_hat to K)
        self.dtype = np.dtype(np.float64) if np.asarray(fsm.nzval).dtype == np.float64 else np.dtype(np.float32)
        colptr = np.ascontiguousarray(fsm.colptr, dtype=np.int64)
        rowval = np.ascontiguousarray(fsm.rowval, dtype=np.int64)
        nzval = np.ascontiguousarray(fsm.nzval, dtype=np.float32 if fsm.nzval.dtype != np.float64 else np.float64)
        aidx = np.ascontiguousarray(fsm.alpha_idx, dtype=np.int64)
        aval = np.ascontiguousarray(fsm.alpha_val, dtype=nzval.dtype)
        s2p = np.ascontiguousarray(C_hat.state2pdf, dtype=np.int32)
        h = C.c_void_p()
        check(lib.mm_fsm_create(SEMIRING_ID[self.semiring], self.S1, fsm.nnz, _lib.MM_CSC, 8, 0, nzval.dtype.itemsize,
                                colptr.ctypes.data, rowval.ctypes.data, nzval.ctypes.data, aidx.shape[0],
                                aidx.ctypes.data, aval.ctypes.data, s2p.ctypes.data, self.P1, C.byref(h)))
        self._h = h

    @classmethod
    def _from_handle(cls, fsm: FSM, C_hat: StateMap, h) -> "CompiledFSM":
        """Around a handle the library has made already (compile_many)."""
        self = cls.__new__(cls)
        self.fsm = fsm
        self.C_hat = C_hat
        self.semiring = fsm.semiring
        self.S1 = fsm.S1
        self.P1 = C_hat.numpdf + 1
        self.dtype = np.dtype(np.float64) if np.asarray(fsm.nzval).dtype == np.float64 else np.dtype(np.float32)
        self._h = h
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:  # lib is None while the interpreter shuts down
            lib.mm_fsm_destroy(h)
            self._h = None

    def info(self) -> dict:
        S1, nnz, P1 = C.c_int64(), C.c_int64(), C.c_int32()
        slots, items = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        check(lib.mm_fsm_info(self._h, C.byref(S1), C.byref(nnz), C.byref(P1), slots, items))
        return dict(S1=S1.value, nnz=nnz.value, P1=P1.value, packed_slots=list(slots), packed_items=list(items))

    def packed_product(self, x: np.ndarray, direction: int = 0):
        """Host evaluation of one semiring product through the packed form (test aid)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        arg = np.empty(self.S1, dtype=np.int32)
        check(lib.mm_debug_packed_product(self._h, direction, x.ctypes.data, out.ctypes.data, arg.ctypes.data))
        return out, arg


    def reach_distance(self, direction: int = 0) -> np.ndarray:
        """Fewest arcs from an initial state (direction 0) / to the phony final state (direction 1) for every
        state of the extended FSM, -1 = unreachable: the static dead-row bound of the fast kernels (host only)."""
        out = np.empty(self.S1, dtype=np.int32)
        check(lib.mm_debug_reach_distance(self._h, direction, out.ctypes.data))
        return out

    def stream_product(self, x: np.ndarray, direction: int = 0, H: int = 1):
        """Host evaluation of the product through the stream form of the stream kernels, for teams of H = 1, 2 or 4 workgroups (test
        aid).  Returns (out, stats = [arc slots per lane over all waves and sets, segments, real arcs / arc slots, slots of the most
        loaded wave])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        stats = np.zeros(4, dtype=np.float64)
        check(lib.mm_debug_stream_team_product(self._h, int(H), direction, x.ctypes.data, out.ctypes.data, stats.ctypes.data))
        return out, stats

    def quad_product(self, x: np.ndarray, direction: int = 0, KQ: int = 5):
        """Host evaluation of the same product through the quad form of the fast kernel (test aid).
        Returns (out, stats = [quads, lanes, LDS cycles/gather naive, after placement])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        stats = np.zeros(4, dtype=np.float64)
        check(lib.mm_debug_quad_product(self._h, direction, KQ, x.ctypes.data, out.ctypes.data, stats.ctypes.data))
        return out, stats

    def quad_layout(self, direction: int = 0, KQ: int = 5):
        """Where the quad form puts every row (test aid).  Returns (order [S1]: internal position -> state, recs [S1, 4] uint16:
        the row records {qe, i1, pdf, i2} the kernel reads, see mm_debug_quad_layout)."""
        order = np.empty(self.S1, dtype=np.int32)
        recs = np.empty((self.S1, 4), dtype=np.uint16)
        check(lib.mm_debug_quad_layout(self._h, direction, KQ, order.ctypes.data, recs.ctypes.data))
        return order, recs


    def row_product(self, x: np.ndarray, direction: int = 0, pair: bool = False, copies: int = 0, scrambled: bool = False, bank_opt: bool = False):
        """Host evaluation of the same product through the row-lane form of the row kernels, or its pair variant
        (test aid); copies / scrambled: the copies of the linear vector the placement may use.
        Returns (out, stats = [KA, compute waves, segments, arcs / arc slots, max wave cost, min wave cost,
        LDS cycles/gather naive, after placement])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        stats = np.zeros(8, dtype=np.float64)
        flags = (1 if pair else 0) | (int(copies) << 1) | (8 if scrambled else 0) | (16 if bank_opt else 0)
        check(lib.mm_debug_row_product_ex(self._h, direction, flags, x.ctypes.data, out.ctypes.data, stats.ctypes.data))
        return out, stats

    def pair_pdf_table(self, direction: int = 0):
        """The pdf-major table of the pair form (what phase B of the pair kernels sums the posteriors through; test aid).
        Returns (table [S1] = 8 * position | (8 * partner position) << 16, pdfse [P + 1, 2] = (first, end) of each pdf's range,
        slot words [S1, 2] of the lanes that finish a row)."""
        import ctypes as C

        tab = np.zeros(self.S1, dtype=np.uint32)
        pdfse = np.zeros((self.P1, 2), dtype=np.uint16)
        slots = np.zeros((self.S1, 2), dtype=np.uint32)
        rows = C.c_int64(0)
        check(lib.mm_debug_pair_pdftab(self._h, direction, C.byref(rows), tab.ctypes.data, pdfse.ctypes.data, slots.ctypes.data))
        assert rows.value == self.S1
        return tab, pdfse, slots

    def split_product(self, x: np.ndarray, direction: int = 0, H: int = 2):
        """Host evaluation of the product through the split pair forms (teams of H workgroups; test aid).  Returns
        (out, stats = [KA, positions of the team's vector, segments, arcs / arc slots, max / min wave cost, LDS
        cycles/gather naive, after placement])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        stats = np.zeros(8, dtype=np.float64)
        check(lib.mm_debug_split_product(self._h, int(H), direction, x.ctypes.data, out.ctypes.data, stats.ctypes.data))
        return out, stats

    def wave_product(self, x: np.ndarray, direction: int = 0):
        """Host evaluation of the product through the wave form (one wave per direction, log domain; test aid).
        Returns (out, stats = [arc slots per lane, segments, arcs / arc slots, LDS cycles/gather])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.S1, dtype=np.float32)
        stats = np.zeros(4, dtype=np.float64)
        check(lib.mm_debug_wave_product(self._h, direction, x.ctypes.data, out.ctypes.data, stats.ctypes.data))
        return out, stats


def compile(fsm: FSM, C_hat) -> CompiledFSM:  # noqa: A001 - the reference's name
    """compile(fsm, C_hat) (src/inference.jl:11-12)."""
    return CompiledFSM(fsm, C_hat)


def compile_many(fsms, C_hats, threads: int = 0):
    """`compile.(fsms, C_hats)` (the reference broadcasts compile over a mini-batch of numerator graphs,
    examples/test_cuda.jl:76-78) in ONE call of the library (mm_fsm_create_many): the graphs are compiled on host threads,
    small graphs get the forms of their kernel at once, and everything goes to the device as one allocation and one
    copy.  C_hats: one state map for all, or one per FSM.  The handles are what ``compile`` would have made."""
    fsms = list(fsms)
    n = len(fsms)
    maps = list(C_hats) if isinstance(C_hats, (list, tuple)) else [C_hats] * n
    if len(maps) != n:
        raise ValueError("compile_many: one C_hat per FSM (or one for all)")
    if n == 0:
        return []
    maps = [m if isinstance(m, StateMap) else StateMap.from_matrix(m) for m in maps]
    sem = fsms[0].semiring
    f64 = np.asarray(fsms[0].nzval).dtype == np.float64
    vdt = np.float64 if f64 else np.float32
    if any(f.semiring != sem or (np.asarray(f.nzval).dtype == np.float64) != f64 for f in fsms):
        raise TypeError("compile_many: the FSMs of one call share the semiring and the float type (FSM{K})")
    keep = []  # the arrays the pointers below refer to

    def arr(a, dt):
        a = np.asarray(a)
        if a.dtype != dt or not a.flags.c_contiguous:
            a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.__array_interface__["data"][0]

    S1 = np.empty(n, np.int64)
    nnz = np.empty(n, np.int64)
    ninit = np.empty(n, np.int64)
    P1 = np.empty(n, np.int32)
    ptrs = np.empty((7, n), np.uint64)  # colptr, rowval, nzval, alpha_idx, alpha_val, state2pdf per graph
    for i, (f, m) in enumerate(zip(fsms, maps)):
        if m.shape[0] != f.S1:
            raise _lib.DimensionMismatch(-2, f"C_hat {i} has {m.shape[0]} rows, the FSM {f.S1} states")
        S1[i], nnz[i], P1[i] = f.S1, f.nnz, m.numpdf + 1
        ptrs[0, i] = arr(f.colptr, np.int64)
        ptrs[1, i] = arr(f.rowval, np.int64)
        ptrs[2, i] = arr(f.nzval, vdt)
        ai = np.asarray(f.alpha_idx)
        ninit[i] = ai.shape[0]
        ptrs[3, i] = arr(ai, np.int64)
        ptrs[4, i] = arr(f.alpha_val, vdt)
        ptrs[5, i] = arr(m.state2pdf, np.int32)
    out = (C.c_void_p * n)()
    check(lib.mm_fsm_create_many(n, SEMIRING_ID[sem], _lib.MM_CSC, 8, 0, 8 if f64 else 4, S1.ctypes.data, nnz.ctypes.data,
                                 ptrs[0].ctypes.data, ptrs[1].ctypes.data, ptrs[2].ctypes.data, ninit.ctypes.data, ptrs[3].ctypes.data,
                                 ptrs[4].ctypes.data, ptrs[5].ctypes.data, P1.ctypes.data, int(threads), out))
    return [CompiledFSM._from_handle(f, m, C.c_void_p(out[i])) for i, (f, m) in enumerate(zip(fsms, maps))]


class BatchedFSM:
    """batch(cfsm...) (src/inference.jl:28-36): B independent compiled FSMs as
    one block-diagonal system.  Repeating one CompiledFSM B times shares its
    device storage (the denominator case)."""

    def __init__(self, cfsms: Sequence[CompiledFSM]):
        self.cfsms = list(cfsms)
        self.B = len(self.cfsms)
        arr = (C.c_void_p * self.B)(*[c._h for c in self.cfsms])
        h = C.c_void_p()
        check(lib.mm_batch_create(arr, self.B, C.byref(h)))
        self._h = h
        self.semiring = self.cfsms[0].semiring
        self.dtype = np.dtype(np.float64) if any(c.dtype == np.float64 for c in self.cfsms) else np.dtype(np.float32)
        self.P = self.cfsms[0].P1 - 1
        if any(c.P1 != self.P + 1 for c in self.cfsms):
            raise _lib.DimensionMismatch(-2, "all FSMs of a batch must share the number of pdfs")
        self.total_states = int(lib.mm_batch_total_states(h))
        self.state_offsets = np.cumsum([0] + [c.S1 for c in self.cfsms])

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.mm_batch_destroy(h)
            self._h = None

    # -- helpers -----------------------------------------------------------------
    def _prep(self, V, lens):
        torch = _torch()
        as_numpy = not isinstance(V, torch.Tensor)
        Vt = torch.as_tensor(np.ascontiguousarray(V, dtype=np.float32)).cuda() if as_numpy else V
        if Vt.dtype != torch.float32 or not Vt.is_cuda:
            raise TypeError("V must be a float32 tensor on the HIP device")
        if Vt.dim() != 3 or Vt.shape[0] != self.B or Vt.shape[2] != self.P:
            raise _lib.DimensionMismatch(-2, f"V must be [B={self.B}, N, P={self.P}], got {tuple(Vt.shape)}")
        if Vt.stride(2) != 1:
            Vt = Vt.contiguous()
        lt = None
        if lens is not None:
            lt = torch.as_tensor(np.asarray(lens, dtype=np.int32)).cuda() if not isinstance(lens, torch.Tensor) else lens
            lt = lt.to(device=Vt.device, dtype=torch.int32).contiguous()
            if lt.numel() != self.B:
                raise _lib.DimensionMismatch(-2, "lens must have B entries")
        return torch, Vt, lt, as_numpy

    @staticmethod
    def _stream(torch):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # -- compute -------------------------------------------------------------------
    def pdfposteriors(self, V, lens=None, out=None):
        """One call of the engine: gamma[B, N, P] (probabilities), ttl[B]."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        gamma = _out_buffer(out, (B, N, P), Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_pdfposteriors_f32(*_head(self._h, Vt, lt, N), gamma.data_ptr(), *gamma.stride(), ttl.data_ptr(), self._stream(torch)))
        return _results((gamma, ttl), as_numpy)

    def has_fast_entry(self) -> bool:
        """True if ``pdfposteriors(V, lens)`` -- mm_pdfposteriors_f32, the fast kernels -- serves this batch: Log batches always,
        ProbSemiring batches of Float32 FSMs (the library keeps their log-semiring twins: ``kernels()`` names the twins' kernels),
        Tropical batches never (their fast entry is ``viterbi``)."""
        if self.semiring == "log":
            return True
        if self.semiring != "prob" or self.dtype == np.float64:
            return False
        try:
            return bool(self.kernels("log"))
        except _lib.MarkovModelsAMDError:
            return False

    def reserve_ex(self, dtype, N1: int):
        """Size the generic entry's workspace for V_hat of N1 = N + 1 columns (mm_batch_reserve_ex): before capturing
        ``pdfposteriors_ex`` in a hipGraph."""
        check(lib.mm_batch_reserve_ex(self._h, np.dtype(dtype).itemsize, int(N1)))

    def pdfposteriors_ex(self, Vhat, maps=None, gamma=None, ttl=None):
        """The generic entry, device resident and asynchronous like the fast one (mm_pdfposteriors_ex): ``Vhat`` a
        float32 / float64 tensor [B, N1, P1] on the device (element (b, n, p) = V_hat_b[p, n]), ``maps`` None or a ctypes
        array of B mm_statemap_t handles the caller keeps alive until the stream has run the call.  Returns the tensors
        (gamma[B, N, P], ttl[B])."""
        torch = _torch()
        if not isinstance(Vhat, torch.Tensor) or not Vhat.is_cuda or Vhat.dtype not in (torch.float32, torch.float64):
            raise TypeError("Vhat must be a float32 / float64 tensor on the HIP device")
        if Vhat.dim() != 3 or Vhat.shape[0] != self.B or Vhat.stride(2) != 1:
            raise _lib.DimensionMismatch(-2, f"Vhat must be [B={self.B}, N + 1, P + 1] with the pdfs contiguous, got {tuple(Vhat.shape)}")
        _, N1, P1 = Vhat.shape
        if gamma is None:
            gamma = torch.zeros((self.B, N1 - 1, P1 - 1), dtype=Vhat.dtype, device=Vhat.device)
        if ttl is None:
            ttl = torch.zeros(self.B, dtype=Vhat.dtype, device=Vhat.device)
        if gamma.dtype != Vhat.dtype or ttl.dtype != Vhat.dtype or tuple(gamma.shape) != (self.B, N1 - 1, P1 - 1) or ttl.numel() != self.B:
            raise _lib.DimensionMismatch(-2, "gamma must be [B, N, P] and ttl [B] of V_hat's dtype")
        check(lib.mm_pdfposteriors_ex(self._h, maps, Vhat.element_size(), P1, Vhat.data_ptr(), Vhat.stride(0), Vhat.stride(1), N1,
                                      gamma.data_ptr(), gamma.stride(0), gamma.stride(1), gamma.stride(2), ttl.data_ptr(),
                                      self._stream(torch)))
        return gamma, ttl

    def pdfposteriors_generic(self, Vhats, Chats=None, dtype=None):
        """The generic entry (mm_pdfposteriors_ex): any semiring of the batch (log / tropical / prob), float32 or
        float64, any sparse state maps (``GeneralStateMap``; None: every FSM's own), any (P+1) x (N+1) matrices V_hat.
        Returns NumPy (gamma[B, P, N], ttl[B]) like the reference (src/inference.jl:145-161)."""
        import ctypes

        torch = _torch()
        Vh = [np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in Vhats]
        if len(Vh) != self.B or any(v.shape != Vh[0].shape for v in Vh):
            raise _lib.DimensionMismatch(-2, "need B matrices V_hat of one (P+1) x (N+1) shape")
        P1, N1 = Vh[0].shape
        # precision: the FSM's K unless asked for (src/inference.jl:147: copyto!(similar(V_hat, K), V_hat))
        dt = np.dtype(dtype) if dtype is not None else self.dtype
        if Chats is not None:  # raw matrices (dense / scipy.sparse) become GeneralStateMap; one-hot StateMap = the FSM's own
            Chats = [c if (c is None or isinstance(c, (StateMap, GeneralStateMap))) else GeneralStateMap(c, self.semiring) for c in Chats]
            if len(Chats) != self.B:
                raise _lib.DimensionMismatch(-2, "need one C_hat per utterance")
        for b in range(self.B):  # rows of V_hat against the pdfs of the map in force (src/inference.jl:146-150)
            want = self.cfsms[b].P1 if (Chats is None or Chats[b] is None or isinstance(Chats[b], StateMap)) else Chats[b].shape[1]
            if P1 != want:
                raise _lib.DimensionMismatch(-2, f"V_hat has {P1} rows, the state map of utterance {b} has {want} pdfs "
                                                 f"(P + 1: was expand() applied?)")
        V = torch.from_numpy(np.ascontiguousarray(np.stack([v.T for v in Vh]), dtype=dt)).cuda()  # [B][N1][P1]
        handles, keep = None, []
        try:
            if Chats is not None:
                arr = (ctypes.c_void_p * self.B)()
                cache = {}
                for b, c in enumerate(Chats):
                    if c is None or isinstance(c, StateMap):
                        arr[b] = None
                        continue
                    if c.shape != (self.cfsms[b].S1, P1):
                        raise _lib.DimensionMismatch(-2, f"C_hat {b} is {c.shape}, expected {(self.cfsms[b].S1, P1)}")
                    if id(c) not in cache:
                        hm = ctypes.c_void_p()
                        ip, ix, dv = (np.ascontiguousarray(c.indptr, dtype=np.int64), np.ascontiguousarray(c.indices, dtype=np.int64),
                                      np.ascontiguousarray(c.data, dtype=np.float64))
                        check(lib.mm_statemap_create(SEMIRING_ID[self.semiring], c.shape[0], c.shape[1], ix.shape[0], 8, 0, 8,
                                                     ip.ctypes.data, ix.ctypes.data, dv.ctypes.data, ctypes.byref(hm)))
                        cache[id(c)] = hm
                        keep.append(hm)
                    arr[b] = cache[id(c)]
                handles = arr
            gamma, ttl = self.pdfposteriors_ex(V, handles)
            return np.ascontiguousarray(gamma.cpu().numpy().transpose(0, 2, 1)), ttl.cpu().numpy()  # (waits for the kernel)
        finally:
            torch.cuda.current_stream().synchronize()  # the call is asynchronous: the maps must outlive it
            for hm in keep:
                lib.mm_statemap_destroy(hm)

    def _export(self, fn, V, lens):
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        out = torch.empty((N + 1, self.total_states), dtype=torch.float32, device=Vt.device)
        check(fn(*_head(self._h, Vt, lt, N), out.data_ptr(), out.stride(0), self._stream(torch)))
        out = out.t()  # (sum S1) x (N+1) like the reference's state_A / state_B
        return out.cpu().numpy() if as_numpy else out

    def arcposteriors(self, V, lens=None, want_init=False):
        """Expected arc counts (mm_arcposteriors_f32): ``(counts[B, max nnz], ttl[B])``, plus ``init[B, max n_init]`` when
        ``want_init``.  ``counts[b, k]`` is the expected number of times utterance b takes the k-th stored entry of its FSM's
        ``T_hat`` (the CSC data order of ``FSM.nzval``, phony final column and self-loop included), ``init[b, m]`` the posterior
        of the m-th initial state (``FSM.alpha_idx`` order); entries beyond an FSM's own are 0.  ``ttl`` = log Z, as
        ``pdfposteriors`` returns it.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        K = max(c.fsm.nnz for c in self.cfsms)
        counts = torch.zeros((B, K), dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        init = None
        if want_init:
            I = max(1, max(len(c.fsm.alpha_idx) for c in self.cfsms))
            init = torch.zeros((B, I), dtype=torch.float32, device=Vt.device)
        check(lib.mm_arcposteriors_f32(*_head(self._h, Vt, lt, N), counts.data_ptr(), counts.stride(0), _ptr(init),
                                       init.stride(0) if init is not None else 0, ttl.data_ptr(), self._stream(torch)))
        return _results((counts, ttl) + ((init,) if want_init else ()), as_numpy)

    def set_arc_classes(self, classes, C=None):
        """The class of every stored entry of ``T_hat`` for ``arcclassposteriors`` (mm_batch_set_arc_classes): ``classes`` is one
        int array of ``nnz`` ids for a batch of one shared FSM, or a list with one array per utterance; ids in ``[-1, C)``, -1 = not
        counted, in the order of ``FSM.nzval`` (phony final column and self-loop included).  ``C`` defaults to the largest id + 1.
        Host work only; calling it again replaces the plan.  Not during a stream capture.  Returns C."""
        return self._set_classes(lib.mm_batch_set_arc_classes, "set_arc_classes", classes, C)

    def set_path_classes(self, classes, C=None):
        """The class of every stored entry of ``T_hat`` for ``classpath`` (mm_batch_set_path_classes): the arguments of
        ``set_arc_classes``, on a tropical batch; at most 65534 classes.  Host work only; calling it again replaces the plan.  Not
        during a stream capture.  Returns C."""
        return self._set_classes(lib.mm_batch_set_path_classes, "set_path_classes", classes, C)

    def _set_classes(self, setter, who, classes, C):
        """(the two class setters: one array for a shared FSM or one per utterance, flattened with offsets)"""
        torch = _torch()
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.MarkovModelsAMDError(-1, f"{who}: the class plan cannot be replaced during a stream capture")
        shared = not isinstance(classes, (list, tuple))
        arrs = [np.ascontiguousarray(c, dtype=np.int32).ravel() for c in ([classes] if shared else classes)]
        if not shared and len(arrs) != self.B:
            raise _lib.DimensionMismatch(-2, f"need one class array per utterance: got {len(arrs)} for B={self.B}")
        if C is None:
            C = max(1, max((int(a.max()) + 1 for a in arrs if a.size), default=1))
        if shared:
            if arrs[0].size != self.cfsms[0].fsm.nnz:
                raise _lib.DimensionMismatch(-2, f"classes has {arrs[0].size} ids, the FSM {self.cfsms[0].fsm.nnz} entries")
            check(setter(self._h, arrs[0].ctypes.data, None, int(C)))
        else:
            flat = np.ascontiguousarray(np.concatenate(arrs), dtype=np.int32)
            offs = np.cumsum([0] + [a.size for a in arrs]).astype(np.int64)
            check(setter(self._h, flat.ctypes.data, offs.ctypes.data, int(C)))
        return int(C)

    def path_class_info(self) -> dict:
        """``path_C`` = the classes of the plan ``set_path_classes`` gave (0: none), ``path_class_cap`` = the most classes whose
        score rows ``classpath`` takes (mm_batch_path_class_info).  Tropical batches only."""
        c, cap = C.c_int32(), C.c_int64()
        check(lib.mm_batch_path_class_info(self._h, C.byref(c), C.byref(cap)))
        return dict(path_C=c.value, path_class_cap=cap.value)

    def info(self, scored=False, classcost=False) -> dict:
        """What the batch knows about its arc-class plan (mm_batch_arc_class_info): ``arcclass_cap`` = the most classified entries
        of one utterance whose per-frame terms ``arcclassposteriors`` keeps in LDS (beyond it: in the workspace), ``arcclass_max_M``
        = the most any utterance of the current plan has (-1: no plan), ``arcclass_C``.  With ``scored`` also ``score_class_cap`` = the most
        classes ``scoredposteriors`` takes (mm_batch_score_class_cap: their score rows fit the LDS beside the kernel's plan); the
        plain call keeps the three keys it has always had.  With ``classcost`` also ``cost_class_cap`` = the most classes ``classcost``
        takes (mm_batch_cost_class_cap: their cost rows fit the LDS behind the cost kernels' plan).  Log batches only."""
        cap, m, c = C.c_int64(), C.c_int64(), C.c_int32()
        check(lib.mm_batch_arc_class_info(self._h, C.byref(cap), C.byref(m), C.byref(c)))
        out = dict(arcclass_cap=cap.value, arcclass_max_M=m.value, arcclass_C=c.value)
        if scored:
            sc = C.c_int64()
            check(lib.mm_batch_score_class_cap(self._h, C.byref(sc)))
            out["score_class_cap"] = sc.value
        if classcost:
            cc = C.c_int64()
            check(lib.mm_batch_cost_class_cap(self._h, C.byref(cc)))
            out["cost_class_cap"] = cc.value
        return out

    def arcclassposteriors(self, V, lens=None):
        """Per-frame arc-class posteriors (mm_arcclassposteriors_f32), Baum-Welch's xi_n summed by the classes ``set_arc_classes``
        gave: ``(xi[B, C, N], ttl[B])``.  ``xi[b, c, t]`` is the posterior probability that utterance b takes an arc of class c between
        frames t and t + 1 (0-based; t = len - 1: an arc into the phony final state; t >= len: the phony self-loop, exactly 1.0 for
        its class and 0.0 elsewhere).  The result is a view of a ``[B, N, C]`` buffer (a frame's classes are adjacent in memory).
        No atomics: bit-identical from call to call.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        nc = max(1, self.info()["arcclass_C"])  # (no plan: the library refuses the call)
        buf = torch.empty((B, N, nc), dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_arcclassposteriors_f32(*_head(self._h, Vt, lt, N), buf.data_ptr(), *buf.stride(), ttl.data_ptr(), self._stream(torch)))
        xi, ttl = _results((buf.permute(0, 2, 1), ttl), as_numpy)
        return (np.ascontiguousarray(xi) if as_numpy else xi), ttl

    def scoredposteriors(self, V, U=None, lens=None, want_gamma=True, want_xi=True, out=None):
        """Posteriors with per-frame arc-class scores (mm_scoredposteriors_f32): ``(gamma[B, N, P], xi[B, C, N], ttl[B])``; what
        ``want_gamma`` / ``want_xi`` do not ask for comes back as None and is not computed.  Under the classes ``set_arc_classes``
        gave, the entry taken between frames t and t + 1 (0-based; t = len - 1: the arc into the phony final state) is weighted by
        ``exp(U[b, t, class])`` on top of its own weight: ``U`` is ``[B, N, C]`` float32 on the device, finite or -inf (-inf removes
        the class at that transition; rows t >= len are not read), None: no scores.  An entry of class -1 and the phony self-loop are
        not scored.  ``ttl`` = log Z(U), ``gamma = d ttl / d V`` (zeros for n >= len), ``xi[b, c, t] = d ttl / d U[b, t, c]`` for
        t < len and what ``arcclassposteriors`` returns beyond; ``xi`` is a view of a ``[B, N, C]`` buffer.  With ``U`` None
        ``xi``, ``ttl`` are those of ``arcclassposteriors`` and ``gamma`` that of ``pdfposteriors``, from one forward pass.  ``out``:
        a [B, N, P] view gamma is written to with its own strides.  No atomics: bit-identical from call to call.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        nc = max(1, self.info()["arcclass_C"])  # (no plan: the library refuses the call)
        Ut = _class_scores(U, "U", (B, N, nc), Vt.device)
        if out is not None and not want_gamma:
            raise ValueError("out given with want_gamma=False")
        gamma = _out_buffer(out, (B, N, P), Vt.device) if want_gamma else None
        buf = torch.empty((B, N, nc), dtype=torch.float32, device=Vt.device) if want_xi else None
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_scoredposteriors_f32(*_head(self._h, Vt, lt, N), _ptr(Ut), *(Ut.stride() if Ut is not None else (0, 0, 0)),
                                          _ptr(gamma), *(gamma.stride() if gamma is not None else (0, 0, 0)),
                                          _ptr(buf), *(buf.stride() if buf is not None else (0, 0, 0)), ttl.data_ptr(), self._stream(torch)))
        gamma, xi, ttl = _results((gamma, None if buf is None else buf.permute(0, 2, 1), ttl), as_numpy)
        return gamma, (np.ascontiguousarray(xi) if as_numpy and xi is not None else xi), ttl

    def weightedposteriors(self, V, W=None, W_init=None, lens=None, want_gamma=True, want_counts=True, want_init=False, out=None):
        """Posteriors with call-time arc weights (mm_weightedposteriors_f32): ``(gamma[B, N, P], counts[B, max nnz], ttl[B])``, plus
        ``init[B, max n_init]`` with ``want_init``; what ``want_gamma`` / ``want_counts`` do not ask for comes back as None.  The
        topology and every compiled form stay the batch's; ``W`` holds the natural-log weight of every stored entry of ``T_hat``
        (the order of ``FSM.nzval``, which ``counts`` uses), ``W_init`` that of every stored entry of ``alpha_hat``
        (``FSM.alpha_idx`` order), both float32 on the device, finite or -inf (-inf: the entry is absent for this call).  A 1-D
        tensor is one vector for the whole batch (all B handles must be the same FSM), ``[B, >= max nnz]`` a vector per
        utterance; None: the FSMs' own.  The phony self-loop stays one(K) whatever ``W`` holds at its index.  The outputs are
        what ``pdfposteriors`` / ``arcposteriors`` return for FSMs compiled with these weights, so ``counts = d ttl / d W``,
        ``init = d ttl / d W_init`` and ``gamma = d ttl / d V``.  ``out``: a [B, N, P] view gamma is written to with its own
        strides.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        K = max(c.fsm.nnz for c in self.cfsms)
        I = max(1, max(len(c.fsm.alpha_idx) for c in self.cfsms))

        def weights(w, need, name):
            if w is None:
                return None, 0
            wt = w if isinstance(w, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32))
            wt = wt.to(device=Vt.device)
            if wt.dtype != torch.float32:
                raise TypeError(f"{name} must be float32")
            if wt.dim() == 1:
                if wt.numel() < need:
                    raise _lib.DimensionMismatch(-2, f"{name} has {wt.numel()} entries, the FSM has {need}")
                return wt.contiguous(), 0
            if wt.dim() != 2 or wt.shape[0] != B or wt.shape[1] < need:
                raise _lib.DimensionMismatch(-2, f"{name} must be [{need}+] or [B={B}, {need}+], got {tuple(wt.shape)}")
            if wt.stride(1) != 1 or (B > 1 and wt.stride(0) < need):
                wt = wt.contiguous()
            return wt, (wt.stride(0) if B > 1 else max(wt.stride(0), need))

        Wt, wsb = weights(W, K, "W")
        Wi, wisb = weights(W_init, max(len(c.fsm.alpha_idx) for c in self.cfsms), "W_init")
        gamma = _out_buffer(out, (B, N, P), Vt.device) if want_gamma else None
        counts = torch.zeros((B, K), dtype=torch.float32, device=Vt.device) if want_counts else None
        init = torch.zeros((B, I), dtype=torch.float32, device=Vt.device) if want_init else None
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_weightedposteriors_f32(*_head(self._h, Vt, lt, N), _ptr(Wt), wsb, _ptr(Wi), wisb,
                                            _ptr(gamma), *(gamma.stride() if gamma is not None else (0, 0, 0)),
                                            _ptr(counts), K, _ptr(init), I, ttl.data_ptr(), self._stream(torch)))
        return _results((gamma, counts, ttl) + ((init,) if want_init else ()), as_numpy)

    def samplepaths(self, V, lens=None, nsamples=1, seed=0, want_logprob=False):
        """Posterior path samples (mm_samplepaths_f32): ``(paths[B, K, N] int32, ttl[B])``, plus ``logprob[B, K]`` when
        ``want_logprob``.  ``paths[b, k, n]`` is the 0-based state of sample k of utterance b at frame n (-1 for n >= len_b, and
        everywhere for an utterance without a path), drawn from the posterior over complete state sequences; ``logprob`` the
        natural-log posterior probability of each sampled sequence; ``ttl`` = log Z, as ``pdfposteriors`` returns it.  A sample
        depends on (graphs, V, lens, seed) and its indices (b, k) alone: the same seed gives the same samples, the first K' of K
        samples are the samples of a call with K'.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        K = int(nsamples)
        paths = torch.empty((B, max(K, 0), N), dtype=torch.int32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        lp = torch.empty((B, max(K, 0)), dtype=torch.float32, device=Vt.device) if want_logprob else None
        check(lib.mm_samplepaths_f32(*_head(self._h, Vt, lt, N), K, int(seed), paths.data_ptr(), max(K, 0) * N, N,
                                     _ptr(lp), max(K, 0) if lp is not None else 0, ttl.data_ptr(), self._stream(torch)))
        return _results((paths, ttl) + ((lp,) if want_logprob else ()), as_numpy)

    def expectedcost(self, V, cost, lens=None, want_gamma=False):
        """Expected path cost under the path posterior and its gradient (mm_expectedcost_f32): ``(risk[B], grad[B, N, P],
        ttl[B])``, plus ``gamma[B, N, P]`` when ``want_gamma``.  ``cost[b, n, p]`` is what utterance b pays for being in a state
        of pdf p at frame n (finite for n < len_b, not read beyond); ``risk[b]`` the posterior expectation of a path's summed
        cost, ``grad`` its derivative with respect to ``V``, ``gamma`` (the pdf posteriors) its derivative with respect to
        ``cost``; ``ttl`` = log Z, as ``pdfposteriors`` returns it.  With ``cost = -onehot(reference pdfs)`` on the denominator
        graph this is lattice-free sMBR (``mbr.smbr_loss``).  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        Ct = torch.as_tensor(np.ascontiguousarray(cost, dtype=np.float32)).cuda() if not isinstance(cost, torch.Tensor) else cost
        if Ct.dtype != torch.float32 or Ct.device != Vt.device:
            raise TypeError("cost must be a float32 tensor on V's device")
        if tuple(Ct.shape) != (B, N, P):
            raise _lib.DimensionMismatch(-2, f"cost must be [B={B}, N={N}, P={P}], got {tuple(Ct.shape)}")
        if Ct.stride(2) != 1:
            Ct = Ct.contiguous()
        risk = torch.empty(B, dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        grad = torch.empty((B, N, P), dtype=torch.float32, device=Vt.device)
        gamma = torch.empty((B, N, P), dtype=torch.float32, device=Vt.device) if want_gamma else None
        check(lib.mm_expectedcost_f32(*_head(self._h, Vt, lt, N), Ct.data_ptr(), Ct.stride(0), Ct.stride(1), risk.data_ptr(),
                                      grad.data_ptr(), _ptr(gamma), *grad.stride(), ttl.data_ptr(), self._stream(torch)))
        return _results((risk, grad, ttl) + ((gamma,) if want_gamma else ()), as_numpy)

    def classcost(self, V, A, lens=None, D=None, want_gamma=False):
        """Expected arc-class cost under the path posterior and its gradient (mm_classcost_f32): ``(risk[B], grad[B, N, P],
        ttl[B])``, plus ``gamma[B, N, P]`` when ``want_gamma``.  Under the classes ``set_arc_classes`` gave, ``A[b, t, c]``
        (``[B, N, C]`` float32 on the device, any strides) is what utterance b pays for taking an entry of class c between frames t
        and t + 1 (0-based; t = len - 1: the arc into the phony final state); ``D[b, n, p]`` (optional) what it pays for a state of
        pdf p at frame n, exactly ``expectedcost``'s ``cost``.  Both finite where they are read; rows t >= len are not read.  An
        entry of class -1 and the phony self-loop cost nothing.  ``risk[b]`` is the posterior expectation of a path's summed cost,
        ``grad`` its derivative with respect to ``V``, ``gamma`` (the pdf posteriors) its derivative with respect to ``D``; its
        derivative with respect to ``A`` is the xi of ``arcclassposteriors``.  With ``A = -onehot(reference classes)`` on the
        denominator graph this is lattice-free MPE (``mbr.mpe_loss``).  No atomics: bit-identical from call to call.  Log batches
        only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        nc = max(1, self.info()["arcclass_C"])  # (no plan: the library refuses the call)
        At = A if isinstance(A, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(A, dtype=np.float32))
        At = At.to(device=Vt.device)
        if At.dtype != torch.float32:
            raise TypeError("A must be float32")
        if tuple(At.shape) != (B, N, nc):
            raise _lib.DimensionMismatch(-2, f"A must be [B={B}, N={N}, C={nc}], got {tuple(At.shape)}")
        Dt = None
        if D is not None:
            Dt = D if isinstance(D, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(D, dtype=np.float32))
            Dt = Dt.to(device=Vt.device)
            if Dt.dtype != torch.float32:
                raise TypeError("D must be float32")
            if tuple(Dt.shape) != (B, N, P):
                raise _lib.DimensionMismatch(-2, f"D must be [B={B}, N={N}, P={P}], got {tuple(Dt.shape)}")
            if Dt.stride(2) != 1:
                Dt = Dt.contiguous()
        risk = torch.empty(B, dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        grad = _out_buffer(None, (B, N, P), Vt.device)
        gamma = _out_buffer(None, (B, N, P), Vt.device) if want_gamma else None
        check(lib.mm_classcost_f32(*_head(self._h, Vt, lt, N), At.data_ptr(), *At.stride(), _ptr(Dt), *(Dt.stride()[:2] if Dt is not None else (0, 0)),
                                   risk.data_ptr(), grad.data_ptr(), _ptr(gamma), *grad.stride(), ttl.data_ptr(), self._stream(torch)))
        return _results((risk, grad, ttl) + ((gamma,) if want_gamma else ()), as_numpy)

    def pathentropy(self, V, lens=None, want_grad=True, want_gamma=False):
        """Entropy of the posterior over complete paths and its gradient (mm_pathentropy_f32): ``(entropy[B], grad[B, N, P],
        ttl[B])``, plus ``gamma[B, N, P]`` when ``want_gamma``.  ``entropy[b]`` = -sum over the paths of P(path | V_b) ln P(path | V_b)
        in nats, ``grad`` its derivative with respect to ``V`` (``None`` without ``want_grad``), ``gamma`` the pdf posteriors,
        ``ttl`` = log Z as ``pdfposteriors`` returns it.  With neither ``want_grad`` nor ``want_gamma`` only the forward kernel
        runs and no frame is kept: the same ``entropy`` and ``ttl``, bit for bit (confidence scoring).  An utterance without a
        path has entropy 0, gradient 0, ttl = -inf.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        ent = torch.empty(B, dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        grad = torch.empty((B, N, P), dtype=torch.float32, device=Vt.device) if want_grad else None
        gamma = torch.empty((B, N, P), dtype=torch.float32, device=Vt.device) if want_gamma else None
        kept = grad if grad is not None else gamma  # the entry takes ONE set of strides for the two
        assert grad is None or gamma is None or grad.stride() == gamma.stride()
        check(lib.mm_pathentropy_f32(*_head(self._h, Vt, lt, N), ent.data_ptr(), _ptr(grad), _ptr(gamma),
                                     *(kept.stride() if kept is not None else (N * P, P, 1)), ttl.data_ptr(), self._stream(torch)))
        return _results((ent, grad, ttl) + ((gamma,) if want_gamma else ()), as_numpy)

    def leakyposteriors(self, V, lens=None, leak=1e-5, out=None):
        """Pdf posteriors of the leaky HMM (mm_leakyposteriors_f32): ``(gamma[B, N, P], ttl[B])`` as ``pdfposteriors`` returns
        them, with the transition matrix replaced by ``(I + leak * u * pi') * T_hat``: after any frame, from any real state, a
        path may jump with weight ``leak * pi(k)`` to initial state k (``pi`` = the FSM's initial vector as given).  The
        denominator forward-backward of LF-MMI training on chunks: log Z stays finite for an utterance that loses every path
        mid-chunk.  ``leak`` is the linear coefficient (1e-5 .. 0.1 in use; 0 = ``pdfposteriors``); ``out`` as for
        ``pdfposteriors``.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        gamma = _out_buffer(out, (B, N, P), Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_leakyposteriors_f32(*_head(self._h, Vt, lt, N), float(leak), gamma.data_ptr(), *gamma.stride(), ttl.data_ptr(),
                                         self._stream(torch)))
        return _results((gamma, ttl), as_numpy)

    def filterposteriors(self, V, lens=None, state=None, out=None, want_state=False, want_filt=True):
        """Forward filtering posteriors with a carried state (mm_filterposteriors_f32): ``(filt[B, N, P], incr[B, N], ttl[B])``,
        plus ``state_out[total_states]`` when ``want_state``.  ``filt[b, n, p]`` = P(pdf_n = p | V_b at frames 0..n), the causal
        counterpart of ``pdfposteriors``' gamma; ``incr[b, n]`` = ln P(V_n | V_0..n-1), the increments of the prefix
        log-likelihood; ``ttl`` = log Z as ``pdfposteriors`` returns it when ``state`` is None.  ``state`` continues a recursion
        where an earlier call stopped: a float32 device tensor ``[total_states]`` of natural logs, element (b, s) at
        ``state_offsets[b] + s`` -- an earlier call's ``state_out`` (the one-step prediction behind its last frame, its final
        entries the log of the mass the final weights accept); None starts from the FSMs' own initial vectors.  Chunking is
        exact: the ``filt`` and ``incr`` of consecutive chunks are those of one call on the whole, and log Z = the sum of all
        ``incr`` + the last ``state_out``'s final entry (``streaming.ForwardFilter`` keeps that book).  ``lens[b] = 0`` passes
        the state through.  With ``want_filt=False`` ``filt`` is None and not computed: the same ``incr``, ``ttl`` and state,
        bit for bit (likelihood only).  ``want_state`` may also be the tensor that receives the state -- ``state`` itself included:
        a workgroup reads its segment before it writes it.  ``out`` as for ``pdfposteriors``.  Frames beyond the lengths are zeros; from a frame
        without a live state on ``filt`` = 0 and ``incr`` = -inf.  No frame is kept: the call uses no workspace.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        if out is not None and not want_filt:
            raise ValueError("out given with want_filt=False")
        filt = _out_buffer(out, (B, N, P), Vt.device) if want_filt else None
        st = _state_vector(state, "state", self.total_states, Vt.device)
        incr = torch.empty((B, N), dtype=torch.float32, device=Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        so = _want_vector(want_state, "the state buffer", self.total_states, Vt.device)
        check(lib.mm_filterposteriors_f32(*_head(self._h, Vt, lt, N), _ptr(st), _ptr(so),
                                          _ptr(filt), *(filt.stride() if filt is not None else (0, 0, 0)),
                                          incr.data_ptr(), incr.stride(0), ttl.data_ptr(), self._stream(torch)))
        return _results((filt, incr, ttl) + ((so,) if so is not None else ()), as_numpy)

    def windowposteriors(self, V, lens=None, state=None, closed=None, commit=None, out=None, want_state=False):
        """Fixed-lag smoothing posteriors (mm_windowposteriors_f32): the forward-backward over a WINDOW of the audio that starts
        from a carried vector and ends open or on the final weights -- ``(gamma[B, N, P], ttl[B], lcommit[B])``, plus
        ``state_out[total_states]`` when ``want_state``.  ``state`` as for ``filterposteriors`` (None: the FSMs' own initial
        vectors).  ``closed`` (int32 ``[B]``, None: all open): 0 -- the audio goes on behind the window, beta = 1 on every real
        state at the last frame, ``gamma[b, n]`` = P(pdf_n | V_b at the window's frames) and ``ttl`` = ln P(window | start);
        != 0 -- the audio ends with the window, the final weights close it (with ``state`` None: ``pdfposteriors``' gamma and
        log Z).  ``commit`` (int32 ``[B]``, clamped to ``[0, lens[b]]``; None: ``lens``): the frame count c whose one-step
        prediction ``state_out`` is -- ``filterposteriors``' state after c frames -- and ``lcommit`` = ln P(the first c frames |
        start).  Re-windowing is exact: a second window over the frames from c on, with ``state`` = this ``state_out`` and the
        same ``closed``, has this window's gamma on those frames, and its ``ttl`` is this ``ttl`` - ``lcommit``
        (``streaming.FixedLagSmoother`` keeps that book).  ``want_state`` may also be the tensor that receives the state,
        ``state`` itself included.  ``out`` as for ``pdfposteriors``.  Frames beyond the lengths are zeros; a window without
        mass has gamma = 0 and ttl = -inf.  d ttl / d V = gamma.  Log batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        gamma = _out_buffer(out, (B, N, P), Vt.device)
        st = _state_vector(state, "state", self.total_states, Vt.device)
        cl, cm = _per_utt(closed, "closed", B, Vt.device), _per_utt(commit, "commit", B, Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        lcommit = torch.empty(B, dtype=torch.float32, device=Vt.device)
        so = _want_vector(want_state, "the state buffer", self.total_states, Vt.device)
        check(lib.mm_windowposteriors_f32(*_head(self._h, Vt, lt, N), _ptr(st), _ptr(cl), _ptr(cm), _ptr(so), lcommit.data_ptr(),
                                          gamma.data_ptr(), *gamma.stride(), ttl.data_ptr(), self._stream(torch)))
        return _results((gamma, ttl, lcommit) + ((so,) if so is not None else ()), as_numpy)

    def segmentposteriors(self, V, lens=None, state=None, end_mode=None, end=None, out=None, want_end=False):
        """Segment posteriors (mm_segmentposteriors_f32): the forward-backward over a SEGMENT of the audio that starts from a carried
        vector like a window and ends open, on the final weights or on a carried END vector -- ``(gamma[B, N, P], ttl[B], lend[B])``,
        plus ``end_out[total_states]`` when ``want_end``.  ``state`` as for ``filterposteriors`` (None: the FSMs' own initial
        vectors).  ``end_mode`` (int32 ``[B]``, None: all open): 0 -- open, beta = 1 on every real state at the last frame; 2 with
        ``end`` given -- the segment ends on ``end`` (float32 ``[total_states]``, natural log, the layout of ``state``: the
        ``end_out`` of the segment behind this one; the final states' entries are not read); anything else -- the final weights.
        ``end_out`` = ln b_0 - ``lend``, ``lend`` = ln max b_0, b_0 the backward vector one step ahead of the segment's first
        frame: what the segment BEFORE this one ends on.  Chaining is exact: with segment A ending on segment B's ``end_out``
        (B started from the filter's state behind A's frames), A and B have on their frames the gamma of one call over both, and
        ``ttl_A + lend_B`` is that call's ttl (``chunkedposteriors`` keeps that book).  ``want_end`` may also be the tensor that
        receives the end vector -- ``end`` itself included: a workgroup reads its segment before it writes it.  ``out`` as for
        ``pdfposteriors``.  Frames beyond the lengths are zeros; ``lens[b] = 0`` hands the end vector the segment was given back;
        a segment without mass has gamma = 0, ttl = lend = -inf and ``end_out`` = -inf everywhere.  d ttl / d V = gamma.  Log
        batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        gamma = _out_buffer(out, (B, N, P), Vt.device)
        st = _state_vector(state, "state", self.total_states, Vt.device)
        ei = _state_vector(end, "end", self.total_states, Vt.device)
        em = _per_utt(end_mode, "end_mode", B, Vt.device)
        ttl = torch.empty(B, dtype=torch.float32, device=Vt.device)
        lend = torch.empty(B, dtype=torch.float32, device=Vt.device)
        eo = _want_vector(want_end, "the end buffer", self.total_states, Vt.device)
        check(lib.mm_segmentposteriors_f32(*_head(self._h, Vt, lt, N), _ptr(st), _ptr(em), _ptr(ei), _ptr(eo), lend.data_ptr(),
                                           gamma.data_ptr(), *gamma.stride(), ttl.data_ptr(), self._stream(torch)))
        return _results((gamma, ttl, lend) + ((eo,) if eo is not None else ()), as_numpy)

    def chunkedposteriors(self, V, lens=None, chunk=1024, out=None):
        """The exact smoothing posteriors of long recordings in the workspace of ONE chunk: ``(gamma[B, N, P], ttl[B])``, the gamma
        and log Z of ``pdfposteriors`` (of ``windowposteriors`` closed), computed in two passes over chunks of ``chunk`` frames.
        Pass 1 is ``filterposteriors(want_filt=False)`` per chunk -- no frame kept, no workspace --, which saves the start state of
        every chunk (``K x total_states`` floats) and gives ttl by the filter's book, the sum of ``incr`` + the last state's final
        entries.  Pass 2 is ``segmentposteriors`` over the chunks in reverse: chunk k runs ``lens_k = clamp(lens - k chunk, 0,
        chunk)`` frames from its saved state and ends on the final weights where the utterance ends in it or before it
        (``lens <= (k + 1) chunk``), else on the end vector chunk k + 1 handed back; a chunk wholly behind an utterance's end has
        no frame and hands the final weights on.  gamma is written chunk by chunk into ``out``.  No call sees more than ``chunk``
        frames, so the alpha~ store is that of ``chunk`` frames whatever N; ``chunk >= N`` is one segment call.  Launches on the
        caller's stream only, no host synchronisation.  An utterance without an accepting path has gamma = 0 and ttl = -inf."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be at least one frame")
        dev = Vt.device
        gamma = _out_buffer(out, (B, N, P), dev)
        if lt is None:
            lt = torch.full((B,), N, dtype=torch.int32, device=dev)
        if chunk >= N:
            _, ttl, _ = self.segmentposteriors(Vt, lt, end_mode=torch.ones(B, dtype=torch.int32, device=dev), out=gamma)
            return _results((gamma, ttl), as_numpy)
        K = (N + chunk - 1) // chunk
        lens_k = [torch.clamp(lt - k * chunk, 0, chunk).to(torch.int32) for k in range(K)]
        # pass 1: states[k] is the state behind chunk k, the start of chunk k + 1 (chunk 0 starts from the FSMs' own vectors)
        states = torch.empty((K, self.total_states), dtype=torch.float32, device=dev)
        loglik = torch.zeros(B, dtype=torch.float64, device=dev)
        for k in range(K):
            _, incr, _, _ = self.filterposteriors(Vt[:, k * chunk : (k + 1) * chunk], lens_k[k], state=states[k - 1] if k else None,
                                                  want_state=states[k], want_filt=False)
            loglik += incr.sum(dim=1, dtype=torch.float64)
        final = self.__dict__.get("_final_entries")  # (uploaded once per batch and device: no copy from the host in later calls)
        if final is None or final.device != dev:
            final = self._final_entries = torch.as_tensor(self.state_offsets[1:] - 1, dtype=torch.int64, device=dev)
        ttl = (loglik + states[K - 1][final].double()).float()
        # pass 2: the end vector travels backwards in one buffer, read and written in place
        endv = torch.empty(self.total_states, dtype=torch.float32, device=dev)
        for k in range(K - 1, -1, -1):
            mode = torch.where(lt <= (k + 1) * chunk, 1, 2).to(torch.int32)
            self.segmentposteriors(Vt[:, k * chunk : (k + 1) * chunk], lens_k[k], state=states[k - 1] if k else None, end_mode=mode,
                                   end=endv if k < K - 1 else None, out=gamma[:, k * chunk : (k + 1) * chunk], want_end=endv if k else False)
        return _results((gamma, ttl), as_numpy)

    def maxstateposteriors(self, V, lens=None):
        """Max-marginals of the tropical semiring, (sum S1) x (N+1), computed on the device."""
        return self._export(lib.mm_maxstateposteriors_f32, V, lens)

    def alpharecursion(self, V, lens=None):
        return self._export(lib.mm_alpharecursion_f32, V, lens)

    def betarecursion(self, V, lens=None):
        return self._export(lib.mm_betarecursion_f32, V, lens)

    def reserve(self, N: int):
        """Size the internal workspace for runs of up to N frames now (so that later calls -- e.g. ones captured in
        a hipGraph -- never reallocate)."""
        check(lib.mm_batch_reserve(self._h, int(N)))

    def set_posterior_floor(self, floor: float = 1e-30):
        """mm_batch_set_posterior_floor: posteriors below `floor` may come out as 0 from the fast kernels (default 1e-30);
        a relaxed floor (1e-12) keeps sharp emissions on the fast path.  Returns self."""
        check(lib.mm_batch_set_posterior_floor(self._h, float(floor)))
        return self

    def set_deterministic(self, on: bool = True):
        """No float atomics in the general kernel: bit-identical gamma on every run (slower on small deep graphs)."""
        check(lib.mm_batch_set_deterministic(self._h, 1 if on else 0))
        return self

    def last_redo_count(self) -> int:
        """Utterances of the last pdfposteriors call that the fast kernels handed to the exact ones (0 = the whole
        batch ran on the fast path).  Synchronises the current stream."""
        import ctypes

        n = ctypes.c_int64(0)
        check(lib.mm_batch_last_redo_count(self._h, self._stream(_torch()), ctypes.byref(n)))
        return int(n.value)

    def last_fallback_count(self) -> int:
        """... and how many of those the float64 exact kernels handed on to the log-domain kernels (normally 0).
        Synchronises the current stream."""
        import ctypes

        n = ctypes.c_int64(0)
        check(lib.mm_batch_last_fallback_count(self._h, self._stream(_torch()), ctypes.byref(n)))
        return int(n.value)

    def set_exact_policy(self, policy: str = "auto"):
        """mm_batch_set_exact_policy: which linear-domain kernels a shared-graph batch starts with -- "auto" (float32 first,
        float64 first while the last finished call left utterances marked: depends on host / device timing for pipelined
        callers), "f32_first" or "f64_first" (both: the launches of a call are a function of the call alone, identical call
        sequences give identical bits).  Pins the path of ``alpharecursion`` / ``betarecursion`` as well ("auto": the item kernel
        first while the last export handed it more than half of the utterances; "f64_first": the item kernel alone)."""
        pol = {"auto": _lib.MM_EXACT_AUTO, "f32_first": _lib.MM_EXACT_F32_FIRST, "f64_first": _lib.MM_EXACT_F64_FIRST}[policy]
        check(lib.mm_batch_set_exact_policy(self._h, pol))
        return self

    def set_mark_policy(self, policy: str = "decide"):
        """mm_batch_set_mark_policy: "decide" (default: the finish kernel clears a range mark of the float32 kernels when its two
        criteria hold -- log gamma within 1e-4 relative above ~1e-24, an absolute error below ~1e-27 for smaller posteriors) or "keep"
        (a range mark always stays: the exact kernels compute the utterance -- the relative bar down to 1e-30)."""
        check(lib.mm_batch_set_mark_policy(self._h, {"decide": _lib.MM_MARKS_DECIDE, "keep": _lib.MM_MARKS_KEEP}[policy]))
        return self

    def set_gamma_mode(self, accumulate: bool = False, scale: float = 1.0):
        """mm_batch_set_gamma_mode: what pdfposteriors writes -- gamma_out = scale * gamma, or (accumulate) gamma_out += scale * gamma
        into the ``out`` tensor of the call (frames beyond the lengths left alone).  Batches of the wave kernel (numerator graphs)
        only: MarkovModelsAMDError(-4) otherwise.  The LF-MMI gradient gamma_den - gamma_num without a third pass (lfmmi.py)."""
        check(lib.mm_batch_set_gamma_mode(self._h, 1 if accumulate else 0, float(scale)))
        return self

    def last_exact_first(self) -> bool:
        """True if the last pdfposteriors call skipped the float32 kernels (the inputs of the call before were hard: the
        float64 exact kernels then run the whole batch at once)."""
        return bool(lib.mm_batch_last_exact_first(self._h))

    def team_xcd_stats(self):
        """(workgroups of the team kernels' launches since the last call of this method whose whole team sat on ONE XCD, all
        such workgroups): how the hardware placed the teams (a measurement aid; synchronises the device)."""
        out = np.zeros(2, dtype=np.int32)
        check(lib.mm_batch_team_xcd_stats(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def kernels(self, semiring: str = "log") -> str:
        """The kernels the engine launches for this batch (informational): "log" = pdfposteriors, "tropical" = bestpath, "export" =
        alpharecursion / betarecursion, "arcs" = arcposteriors, "sample" = samplepaths, "cost" = expectedcost, "leaky" =
        leakyposteriors, "entropy" = pathentropy, "filter" = filterposteriors, "window" = windowposteriors,
        "vitwindow" = viterbiwindow (tropical batches), "weighted" = weightedposteriors, "segment" = segmentposteriors,
        "classpath" = classpath (tropical batches), "lattice" = lattice (tropical batches), "latticeposteriors" = latticeposteriors
        (tropical batches), "latticecost" = latticecost (tropical batches), "latticebest" = latticebest (tropical batches), "latticesample" =
        latticesample (tropical batches)."""
        import ctypes

        buf = ctypes.create_string_buffer(1024)
        check(lib.mm_batch_kernels(self._h, {"log": 0, "tropical": 1, "export": 3, "arcs": 4, "sample": 5, "cost": 6, "leaky": 7, "entropy": 8, "filter": 9, "window": 10, "vitwindow": 11, "weighted": 12, "segment": 13, "arcclass": 14, "scored": 15, "classcost": 16, "classpath": 17, "lattice": 18, "latticeposteriors": 19, "latticecost": 20, "latticebest": 21, "latticesample": 22}[semiring], buf, 1024))
        return buf.value.decode()

    def kernels_generic(self) -> str:
        """What the last call of the generic entry (mm_pdfposteriors_ex) launched for this batch (informational)."""
        import ctypes

        buf = ctypes.create_string_buffer(1024)
        check(lib.mm_batch_kernels(self._h, 2, buf, 1024))
        return buf.value.decode()

    def viterbi(self, V, lens=None, return_backpointers=False):
        """Best paths: (path[B, N] 0-based states, -1 beyond len; score[B][, bp[N+1, sum S1]])."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        path = torch.empty((B, N), dtype=torch.int32, device=Vt.device)
        score = torch.empty(B, dtype=torch.float32, device=Vt.device)
        bp = torch.empty((N + 1, self.total_states), dtype=torch.int32, device=Vt.device) if return_backpointers else None
        check(lib.mm_viterbi_f32(*_head(self._h, Vt, lt, N), path.data_ptr(), path.stride(0), score.data_ptr(), _ptr(bp),
                                 bp.stride(0) if bp is not None else 0, self._stream(torch)))
        return _results((path, score) + ((bp,) if bp is not None else ()), as_numpy)

    def viterbiwindow(self, V, lens=None, state=None, closed=None, commit=None, commit_converged=False, want_state=False):
        """Windowed best paths (mm_viterbiwindow_f32): the Viterbi recursion over a WINDOW of the audio that starts from a carried
        vector and ends open or in the final state -- ``(path[B, N], score[B], converged[B], ncommit[B], mcommit[B], state_out)``;
        ``state_out[total_states]`` is None without ``want_state``.  ``state`` is an earlier call's ``state_out`` (float32
        ``[total_states]``, natural log, element (b, s) at ``state_offsets[b] + s``); None starts from the FSMs' own initial vectors.
        ``closed`` (int32 ``[B]``, None: all open): 0 -- the audio goes on behind the window, the path ends in the best real state of
        the last frame; != 0 -- the audio ends with the window, the path ends in the final state (with ``state`` None: ``viterbi``'s
        path and score, bit for bit).  ``converged[b]`` is the convergence point: the last frame count n at which every surviving
        path passes ONE state -- ``path[b, :n]`` is final, whatever audio follows (0: none yet).  ``commit`` (int32 ``[B]``, clamped to
        ``[0, lens[b]]``; None: ``lens``, or 0 with ``commit_converged``) is the frame count c that ``state_out`` and ``mcommit``
        (the largest score of a path over the first c frames, taken off ``state_out``) belong to; ``commit_converged`` raises it to
        ``converged`` where that is later; ``ncommit`` returns it.  Re-windowing: a second window over the frames from c on, with
        ``state`` = this ``state_out`` and the same ``closed``, continues this path and scores ``score - mcommit``
        (``streaming.OnlineViterbi`` keeps that book).  ``want_state`` may also be the tensor that receives the state, ``state``
        itself included.  ``path`` is -1 beyond the lengths and where there is no path.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        st = _state_vector(state, "state", self.total_states, Vt.device)
        cl, cm = _per_utt(closed, "closed", B, Vt.device), _per_utt(commit, "commit", B, Vt.device)
        path = torch.empty((B, N), dtype=torch.int32, device=Vt.device)
        score = torch.empty(B, dtype=torch.float32, device=Vt.device)
        conv = torch.empty(B, dtype=torch.int32, device=Vt.device)
        ncommit = torch.empty(B, dtype=torch.int32, device=Vt.device)
        mcommit = torch.empty(B, dtype=torch.float32, device=Vt.device)
        so = _want_vector(want_state, "the state buffer", self.total_states, Vt.device)
        check(lib.mm_viterbiwindow_f32(*_head(self._h, Vt, lt, N), _ptr(st), _ptr(cl), _ptr(cm), 1 if commit_converged else 0, _ptr(so),
                                       mcommit.data_ptr(), ncommit.data_ptr(), path.data_ptr(), path.stride(0), score.data_ptr(),
                                       conv.data_ptr(), self._stream(torch)))
        return _results((path, score, conv, ncommit, mcommit, so), as_numpy)

    def classpath(self, V, U=None, lens=None, want_classes=True):
        """Best paths that report arc classes, under per-frame arc-class scores (mm_classpath_f32): ``(path[B, N], classes[B, N],
        score[B])``; ``classes`` is None without ``want_classes``.  Under the classes ``set_path_classes`` gave, the entry taken
        between frames t and t + 1 (0-based; t = len - 1: the arc into the phony final state) adds ``U[b, t, class]`` to its own
        weight: ``U`` is ``[B, N, C]`` float32 on the device, finite or -inf (-inf removes the class at that transition; rows
        t >= len are not read), None: no scores -- ``path`` and ``score`` are then ``viterbi``'s, bit for bit.  An entry of class -1
        and the phony self-loop are not scored.  ``classes[b, t]`` is the class of the entry the best path takes at transition t
        (-1: an unclassified entry); among several best arcs into a state the lowest source wins, then the lowest class id, -1
        last.  ``path`` and ``classes`` are -1 beyond the lengths and where there is no path (``score`` = -inf).  Without a plan
        only ``U`` None with ``want_classes`` False is accepted.  No atomics: bit-identical from call to call.  Tropical batches
        only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        Ut = _class_scores(U, "U", (B, N, max(1, self.path_class_info()["path_C"])), Vt.device) if U is not None else None
        path = torch.empty((B, N), dtype=torch.int32, device=Vt.device)
        cls = torch.empty((B, N), dtype=torch.int32, device=Vt.device) if want_classes else None
        score = torch.empty(B, dtype=torch.float32, device=Vt.device)
        check(lib.mm_classpath_f32(*_head(self._h, Vt, lt, N), _ptr(Ut), *(Ut.stride() if Ut is not None else (0, 0, 0)), path.data_ptr(),
                                   path.stride(0), _ptr(cls), cls.stride(0) if cls is not None else 0, score.data_ptr(), self._stream(torch)))
        return _results((path, cls, score), as_numpy)

    def lattice(self, V, beam, lens=None, max_arcs=None):
        """Beam-pruned best-path lattices (mm_lattice_f32): a ``Lattice`` of ``counts[B, N]``, ``offsets[B * N + 1]``, ``arc``,
        ``score`` and ``best[B]``.  For every utterance b and transition t (0-based, between frames t and t + 1; t = len - 1: the arc
        into the phony final state) it lists the stored entries k of the FSM -- in ``arcposteriors``' entry order, ascending -- that lie
        on a complete path weighing at least ``best[b] - beam[b]``, each with its through-score minus ``best[b]``.  ``beam`` is a
        number or a ``[B]`` tensor, natural log; negative or NaN keeps nothing, inf keeps every arc on any complete path.  On
        unrounded inputs the scores carry float32 rounding of about ``(N + 3) * 2**-24 * max|alpha|``: a beam of 0 is not meaningful
        there.  ``max_arcs`` None: the method makes the count-only call, READS THE TOTAL BACK (one host synchronisation), allocates
        exactly, and calls again.  ``max_arcs`` given: one call into buffers of that many records and no synchronisation until the
        total is compared -- ``MarkovModelsAMDError`` if it exceeds ``max_arcs``; inside a stream capture the comparison is left out
        (records beyond ``max_arcs`` are never written; compare ``offsets[-1]`` after the replay), which makes this the capturable
        form.  ``decode.lattice_arcs`` / ``decode.lattice_fsm`` read one utterance off the result.  No atomics: bit-identical from
        call to call.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        dev = Vt.device
        bt = _beam_vector(beam, B, dev)
        cap = _record_cap(max_arcs)
        counts = torch.empty((B, N), dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        best = torch.empty(B, dtype=torch.float32, device=dev)

        def call(arc, score, n):
            check(lib.mm_lattice_f32(*_head(self._h, Vt, lt, N), bt.data_ptr(), counts.data_ptr(), counts.stride(0), total.data_ptr(),
                                     best.data_ptr(), _ptr(arc), _ptr(score), n, self._stream(torch)))

        capturing = torch.cuda.is_current_stream_capturing()
        if cap is None:
            call(None, None, 0)
            cap = int(total.item())
        arc = torch.empty(cap, dtype=torch.int32, device=dev)
        score = torch.empty(cap, dtype=torch.float32, device=dev)
        call(arc, score, cap)
        if max_arcs is not None and not capturing:
            n = int(total.item())
            if n > cap:
                raise _lib.MarkovModelsAMDError(-1, f"lattice: {n} arcs are within the beam, max_arcs is {cap}")
            arc, score = arc[:n], score[:n]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)])
        return Lattice(*_results((counts, offsets, arc, score, best), as_numpy))

    def _lattice_inputs(self, who, torch, lat, Vt, extra):
        """The checks of the entries that read a lattice: ``(offsets, arc, nrec, extra)`` as contiguous tensors on V's device
        (``extra`` None as it is).  DimensionMismatch for offsets that are not [B * N + 1], an ``arc`` that is no vector and an
        ``extra`` of another length; ValueError when ``lat.arc`` holds fewer records than ``lat.offsets[-1]`` (one read-back, left
        out inside a stream capture)."""
        B, N, _ = Vt.shape
        dev = Vt.device
        offsets = _on_device(lat.offsets, torch.int64, dev)
        arc = _on_device(lat.arc, torch.int32, dev)
        if offsets.dim() != 1 or offsets.numel() != B * N + 1:
            raise _lib.DimensionMismatch(-2, f"lat.offsets must be [B * N + 1 = {B * N + 1}], got {tuple(offsets.shape)}")
        nrec = arc.numel()
        if arc.dim() != 1:
            raise _lib.DimensionMismatch(-2, f"lat.arc must be a vector, got {tuple(arc.shape)}")
        et = None
        if extra is not None:
            et = _on_device(extra, torch.float32, dev)
            if et.dim() != 1 or et.numel() != nrec:
                raise _lib.DimensionMismatch(-2, f"extra must be [{nrec}], one score per record, got {tuple(et.shape)}")
        if not torch.cuda.is_current_stream_capturing():
            total = int(offsets[-1].item())
            if total > nrec:
                raise ValueError(f"{who}: the lattice has {total} records, lat.arc holds {nrec} (max_arcs cut it)")
        return offsets, arc, nrec, et

    def latticebest(self, lat, V, lens=None, extra=None, want_path=True):
        """Lattice best paths (mm_latticebest_f32), the tropical twin of ``latticeposteriors``: over the records of ``lat`` -- a
        ``Lattice`` of ``BatchedFSM.lattice`` on this batch, or a subset of one -- under the emissions ``V`` of THIS call and an
        optional score ``extra`` per record (a rescoring).  Returns ``LatticeBest(best, score, rec, path)``: ``best[B]`` the weight of
        the best path (-inf: none), ``score`` float32 per record, the best path through the record minus ``best`` (-inf: none),
        ``rec[B, N]`` int64 the best path's record of every transition (an index into ``lat.arc``; ties go to the lowest record) and
        ``path[B, N]`` int32 the source state of that record, ``bestpath``'s convention; both -1 at and behind ``len`` and without a
        path, both None with ``want_path=False``.  ``extra[r] = -inf`` removes record r.  ``decode.lattice_rescore`` re-prunes the
        lattice by ``score``, ``decode.lattice_onebest`` reads one utterance's best path.  Inputs and results as ``latticeposteriors``
        handles them, its ValueError for a lattice cut by ``max_arcs`` included.  Adds and integer maxima only: bit-identical from
        call to call.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        dev = Vt.device
        offsets, arc, nrec, et = self._lattice_inputs("latticebest", torch, lat, Vt, extra)
        best = torch.empty(B, dtype=torch.float32, device=dev)
        score = torch.empty(nrec, dtype=torch.float32, device=dev)
        rec = torch.empty((B, N), dtype=torch.int64, device=dev) if want_path else None
        path = torch.empty((B, N), dtype=torch.int32, device=dev) if want_path else None
        check(lib.mm_latticebest_f32(*_head(self._h, Vt, lt, N), offsets.data_ptr(), arc.data_ptr(), nrec, _ptr(et), best.data_ptr(), score.data_ptr(),
                                     _ptr(rec), N, _ptr(path), N, self._stream(torch)))
        return LatticeBest(*_results((best, score, rec, path), as_numpy))

    def latticesample(self, lat, V, nsamples, seed=0, lens=None, extra=None, want_path=True, want_logprob=True):
        """Lattice path sampling (mm_latticesample_f32): ``nsamples`` independent draws per utterance from the posterior over the
        RECORD sequences of ``lat`` -- a ``Lattice`` of ``BatchedFSM.lattice`` on this batch, or a subset of one -- under the
        emissions ``V`` of THIS call and an optional score ``extra`` per record; parallel entries between two states are separate
        outcomes.  Returns ``LatticeSamples(rec, path, logprob, logz)``: ``rec[B, K, N]`` int64 the records (indices into
        ``lat.arc``), ``path[B, K, N]`` int32 their source states (None with ``want_path=False``), both -1 at and behind ``len`` and
        without a path; ``logprob[B, K]`` the log posterior of each sample (None with ``want_logprob=False``; -inf without a path);
        ``logz[B]`` as ``latticeposteriors`` returns it.  A sample is a function of the lattice, ``V``, ``extra``, ``lens``,
        ``seed``, its utterance's POSITION b and its index k alone: the first samples of a larger call are those of a smaller one,
        a repeated call returns the same bits, and equal utterances at different positions get different samples.  A record with
        ``extra = -inf`` is never drawn.  The costs of the samples (an edit distance, say) go into
        ``lattices.lattice_sampled_risk``.  Inputs and results as ``latticeposteriors`` handles them, its ValueError for a lattice
        cut by ``max_arcs`` included.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        dev = Vt.device
        offsets, arc, nrec, et = self._lattice_inputs("latticesample", torch, lat, Vt, extra)
        K = int(nsamples)
        Ka = max(K, 0)
        fwd = torch.empty(nrec, dtype=torch.float32, device=dev)
        rec = torch.empty((B, Ka, N), dtype=torch.int64, device=dev)
        path = torch.empty((B, Ka, N), dtype=torch.int32, device=dev) if want_path else None
        logprob = torch.empty((B, Ka), dtype=torch.float32, device=dev) if want_logprob else None
        logz = torch.empty(B, dtype=torch.float32, device=dev)
        check(lib.mm_latticesample_f32(*_head(self._h, Vt, lt, N), offsets.data_ptr(), arc.data_ptr(), nrec, _ptr(et), K, int(seed), fwd.data_ptr(),
                                       rec.data_ptr(), Ka * N, N, _ptr(path), Ka * N, N, _ptr(logprob), Ka, logz.data_ptr(), self._stream(torch)))
        return LatticeSamples(*_results((rec, path, logprob, logz), as_numpy))

    def latticeposteriors(self, lat, V, lens=None, extra=None, want_gamma=True):
        """Lattice posteriors (mm_latticeposteriors_f32): the log-semiring forward-backward over the records of ``lat`` -- a
        ``Lattice`` of ``BatchedFSM.lattice`` on this batch, or a subset of one (``decode.lattice_prune``) -- under the emissions
        ``V`` of THIS call (a second model's, or the first one's at another scale) and an optional score ``extra`` per record.
        Returns ``LatticePosteriors(post, logz, gamma)``: ``post`` float32 per record, the log posterior of the record among the
        lattice's paths (-inf: no path through it); ``logz[B]`` the lattice's log-sum (-inf: no path); ``gamma[B, N, P]`` the pdf
        occupancies = d logz / d V (``want_gamma=False``: None, and the second kernel does not run); ``exp(post)`` is
        d logz / d extra.  ``lens`` are those of the lattice call.  ``lat``'s members may be tensors or NumPy arrays; the results are
        NumPy arrays if ``V`` came as NumPy.  ValueError when ``lat.arc`` holds fewer records than ``lat.offsets[-1]`` (a lattice
        cut by ``max_arcs``) -- one read-back, left out inside a stream capture.  Integer maxima and fixed-point sums: bit-identical
        from call to call.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        dev = Vt.device
        offsets, arc, nrec, et = self._lattice_inputs("latticeposteriors", torch, lat, Vt, extra)
        post = torch.empty(nrec, dtype=torch.float32, device=dev)
        logz = torch.empty(B, dtype=torch.float32, device=dev)
        gamma = torch.empty((B, N, P), dtype=torch.float32, device=dev) if want_gamma else None
        check(lib.mm_latticeposteriors_f32(*_head(self._h, Vt, lt, N), offsets.data_ptr(), arc.data_ptr(), nrec, _ptr(et), post.data_ptr(),
                                           logz.data_ptr(), _ptr(gamma), gamma.stride(0) if want_gamma else 0, gamma.stride(1) if want_gamma else 0,
                                           self._stream(torch)))
        return LatticePosteriors(*_results((post, logz, gamma), as_numpy))

    def latticecost(self, lat, V, cost, lens=None, extra=None, want_grad=True, want_gamma=False):
        """Lattice expected cost (mm_latticecost_f32): the expectation of ``A(path) = sum of cost[r]`` over the paths of ``lat``,
        weighed as ``latticeposteriors`` weighs them under ``V`` and ``extra``, and its gradient -- lattice-based sMBR / MPE.
        ``cost`` is one float32 per record, finite.  Returns ``LatticeCost(risk, diff, post, logz, grad, gamma)``: ``risk[B]`` (0 for
        an utterance without a path), ``diff`` per record = d risk / d extra, ``post`` / ``logz`` / ``gamma`` bit for bit those of
        ``latticeposteriors``, ``grad[B, N, P]`` = d risk / d V (``want_grad=False`` / ``want_gamma=False``: None; with both off the
        second kernel does not run); ``exp(post)`` is d risk / d cost.  Inputs and results as ``latticeposteriors`` handles them,
        its ValueError for a lattice cut by ``max_arcs`` included.  Bit-identical from call to call.  Tropical batches only."""
        torch, Vt, lt, as_numpy = self._prep(V, lens)
        B, N, P = Vt.shape
        dev = Vt.device
        offsets = _on_device(lat.offsets, torch.int64, dev)
        arc = _on_device(lat.arc, torch.int32, dev)
        if offsets.dim() != 1 or offsets.numel() != B * N + 1:
            raise _lib.DimensionMismatch(-2, f"lat.offsets must be [B * N + 1 = {B * N + 1}], got {tuple(offsets.shape)}")
        nrec = arc.numel()
        if arc.dim() != 1:
            raise _lib.DimensionMismatch(-2, f"lat.arc must be a vector, got {tuple(arc.shape)}")
        ct = _on_device(cost, torch.float32, dev)
        if ct.dim() != 1 or ct.numel() != nrec:
            raise _lib.DimensionMismatch(-2, f"cost must be [{nrec}], one cost per record, got {tuple(ct.shape)}")
        et = None
        if extra is not None:
            et = _on_device(extra, torch.float32, dev)
            if et.dim() != 1 or et.numel() != nrec:
                raise _lib.DimensionMismatch(-2, f"extra must be [{nrec}], one score per record, got {tuple(et.shape)}")
        if not torch.cuda.is_current_stream_capturing():
            total = int(offsets[-1].item())
            if total > nrec:
                raise ValueError(f"latticecost: the lattice has {total} records, lat.arc holds {nrec} (max_arcs cut it)")
        risk = torch.empty(B, dtype=torch.float32, device=dev)
        diff = torch.empty(nrec, dtype=torch.float32, device=dev)
        post = torch.empty(nrec, dtype=torch.float32, device=dev)
        logz = torch.empty(B, dtype=torch.float32, device=dev)
        grad = torch.empty((B, N, P), dtype=torch.float32, device=dev) if want_grad else None
        gamma = torch.empty((B, N, P), dtype=torch.float32, device=dev) if want_gamma else None
        check(lib.mm_latticecost_f32(*_head(self._h, Vt, lt, N), offsets.data_ptr(), arc.data_ptr(), nrec, _ptr(et), ct.data_ptr(), risk.data_ptr(),
                                     diff.data_ptr(), post.data_ptr(), logz.data_ptr(), _ptr(grad), _ptr(gamma), N * P, P, self._stream(torch)))
        return LatticeCost(*_results((risk, diff, post, logz, grad, gamma), as_numpy))

    def totalsum(self, n: int, cumulative: bool = False):
        """Per FSM of the batch: omega . v_n (totalsum) or the semiring sum over k <= n of omega . v_k
        (totalcumsum), v_1 = alpha, v_k = T' v_{k-1} (src/algorithms.jl:8-29).  float32 tensor [B]."""
        torch = _torch()
        out = torch.empty(self.B, dtype=torch.float32, device="cuda")
        check(lib.mm_totalsum_f32(self._h, int(n), int(bool(cumulative)), out.data_ptr(), self._stream(torch)))
        return out


def batch(*cfsms: CompiledFSM) -> BatchedFSM:
    """batch(fsm1, fsms...) (src/inference.jl:28-36)."""
    return BatchedFSM(cfsms)


def expand(lhs, seqlength: Optional[int] = None, semiring: str = "log"):
    """expand(V, seqlength) (src/inference.jl:54-60): the P x N likelihoods
    become (P+1) x (N+1): a phony pdf row (zero(K) up to seqlength, one(K) after) and
    an extra frame; real pdfs are zero(K) beyond seqlength.  zero = -inf, one = 0 for the
    Log/Tropical semirings, 0 and 1 for ProbSemiring."""
    a = np.asarray(lhs)
    P, N = a.shape
    L = N if seqlength is None else int(seqlength)
    out = np.full((P + 1, N + 1), _SEM_ZERO[semiring], dtype=a.dtype if a.dtype.kind == "f" else np.float32)
    out[:P, :L] = a[:, :L]
    out[P, L:] = _SEM_ONE[semiring]
    return out


def _unexpand(Vhats: Sequence[np.ndarray], semiring: str = "log"):
    """Recover (V[B, N, P], lens) from matrices made by ``expand`` (what the fast kernels take: they implement expand's
    semantics themselves); None if a matrix is not of that form -- the caller then takes the generic path.  The form
    (src/inference.jl:54-60): the phony row zero(K) up to the length and one(K) after, the real rows zero(K) beyond it --
    zero(K) / one(K) = -inf / 0 for the Log and Tropical semirings, 0 / 1 for ProbSemiring."""
    Vh = [np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in Vhats]
    shp = Vh[0].shape
    if any(v.shape != shp for v in Vh):
        raise _lib.DimensionMismatch(-2, "all V_hat must share one (P+1) x (N+1) shape")
    P1, N1 = shp
    zero, one = _SEM_ZERO[semiring], _SEM_ONE[semiring]
    lens = []
    for v in Vh:
        ph = v[P1 - 1]
        L = int(np.argmax(ph == one)) if (ph == one).any() else N1
        ok = np.all(ph[:L] == zero) and np.all(ph[L:] == one) and np.all(v[: P1 - 1, L:] == zero) and L <= N1 - 1
        if not ok:
            return None
        lens.append(L)
    V = np.stack([v[: P1 - 1, : N1 - 1].T for v in Vh]).astype(np.float32)
    if semiring != "prob":
        V[~np.isfinite(V) & (V < 0)] = -np.inf
    return np.ascontiguousarray(V), np.asarray(lens, dtype=np.int32)


def _need_expanded(Vhats, semiring: str = "log"):
    un = _unexpand(Vhats, semiring)
    if un is None:
        raise ValueError("V_hat is not of the form expand(V, seqlength) produces (only pdfposteriors takes arbitrary V_hat)")
    return un


# ---- compiled graphs of the reference-shaped entries: a process-wide LRU keyed by CONTENT.  `pdfposteriors(fsm::FSM, V_hats,
# C_hats)` (src/inference.jl:145-161) takes plain FSMs and transposes / re-batches them on every call (:148-151); here a graph
# is compiled (packed into the kernels' forms, uploaded) the first time its content is seen and found again by a 128-bit hash of
# its fields afterwards -- the denominator graph of every call, the numerator graphs of an utterance across epochs.  Misses of
# one call are compiled together (compile_many: host threads, one allocation, one copy).
_COMPILED_LRU: "OrderedDict[bytes, CompiledFSM]" = None  # type: ignore[assignment]
_COMPILED_LRU_MAX = 8192            # entries ...
_COMPILED_LRU_MAX_BYTES = 16 << 30  # ... and an estimate of the device bytes their kernel forms hold (large graphs pin a lot of HBM each)
_COMPILED_LRU_BYTES = 0
_CACHE_STATS = {"hits": 0, "misses": 0, "memo_hits": 0}


def _device_bytes_estimate(cf: "CompiledFSM") -> int:
    """What a compiled graph holds on the device, roughly: both directions' arcs in two or three kernel forms (8 to 16 bytes per arc
    slot and form, padded) and per-state tables."""
    return int(96 * cf.fsm.nnz + 64 * cf.S1 + 4096)


def compiled_cache_stats(reset: bool = False) -> dict:
    """{"hits", "misses", "memo_hits", "entries"} of the compiled-graph cache behind the reference-shaped entries."""
    out = dict(_CACHE_STATS, entries=0 if _COMPILED_LRU is None else len(_COMPILED_LRU), bytes_estimate=_COMPILED_LRU_BYTES)
    if reset:
        for k in _CACHE_STATS:
            _CACHE_STATS[k] = 0
    return out


def compiled_cache_clear():
    global _COMPILED_LRU, _COMPILED_LRU_BYTES
    _COMPILED_LRU = None
    _COMPILED_LRU_BYTES = 0


def _content_key(part: FSM, c: StateMap) -> bytes:
    try:
        import xxhash

        h = xxhash.xxh3_128()
    except ImportError:  # pragma: no cover
        import hashlib

        h = hashlib.blake2b(digest_size=16)
    nz = np.ascontiguousarray(part.nzval)
    h.update(f"{part.semiring}|{part.S1}|{part.nnz}|{nz.dtype.str}|{c.numpdf}|".encode())
    for a in (part.colptr, part.rowval, nz, part.alpha_idx, part.alpha_val, c.state2pdf):
        a = np.ascontiguousarray(a)
        h.update(memoryview(a).cast("B"))
        h.update(b"|")
    return h.digest()


def _compiled_for(parts, Cs) -> List[CompiledFSM]:
    global _COMPILED_LRU, _COMPILED_LRU_BYTES
    from collections import OrderedDict

    if _COMPILED_LRU is None:
        _COMPILED_LRU = OrderedDict()
    lru = _COMPILED_LRU
    local, keys = {}, []
    for part, c in zip(parts, Cs):  # (the same objects repeated -- one denominator graph B times -- are hashed once)
        ik = (id(part), id(c))
        if ik not in local:
            local[ik] = _content_key(part, c)
        keys.append(local[ik])
    miss = {}
    for k, part, c in zip(keys, parts, Cs):
        if k in lru:
            lru.move_to_end(k)
        elif k not in miss:
            miss[k] = (part, c)
    _CACHE_STATS["hits"] += len(keys) - len(miss)
    _CACHE_STATS["misses"] += len(miss)
    if miss:
        # one call per (semiring, float type) group: compile_many's graphs share both
        groups = {}
        for k, (part, c) in miss.items():
            groups.setdefault((part.semiring, np.asarray(part.nzval).dtype == np.float64), []).append((k, part, c))
        for grp in groups.values():
            made = compile_many([g[1] for g in grp], [g[2] for g in grp]) if len(grp) > 1 else [CompiledFSM(grp[0][1], grp[0][2])]
            for (k, _, _), cf in zip(grp, made):
                lru[k] = cf
                _COMPILED_LRU_BYTES += _device_bytes_estimate(cf)
    out = [lru[k] for k in keys]  # (before anything is evicted: a batch larger than the bounds still gets its graphs)
    while len(lru) > 1 and (len(lru) > _COMPILED_LRU_MAX or _COMPILED_LRU_BYTES > _COMPILED_LRU_MAX_BYTES):
        _, old = lru.popitem(last=False)
        _COMPILED_LRU_BYTES -= _device_bytes_estimate(old)
    return out


def _as_batch(fsm, Chats) -> BatchedFSM:
    if isinstance(fsm, BatchedFSM):
        return fsm
    if isinstance(fsm, CompiledFSM):
        return BatchedFSM([fsm])
    if Chats is None:
        raise TypeError("pdfposteriors(fsm::FSM, V_hats, C_hats) needs the state maps")
    # the same FSM object with the same map objects as last time (a training loop's denominator): the batch as it was -- if the
    # object still holds what it held (a fingerprint of its arrays: their buffers, sizes and a strided sample of their values --
    # an FSM mutated in place between calls misses here and is found, or compiled, by its content below; the reference re-reads the
    # FSM on every call)
    memo = fsm.__dict__.get("_mm_batch_memo")
    if memo is not None and len(memo[0]) == len(Chats) and all(a is b for a, b in zip(memo[0], Chats)) and memo[2] == _fingerprint(fsm, Chats):
        _CACHE_STATS["memo_hits"] += 1
        return memo[1]
    # (a general sparse C_hat rides along as an argument of the generic entry; its FSM handle gets a placeholder map)
    Cs = [c if isinstance(c, StateMap) else
          (StateMap(np.zeros(c.shape[0] - 1, dtype=np.int64), c.numpdf) if isinstance(c, GeneralStateMap) else StateMap.from_matrix(c))
          for c in Chats]
    parts = split_blocks(fsm, [c.shape[0] for c in Cs])
    bf = BatchedFSM(_compiled_for(parts, Cs))
    fsm.__dict__["_mm_batch_memo"] = (list(Chats), bf, _fingerprint(fsm, Chats))
    return bf


def _fingerprint(fsm: FSM, Chats) -> tuple:
    """Cheap (O(1) in the size of the graph) and sensitive to what in-place edits do: for every array of the FSM and of the first and
    last state map its buffer address, size and 64 evenly spaced values."""
    def one(a):
        a = np.asarray(a)
        if a.size == 0:
            return (0, 0, b"")
        flat = a.reshape(-1)
        return (a.__array_interface__["data"][0], a.size, flat[:: max(1, a.size // 64)][:65].tobytes())

    arrs = [fsm.colptr, fsm.rowval, fsm.nzval, fsm.alpha_idx, fsm.alpha_val]
    for c in (Chats[0], Chats[-1]):
        s2p = getattr(c, "state2pdf", None)
        if s2p is not None:
            arrs.append(s2p)
    return tuple(one(a) for a in arrs)


def _device_vhats(Vhats):
    """The V_hats as ONE device tensor [B, P+1, N+1] if they are float32 tensors on the HIP device (a list of (P+1) x (N+1)
    matrices, or the stacked tensor itself), else None."""
    try:
        import torch
    except ImportError:  # pragma: no cover
        return None
    if isinstance(Vhats, torch.Tensor):
        return Vhats if (Vhats.is_cuda and Vhats.dim() == 3 and Vhats.dtype == torch.float32) else None
    Vh = list(Vhats)
    if not Vh or not all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 2 and v.dtype == torch.float32 for v in Vh):
        return None
    if any(v.shape != Vh[0].shape for v in Vh):
        raise _lib.DimensionMismatch(-2, "all V_hat must share one (P+1) x (N+1) shape")
    return torch.stack(Vh)


def _pdfposteriors_device(bf: BatchedFSM, Vd, seqlengths):
    """The reference call shape on device-resident V_hats, nothing crossing to the host unless asked to: the (P+1) x (N+1)
    matrices of expand() (src/inference.jl:54-60) become the engine's [B, N, P] log-likelihoods + lengths by one transposing
    copy; the lengths come from ``seqlengths`` (trusted, asynchronous) or -- one small reduction and a host read -- from the phony
    row, whose form is then checked like _unexpand checks it.  Returns device tensors (gamma[B, P, N] as a view, ttl[B])."""
    torch = _torch()
    B, P1, N1 = Vd.shape
    if B != bf.B:
        raise _lib.DimensionMismatch(-2, f"{B} matrices V_hat for a batch of {bf.B} FSMs")
    if seqlengths is None:
        zero, one = _SEM_ZERO[bf.semiring], _SEM_ONE[bf.semiring]
        ph = Vd[:, P1 - 1, :]
        lens = (ph == zero).sum(dim=1).to(torch.int32)
        step = torch.arange(N1, device=Vd.device)[None, :] < lens[:, None]
        ok = bool((torch.where(step, ph == zero, ph == one).all() & (lens <= N1 - 1).all()).item())
        if ok:  # real pdfs beyond the length are zero(K)
            ok = bool((Vd[:, : P1 - 1, :] == zero).masked_fill(step[:, None, :], True).all().item())
        if not ok:
            return None
    else:
        lens = torch.as_tensor(seqlengths, dtype=torch.int32, device=Vd.device)
    V = Vd[:, : P1 - 1, : N1 - 1].transpose(1, 2).contiguous()
    g, ttl = bf.pdfposteriors(V, lens)
    return g.transpose(1, 2), ttl


def pdfposteriors(fsm, Vhats, Chats=None, seqlengths=None):
    """pdfposteriors(fsm, V_hats, C_hats) (src/inference.jl:145-161) -- ``fsm`` the
    rawunion of the batch -- or pdfposteriors2(cfsm, V_hats) (:164-180) when
    given a BatchedFSM/CompiledFSM.  Returns (gamma[B, P, N] probabilities,
    ttl[B]): NumPy arrays for host inputs, like the reference returns fresh arrays; DEVICE tensors for float32 V_hats
    that live on the HIP device (a list of (P+1) x (N+1) tensors or one [B, P+1, N+1] tensor), with nothing but the
    compiled-graph cache between the call and the kernels (``seqlengths``: the lengths expand() was given, so that they
    need not be read back from the phony row)."""
    if not hasattr(Vhats, "dim"):  # (a generator is read once)
        Vhats = list(Vhats)
    Vd = _device_vhats(Vhats)
    if Chats is not None:  # general sparse maps that are one-hot after all take the fast kernels
        Chats = [(c.one_hot() or c) if isinstance(c, GeneralStateMap) else c for c in Chats]
    bf = _as_batch(fsm, Chats)
    general_c = Chats is not None and any(isinstance(c, GeneralStateMap) for c in Chats)
    # (ProbSemiring{Float32}: the fast entry too -- the library runs the log twins of the FSMs on log V_hat, mm_pdfposteriors_f32)
    fast = not (general_c or bf.dtype == np.float64) and (bf.semiring != "prob" or bf.has_fast_entry())
    if Vd is not None and fast:
        out = _pdfposteriors_device(bf, Vd, seqlengths)
        if out is not None:
            return out
    Vh = [np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in Vhats]
    # the precision follows the FSM's K like the reference (src/inference.jl:147 converts V_hat to K): a Float32 FSM computes
    # in float32 whatever the dtype of V_hat (NumPy's default float64 included), a Float64 FSM in float64
    un = _unexpand(Vh, bf.semiring) if fast else None
    if un is None:
        # a Float64 FSM, ProbSemiring, a general C_hat, or V_hat that expand() did not make: the generic entry
        return bf.pdfposteriors_generic(Vh, Chats if general_c else None)
    V, lens = un
    g, ttl = bf.pdfposteriors(V, lens)
    return np.ascontiguousarray(g.transpose(0, 2, 1)), ttl


def _expanded_inputs(fsm, Vhats, Chats, seqlengths):
    """``(bf, V, lens, on_device)`` for the entries in ``pdfposteriors``' call shape that take only what ``expand`` makes: float32
    V_hats on the HIP device given with their ``seqlengths`` stay there (one transposing copy to the engine's [B, N, P]), everything
    else goes through the host.  The caller transposes its [B, N, P] result back: a view on the device, a fresh array on the host."""
    if not hasattr(Vhats, "dim"):  # (a generator is read once)
        Vhats = list(Vhats)
    bf = _as_batch(fsm, Chats)
    Vd = _device_vhats(Vhats)
    if Vd is not None and seqlengths is not None:
        torch = _torch()
        B, P1, N1 = Vd.shape
        if B != bf.B:
            raise _lib.DimensionMismatch(-2, f"{B} matrices V_hat for a batch of {bf.B} FSMs")
        lens = torch.as_tensor(seqlengths, dtype=torch.int32, device=Vd.device)
        return bf, Vd[:, : P1 - 1, : N1 - 1].transpose(1, 2).contiguous(), lens, True
    # (device V_hats without their lengths: to the host, as pdfposteriors moves them, where the phony row gives the lengths)
    Vh = [np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in Vhats]
    return (bf, *_need_expanded(Vh, bf.semiring), False)


def leakyposteriors(fsm, Vhats, Chats=None, leak=1e-5, seqlengths=None):
    """Pdf posteriors of the leaky HMM -- see ``BatchedFSM.leakyposteriors`` -- in ``pdfposteriors``' call shape: ``fsm`` the
    rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring, Float32); V_hats what ``expand``
    makes.  Returns (gamma[B, P, N] probabilities, ttl[B]): NumPy arrays for host inputs, device tensors for float32 V_hats on
    the HIP device given with their ``seqlengths``."""
    bf, V, lens, on_device = _expanded_inputs(fsm, Vhats, Chats, seqlengths)
    g, ttl = bf.leakyposteriors(V, lens, leak=leak)
    return (g.transpose(1, 2) if on_device else np.ascontiguousarray(g.transpose(0, 2, 1))), ttl


def filterposteriors(fsm, Vhats, Chats=None, seqlengths=None):
    """Forward filtering posteriors -- see ``BatchedFSM.filterposteriors`` -- in ``pdfposteriors``' call shape, from the FSMs' own
    initial vectors: ``fsm`` the rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring,
    Float32); V_hats what ``expand`` makes.  Returns (filt[B, P, N] probabilities, incr[B, N], ttl[B]): NumPy arrays for host
    inputs, device tensors for float32 V_hats on the HIP device given with their ``seqlengths``."""
    bf, V, lens, on_device = _expanded_inputs(fsm, Vhats, Chats, seqlengths)
    f, incr, ttl = bf.filterposteriors(V, lens)
    return (f.transpose(1, 2) if on_device else np.ascontiguousarray(f.transpose(0, 2, 1))), incr, ttl


def windowposteriors(fsm, Vhats, Chats=None, seqlengths=None, closed=None):
    """Window posteriors -- see ``BatchedFSM.windowposteriors`` -- in ``pdfposteriors``' call shape, from the FSMs' own initial
    vectors: ``fsm`` the rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring, Float32);
    V_hats what ``expand`` makes; ``closed`` None: every window ends open.  Returns (gamma[B, P, N] probabilities, ttl[B]):
    NumPy arrays for host inputs, device tensors for float32 V_hats on the HIP device given with their ``seqlengths``."""
    bf, V, lens, on_device = _expanded_inputs(fsm, Vhats, Chats, seqlengths)
    g, ttl, _ = bf.windowposteriors(V, lens, closed=closed)
    return (g.transpose(1, 2) if on_device else np.ascontiguousarray(g.transpose(0, 2, 1))), ttl


def chunkedposteriors(fsm, Vhats, Chats=None, seqlengths=None, chunk=1024):
    """The exact smoothing posteriors in the workspace of one chunk -- see ``BatchedFSM.chunkedposteriors`` -- in ``pdfposteriors``'
    call shape: ``fsm`` the rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring, Float32);
    V_hats what ``expand`` makes.  Returns (gamma[B, P, N] probabilities, ttl[B]): NumPy arrays for host inputs, device tensors for
    float32 V_hats on the HIP device given with their ``seqlengths``."""
    bf, V, lens, on_device = _expanded_inputs(fsm, Vhats, Chats, seqlengths)
    g, ttl = bf.chunkedposteriors(V, lens, chunk=chunk)
    return (g.transpose(1, 2) if on_device else np.ascontiguousarray(g.transpose(0, 2, 1))), ttl


def arcposteriors(fsm, Vhats, Chats=None, want_init=False):
    """Expected arc counts of every utterance (Baum-Welch's xi summed over the frames): ``(counts[B, max nnz], ttl[B])``, plus
    ``init[B, max n_init]`` with ``want_init`` -- see ``BatchedFSM.arcposteriors``.  ``fsm`` and the arguments as for
    ``pdfposteriors``: the rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM; ``counts[b, k]`` belongs to
    the k-th stored ``T_hat`` entry of utterance b's own FSM.  V_hats must be what ``expand`` makes.  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    return bf.arcposteriors(V, lens, want_init=want_init)


def arcclassposteriors(fsm, Vhats, classes, Chats=None, C=None):
    """Per-frame arc-class posteriors (Baum-Welch's xi_n summed by class): ``(xi[B, C, N], ttl[B])`` -- see
    ``BatchedFSM.set_arc_classes`` / ``BatchedFSM.arcclassposteriors``.  ``fsm`` and the V_hats as for ``arcposteriors``;
    ``classes``: one id array for a batch that repeats one FSM, or a list with one per utterance.  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    bf.set_arc_classes(classes, C)
    return bf.arcclassposteriors(V, lens)


def scoredposteriors(fsm, Vhats, classes, U, Chats=None, C=None):
    """Posteriors with per-frame arc-class scores: ``(gamma[B, N, P], xi[B, C, N], ttl[B])`` -- see ``BatchedFSM.set_arc_classes`` /
    ``BatchedFSM.scoredposteriors``.  ``fsm``, the V_hats and ``classes`` as for ``arcclassposteriors``; ``U`` the scores
    ``[B, N, C]`` (None: none).  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    bf.set_arc_classes(classes, C)
    return bf.scoredposteriors(V, U, lens)


def classcost(fsm, Vhats, classes, A, Chats=None, C=None, D=None):
    """Expected arc-class cost of every utterance under its path posterior, and the gradient: ``(risk[B], grad[B, N, P], ttl[B])`` --
    see ``BatchedFSM.set_arc_classes`` / ``BatchedFSM.classcost``.  ``fsm``, the V_hats and ``classes`` as for
    ``arcclassposteriors``; ``A`` the class costs ``[B, N, C]``, ``D`` the pdf costs ``[B, N, P]`` (None: none).  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    bf.set_arc_classes(classes, C)
    return bf.classcost(V, A, lens, D=D)


def weightedposteriors(fsm, Vhats, W, Chats=None, W_init=None, seqlengths=None):
    """Posteriors with call-time arc weights -- see ``BatchedFSM.weightedposteriors`` -- in ``pdfposteriors``' call shape: ``fsm``
    the rawunion of the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring); V_hats what ``expand`` makes
    (``seqlengths`` None: the phony row gives the lengths); ``W`` one weight vector for the batch (1-D; the batch must repeat one
    FSM) or one per utterance ([B, max nnz]), ``W_init`` likewise or None.  Returns NumPy (gamma[B, P, N], counts[B, max nnz],
    ttl[B], init[B, max n_init])."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    if seqlengths is not None:
        lens = np.asarray(seqlengths, dtype=np.int32)
    g, c, ttl, init = bf.weightedposteriors(V, W, W_init, lens, want_init=True)
    return np.ascontiguousarray(g.transpose(0, 2, 1)), c, ttl, init


def expectedcost(fsm, Vhats, costs, Chats=None):
    """Expected path cost of every utterance under its path posterior, and the gradient: ``(risk[B], grad[B, P, N], ttl[B])`` --
    see ``BatchedFSM.expectedcost``.  ``fsm`` and the arguments as for ``pdfposteriors``: the rawunion of the batch with its state
    maps, or a BatchedFSM / CompiledFSM; V_hats must be what ``expand`` makes; ``costs[b]`` is a P x N_b matrix, N_b at least
    the utterance's length (the cost of pdf p at frame n, laid out like the real rows of a V_hat; columns beyond the length are
    ignored).  ``grad`` comes back in ``pdfposteriors``' layout.  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    B, N, P = V.shape
    cost = np.zeros((B, N, P), dtype=np.float32)
    costs = list(costs)
    if len(costs) != B:
        raise _lib.DimensionMismatch(-2, f"{len(costs)} cost matrices for a batch of {B} FSMs")
    for b, c in enumerate(costs):
        c = np.asarray(c.cpu() if hasattr(c, "cpu") else c, dtype=np.float32)
        if c.ndim != 2 or c.shape[0] != P or c.shape[1] < lens[b]:
            raise _lib.DimensionMismatch(-2, f"cost {b} must be P={P} x (at least {int(lens[b])} frames), got {c.shape}")
        cost[b, : lens[b]] = c[:, : lens[b]].T
    risk, grad, ttl = bf.expectedcost(V, cost, lens)
    return risk, np.ascontiguousarray(grad.transpose(0, 2, 1)), ttl


def pathentropy(fsm, Vhats, Chats=None):
    """Entropy of every utterance's posterior over complete paths, and its gradient in the emissions: ``(entropy[B],
    grad[B, P, N], ttl[B])`` -- see ``BatchedFSM.pathentropy``.  ``fsm`` and the arguments as for ``pdfposteriors``: the rawunion of
    the batch with its state maps, or a BatchedFSM / CompiledFSM (log semiring); V_hats must be what ``expand`` makes.  ``grad``
    comes back in ``pdfposteriors``' layout.  NumPy arrays out."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    ent, grad, ttl = bf.pathentropy(V, lens)
    return ent, np.ascontiguousarray(grad.transpose(0, 2, 1)), ttl


def samplepaths(fsm, Vhats, Chats=None, nsamples=1, seed=0):
    """State sequences drawn from the posterior over complete paths (forward filtering, backward sampling): per utterance a
    ``[K, len_b]`` int32 array of 0-based states (what ``bestpath`` returns for its one path) and the ``[K]`` natural-log posterior
    probabilities of the sampled sequences -- see ``BatchedFSM.samplepaths``.  ``fsm`` and the arguments as for ``bestpath``, on a
    log-semiring FSM; V_hats must be what ``expand`` makes.  The same ``seed`` gives the same samples."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats, bf.semiring)
    paths, _, lp = bf.samplepaths(V, lens, nsamples=nsamples, seed=seed, want_logprob=True)
    return [paths[b, :, : lens[b]].copy() for b in range(bf.B)], [lp[b].copy() for b in range(bf.B)]


def alpharecursion(fsm, Vhats, Chats=None):
    """alpha-recursion (src/inference.jl:62-74) on C_hat * V_hat as pdfposteriors calls
    it (:150-152): the (sum S1) x (N+1) matrix state_A."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats)
    return bf.alpharecursion(V, lens)


def betarecursion(fsm, Vhats, Chats=None):
    """beta-recursion (src/inference.jl:99-110): state_B."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats)
    return bf.betarecursion(V, lens)


def bestpath(fsm, Vhats, Chats=None):
    """bestpath (docs/src/inference.md:6; historical examples/demo.ipynb cell 23):
    per utterance the 0-based state sequence of the best path and its weight."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats)
    path, score = bf.viterbi(V, lens)
    return [path[b, : lens[b]].copy() for b in range(bf.B)], score


def classbestpath(fsm, Vhats, classes, U=None, Chats=None, C=None):
    """Best paths with the classes of their arcs -- see ``BatchedFSM.set_path_classes`` / ``BatchedFSM.classpath`` -- in
    ``bestpath``'s call shape: per utterance the 0-based state sequence of the best path and the class of the entry taken at every
    transition (the label sequence with its times: ``decode.events``), and the paths' weights.  ``classes``: one id array for a
    batch that repeats one FSM, or a list with one per utterance; ``U`` the scores ``[B, N, C]`` (None: none)."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats)
    bf.set_path_classes(classes, C)
    path, cls, score = bf.classpath(V, U, lens)
    return [path[b, : lens[b]].copy() for b in range(bf.B)], [cls[b, : lens[b]].copy() for b in range(bf.B)], score


def windowbestpath(fsm, Vhats, Chats=None, closed=None):
    """Windowed best paths -- see ``BatchedFSM.viterbiwindow`` -- in ``bestpath``'s call shape, from the FSMs' own initial vectors:
    per utterance the 0-based state sequence of the window's best path, its weight and its convergence point (the leading
    ``converged[b]`` states are final whatever audio follows).  ``closed`` None: every window ends open."""
    bf = _as_batch(fsm, Chats)
    V, lens = _need_expanded(Vhats)
    path, score, conv, _, _, _ = bf.viterbiwindow(V, lens, closed=closed)
    return [path[b, : lens[b]].copy() for b in range(bf.B)], score, conv


def maxstateposteriors(fsm, Vhats, Chats=None):
    """maxstateposteriors (docs/src/inference.md:5; absent from src/ at this commit, historical use
    test/test_algorithms.jl:280): the max-marginals of the tropical semiring, mu = alpha (*) beta (/) best --
    for every state and frame the weight of the best complete path through it, relative to the best path
    overall (0 on a best path, -inf where no complete path passes).  Tropical FSMs; returns the
    (sum S1) x (N+1) matrix in the layout of alpha-recursion / beta-recursion."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("maxstateposteriors needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.maxstateposteriors(V, lens)


def lattice(fsm, Vhats, beam, Chats=None):
    """Beam-pruned best-path lattices -- see ``BatchedFSM.lattice`` -- in ``maxstateposteriors``' call shape: the ``Lattice`` of the
    batch (NumPy members), every arc on a complete path within ``beam`` of the best one.  Tropical FSMs."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("lattice needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.lattice(V, beam, lens)


def latticeposteriors(fsm, lat, Vhats, Chats=None, extra=None):
    """Lattice posteriors -- see ``BatchedFSM.latticeposteriors`` -- in ``lattice``'s call shape: the ``LatticePosteriors`` (NumPy
    members) of the lattice ``lat`` of the batch under the expanded emissions ``Vhats``.  Tropical FSMs."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("latticeposteriors needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.latticeposteriors(lat, V, lens, extra)


def latticecost(fsm, lat, Vhats, cost, Chats=None, extra=None):
    """Lattice expected cost -- see ``BatchedFSM.latticecost`` -- in ``lattice``'s call shape: the ``LatticeCost`` (NumPy members, with
    ``grad``, without ``gamma``) of the lattice ``lat`` of the batch under the expanded emissions ``Vhats`` and the per-record costs
    ``cost``.  Tropical FSMs."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("latticecost needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.latticecost(lat, V, cost, lens, extra)


def latticebest(fsm, lat, Vhats, Chats=None, extra=None):
    """Lattice best paths -- see ``BatchedFSM.latticebest`` -- in ``lattice``'s call shape: the ``LatticeBest`` (NumPy members, with
    ``rec`` and ``path``) of the lattice ``lat`` of the batch under the expanded emissions ``Vhats``.  Tropical FSMs."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("latticebest needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.latticebest(lat, V, lens, extra)


def latticesample(fsm, lat, Vhats, nsamples, seed=0, Chats=None, extra=None):
    """Lattice path sampling -- see ``BatchedFSM.latticesample`` -- in ``lattice``'s call shape: the ``LatticeSamples`` (NumPy members,
    with ``path`` and ``logprob``) of ``nsamples`` draws per utterance from the posterior of the lattice ``lat`` of the batch under the
    expanded emissions ``Vhats``.  Tropical FSMs."""
    bf = _as_batch(fsm, Chats)
    if bf.semiring != "tropical":
        raise TypeError("latticesample needs TropicalSemiring FSMs")
    V, lens = _need_expanded(Vhats)
    return bf.latticesample(lat, V, nsamples, seed, lens, extra)


def _total(fsm, n, cumulative):
    if isinstance(fsm, (BatchedFSM, CompiledFSM)):
        bf = _as_batch(fsm, None)
    else:  # no emissions are involved: any state map will do
        bf = BatchedFSM([CompiledFSM(fsm, StateMap(np.zeros(fsm.S1 - 1, dtype=np.int64), 1))])
    out = bf.totalsum(n, cumulative).cpu().numpy()
    return out if isinstance(fsm, BatchedFSM) else float(out[0])


def totalsum(fsm, n: int):
    """totalsum(alpha, T, omega, n) (src/algorithms.jl:23-29) of an FSM: the weight of all paths of exactly n
    states, in the FSM's semiring, as a natural-log float (an array for a BatchedFSM)."""
    return _total(fsm, n, False)


def totalcumsum(fsm, n: int):
    """totalcumsum(alpha, T, omega, n) (src/algorithms.jl:8-16): paths of up to n states."""
    return _total(fsm, n, True)


def totalweightsum(fsm, n: Optional[int] = None):
    """totalweightsum(fsm, n = nstates(fsm)) (src/algorithms.jl:36)."""
    if n is None:
        if isinstance(fsm, BatchedFSM):
            raise TypeError("totalweightsum of a batch needs n")
        n = fsm.S1 - 1
    return _total(fsm, n, True)


# the reference's own (unicode) export names, src/MarkovModels.jl:40-45
αrecursion = alpharecursion
βrecursion = betarecursion
