"""The argument checks the BatchedFSM entries share (markovmodels.jl_amd/inference.py: _out_buffer, _state_vector, _want_vector,
_per_utt, _results, _ptr), called directly on CPU tensors with the CPU standing in for V's device: the bad and good inputs of
tests/test_gpu_binding_arguments.py, the same exception classes and messages, no GPU."""
from importlib import import_module

import numpy as np
import pytest
import torch

B, N, P, T = 2, 4, 3, 10
CPU = torch.device("cpu")
META = torch.device("meta")  # a device that is not V's


@pytest.fixture(scope="module")
def inf(mm):
    return import_module(mm.__name__ + ".inference")


def _raises(mm, exc, text, fn, *args):
    with pytest.raises(exc) as e:
        fn(*args)
    assert type(e.value) is exc and text in str(e.value), (type(e.value), str(e.value))
    if exc is mm.DimensionMismatch:
        assert e.value.code == -2


def test_out_buffer(mm, inf):
    fresh = inf._out_buffer(None, (B, N, P), CPU)
    assert fresh.shape == (B, N, P) and fresh.dtype == torch.float32 and fresh.device == CPU and fresh.is_contiguous()
    good = torch.zeros((B, N + 3, 2 * P))[:, :N, ::2]  # a view with strides of its own
    assert inf._out_buffer(good, (B, N, P), CPU) is good
    for bad in (torch.zeros((B, N, P), dtype=torch.float64), torch.zeros((B, N, P), device=META), np.zeros((B, N, P), dtype=np.float32)):
        _raises(mm, TypeError, "out must be a float32 tensor on V's device", inf._out_buffer, bad, (B, N, P), CPU)
    for shape in ((B, N, P + 1), (B, N + 1, P), (B * N, P)):
        _raises(mm, mm.DimensionMismatch, f"out must be [B={B}, N={N}, P={P}], got {shape}", inf._out_buffer, torch.zeros(shape), (B, N, P), CPU)
    # the kind is looked at before the shape
    _raises(mm, TypeError, "out must be a float32 tensor", inf._out_buffer, torch.zeros((B * N, P), dtype=torch.float64), (B, N, P), CPU)


def _bad_vectors(good):
    return [(good.double(), TypeError, " must be a float32 tensor on V's device"),
            (good.to(META), TypeError, " must be a float32 tensor on V's device"),
            (torch.zeros(T + 1), None, f" must be a contiguous [{T}] vector, got {(T + 1,)}"),
            (good[None], None, f" must be a contiguous [{T}] vector, got {(1, T)}"),
            (torch.zeros(2 * T)[::2], None, f" must be a contiguous [{T}] vector, got {(T,)}")]


@pytest.mark.parametrize("name", ["state", "end"])
def test_state_vector(mm, inf, name):
    good = torch.arange(T, dtype=torch.float32)
    assert inf._state_vector(None, name, T, CPU) is None
    assert inf._state_vector(good, name, T, CPU) is good
    for bad, exc, text in _bad_vectors(good):
        _raises(mm, exc or mm.DimensionMismatch, name + text, inf._state_vector, bad, name, T, CPU)
    # what is not a tensor comes through NumPy as float32: float64 arrays, lists
    for x in (good.numpy().astype(np.float64), good.tolist()):
        got = inf._state_vector(x, name, T, CPU)
        assert got.dtype == torch.float32 and got.device == CPU and torch.equal(got, good)
    _raises(mm, mm.DimensionMismatch, f"{name} must be a contiguous [{T}] vector, got {(B, T // B)}", inf._state_vector,
            np.zeros((B, T // B)), name, T, CPU)


@pytest.mark.parametrize("name", ["the state buffer", "the end buffer"])
def test_want_vector(mm, inf, name):
    assert inf._want_vector(False, name, T, CPU) is None and inf._want_vector(None, name, T, CPU) is None
    made = inf._want_vector(True, name, T, CPU)
    assert made.shape == (T,) and made.dtype == torch.float32 and made.device == CPU
    good = torch.zeros(T)
    assert inf._want_vector(good, name, T, CPU) is good
    for bad, exc, text in _bad_vectors(good):
        _raises(mm, exc or mm.DimensionMismatch, name + text, inf._want_vector, bad, name, T, CPU)
    # only a tensor is a buffer: a NumPy array is asked whether it is true, which NumPy refuses
    with pytest.raises(ValueError, match="truth value"):
        inf._want_vector(np.zeros(T, dtype=np.float32), name, T, CPU)


@pytest.mark.parametrize("name", ["closed", "commit", "end_mode"])
def test_per_utt(mm, inf, name):
    assert inf._per_utt(None, name, B, CPU) is None
    want = torch.tensor([2, 1], dtype=torch.int32)
    for x in ([2, 1], np.array([2, 1], dtype=np.int64), torch.tensor([2, 1], dtype=torch.int64), torch.tensor([2, 9, 1], dtype=torch.int32)[::2]):
        got = inf._per_utt(x, name, B, CPU)
        assert got.dtype == torch.int32 and got.device == CPU and got.is_contiguous() and torch.equal(got, want)
    _raises(mm, mm.DimensionMismatch, f"{name} must be a [{B}] vector, got {(B + 1,)}", inf._per_utt, [2, 1, 0], name, B, CPU)
    _raises(mm, mm.DimensionMismatch, f"{name} must be a [{B}] vector, got {(B, 1)}", inf._per_utt, want[:, None], name, B, CPU)


def test_results_and_ptr(inf):
    a, b = torch.arange(3, dtype=torch.float32), torch.arange(4, dtype=torch.int32)
    res = (a, None, b)
    assert inf._results(res, False) is res
    out = inf._results(res, True)
    assert isinstance(out, tuple) and len(out) == 3 and out[1] is None
    assert isinstance(out[0], np.ndarray) and np.array_equal(out[0], a.numpy()) and out[2].dtype == np.int32
    assert inf._ptr(None) is None and inf._ptr(a) == a.data_ptr()
