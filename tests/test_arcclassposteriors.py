"""Per-frame arc-class posteriors without a GPU: the float64 reference helper against path enumeration, the identities the
definition implies, the two host helpers that make class arrays, and the bindings of the new entry."""
import os
import re

import numpy as np
import pytest

import arc_reference as ar
import arcclass_reference as acr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(wl, which):
    return wl.l2r_hmm(3) if which == "l2r3" else wl.random_fsm(4, 3, mean_deg=2.0, seed=9)


def _layouts(g, f):
    """(name, cls, C): one class per entry, the source state's pdf, the destination's pdf, a sparse layout with an empty class."""
    i, j, _ = ar.fsm_entries(f)
    s2p = ar._s2p_full(g)
    sparse = np.full(f.nnz, -1)
    sparse[::2] = 0
    sparse[1::4] = 2
    return [("entry", np.arange(f.nnz), f.nnz), ("src", s2p[i], g.P + 1), ("dst", s2p[j], g.P + 1), ("sparse", sparse, 3)]


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
@pytest.mark.parametrize("L", [4, 2, 0])
def test_reference_against_path_enumeration(mm, wl, oracle, which, L):
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N = 4
    V = np.random.default_rng(10 + L).standard_normal((N, g.P))
    for name, cls, C in _layouts(g, f):
        xi, z, exact = acr.reference(o, oc, g, f, cls, C, V, L, N)
        xe, ze = acr.enumerate_paths(g, f, cls, C, V, L, N)
        if L == 0 or (which == "l2r3" and L < 3):  # no frame, or fewer frames than the chain has states: no accepting path
            assert np.isneginf(z) and np.isneginf(ze) and (xi == 0).all() and (xe == 0).all() and exact.all()
            continue
        assert np.isfinite(z) and np.isclose(z, ze, rtol=1e-10, atol=1e-10), name
        assert np.allclose(xi, xe, rtol=1e-9, atol=1e-12), name
        assert (xi[exact] == xe[exact]).all() or np.allclose(xi[exact], xe[exact], atol=1e-15)
        assert acr.check(xi, z, xe, ze, exact) <= 1e-3  # (the bar's own plumbing on a perfect answer)


@pytest.mark.parametrize("which", ["l2r3", "rand4"])
def test_identities(mm, wl, oracle, which):
    """Sum over the classes = 1 in every frame, sum over the frames = the arc counts by class, source-pdf classes = gamma,
    destination-pdf classes = gamma one frame on; float64 at 1e-10."""
    o, oc = oracle
    g = _tiny(wl, which)
    f = wl.to_fsm(mm, g, dtype=np.float64)
    N, P = 7, g.P
    V = np.random.default_rng(3).standard_normal((N, P))
    for L in (7, 5, 3):
        c_ref, _, z = ar.reference(o, oc, g, f, V, L, N)
        assert np.isfinite(z)
        for name, cls, C in _layouts(g, f):
            xi, z2, exact, gamma = acr.reference(o, oc, g, f, cls, C, V, L, N, want_gamma=True)
            assert z2 == z
            if name != "sparse":
                assert np.allclose(xi.sum(axis=0), 1.0, atol=1e-10), (name, L)
            by_class = np.zeros(C)
            np.add.at(by_class, cls[cls >= 0], c_ref[cls >= 0])
            assert np.allclose(xi.sum(axis=1), by_class, atol=1e-10), (name, L)
            if name == "src":
                assert np.allclose(xi[:, :L], gamma[:, :L], atol=1e-10)
                assert (xi[:P, L:] == 0).all() and (xi[P, L:] == 1).all()
            if name == "dst":
                assert np.allclose(xi[:, : L - 1], gamma[:, 1:L], atol=1e-10)
                assert np.allclose(xi[P, L - 1], 1.0, atol=1e-10) and np.allclose(xi[:P, L - 1], 0.0, atol=1e-12)  # the final arcs
                assert (xi[P, L:] == 1).all()
            if name == "sparse":
                assert exact[1].all() and (xi[1] == 0).all()  # the empty class


def _two_group_fsm(mm):
    """Five states: 0, 1, 2 in group 0 and 3, 4 in group 1; 2 -> 3 and 4 -> 0 cross; 1 and 4 are final."""
    arcs = [((0, 0), -0.5), ((0, 1), -1.0), ((1, 2), -0.3), ((2, 2), -0.7), ((2, 3), -0.9), ((3, 4), -0.2), ((4, 4), -1.1), ((4, 0), -1.3),
            ((1, 0), -2.0)]
    return mm.FSM([(0, 0.0), (3, -1.0)], arcs, [(1, -0.4), (4, -0.6)], list("abcde"))


def test_boundary_classes_on_a_hand_made_graph(mm):
    f = _two_group_fsm(mm)
    i, j, _ = ar.fsm_entries(f)
    group = np.array([0, 0, 0, 1, 1])
    b = mm.boundary_classes(f, group)
    assert b.dtype == np.int32 and b.shape == (f.nnz,)
    want = {(2, 3): 1, (4, 0): 0}
    for k in range(f.nnz):
        assert b[k] == want.get((int(i[k]), int(j[k])), -1), (int(i[k]), int(j[k]), b[k])
    assert (b[j == 5] == -1).all() and (b >= 0).sum() == 2  # the phony column and self-loop are no boundaries
    assert (mm.boundary_classes(f, np.concatenate([group, [7]])) == b).all()  # a group for the phony state changes nothing
    d = mm.arc_classes_by_destination(f, group)
    assert (d[j < 5] == group[j[j < 5]]).all() and (d[j == 5] == -1).all()
    d1 = mm.arc_classes_by_destination(f, np.concatenate([group, [2]]))
    assert (d1[j == 5] == 2).all() and (d1[j < 5] == d[j < 5]).all()
    with pytest.raises(ValueError):
        mm.boundary_classes(f, group[:3])


def test_helpers_follow_a_scrambled_entry_order(mm):
    """The entries of every column of T_hat in a scrambled order (FSM.from_fields takes them as they come): the class of an
    entry stays with the entry."""
    f = _two_group_fsm(mm)
    i, j, w = ar.fsm_entries(f)
    order = np.lexsort((np.random.default_rng(1).random(i.size), j))  # by column, scrambled inside a column
    assert (order != np.arange(i.size)).any()
    f2 = mm.FSM.from_fields(f.alpha_idx, f.alpha_val, f.colptr, f.rowval[order], f.nzval[order], f.labels)
    group = np.array([0, 0, 0, 1, 1])
    assert (mm.boundary_classes(f2, group) == mm.boundary_classes(f, group)[order]).all()
    assert (mm.arc_classes_by_destination(f2, group) == mm.arc_classes_by_destination(f, group)[order]).all()
    s = np.array([4, 3, 2, 1, 0, 5])
    assert (mm.arc_classes_by_destination(f2, s) == s[j[order]]).all()


def test_entry_is_bound(mm):
    assert callable(mm.arcclassposteriors) and hasattr(mm.BatchedFSM, "arcclassposteriors") and hasattr(mm.BatchedFSM, "set_arc_classes")
    for s in ("mm_arcclassposteriors_f32", "mm_batch_set_arc_classes", "mm_batch_arc_class_info"):
        assert s in mm.SYMBOLS
    from importlib import import_module

    lib = import_module(mm.__name__ + "._lib").lib
    assert len(lib.mm_arcclassposteriors_f32.argtypes) == 12 and len(lib.mm_batch_set_arc_classes.argtypes) == 4
    hdr = open(os.path.join(ROOT, "include", "markovmodels_amd.h")).read()
    assert "int mm_arcclassposteriors_f32(" in hdr and "int mm_batch_set_arc_classes(" in hdr and "#define MM_ABI_VERSION 4 " in hdr


def test_julia_shim_has_the_literal_ccalls():
    src = open(os.path.join(ROOT, "julia", "MarkovModelsAMD.jl")).read()
    assert re.search(r"ccall\(\(:mm_arcclassposteriors_f32, LIB\)", src)
    assert re.search(r"ccall\(\(:mm_batch_set_arc_classes, LIB\)", src)
    assert re.search(r"function arcclassposteriors\(", src) and re.search(r"function set_arc_classes!\(", src)
