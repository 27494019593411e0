"""GPU tests of the arc window of the pair kernels (mm_kernel_pairs.hip: pair_two / MM_PAIR_TWO): one chain of four packed FMAs
per quad of arcs that runs on through the quad's second pair, and a rare path for the quads in which a segment ends -- after the
first pair (finish from the sums as they stood there, second pair again from zero), after the second, after both, in consecutive
quads, right before the window's early exits, in its last quad.  tests/test_pair_window_cases.py proves on the host that the
graphs below take every one of these paths, forward and backward (both phases of a direction run one form).  Here: the float32
kernels alone against the float64 oracle with the accuracy bar of test_gpu_parity.py, no utterance marked for the exact
kernels, and the same bits from two calls.  Small batches: three utterances of unequal lengths (the odd one is a pair with itself:
the copy path), one of a single frame."""
import numpy as np
import pytest

import graphs
from test_gpu_parity import _with_env, check_gamma
from test_pair_window_cases import GRAPHS

pytestmark = pytest.mark.gpu
FORCE = {"pair": {"MM_DEBUG": "1", "MM_KERNEL": "pair"}, "team": {"MM_DEBUG": "1", "MM_KERNEL": "split"}}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# (lengths at which the float32 kernels mark no utterance of any of the graphs for the exact kernels, so that every value checked
# below is theirs; at some others -- (8, 5, 8), (6, 3, 6), (10, 10, 3) -- they mark a short utterance of the 2000-state graphs)
@pytest.mark.parametrize("N,lens", [(12, (12, 7, 1)), (9, (9, 6, 2))])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_window_paths_against_the_oracle(mm, wl, oracle, torch, name, N, lens):
    make, form, kernels = GRAPHS[name]
    if name == "small":
        kernels += " (forward and backward agents in one grid, the instances for graphs of up to 127 states)"
    g = make(wl)
    o, oc = oracle
    B = len(lens)
    rng = np.random.default_rng(1000 * N + len(name))
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.asarray(lens, dtype=np.int32)
    g_ref, t_ref = oc.batch_shared(graphs.to_oracle(o, g), g.state2pdf, g.P, V, lens, dtype=np.float64, nthreads=4)
    cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    bf = _with_env(FORCE[form], lambda: mm.batch(*([cf] * B)))
    assert kernels in bf.kernels(), bf.kernels()
    Vd, ld = torch.from_numpy(V).cuda(), torch.from_numpy(lens).cuda()
    gam, ttl = bf.pdfposteriors(Vd, ld)
    torch.cuda.synchronize()
    assert bf.last_redo_count() == 0
    gam, ttl = gam.cpu().numpy(), ttl.cpu().numpy()
    # Which utterances have a path at all (else Z = 0, gamma = 0 and ttl = zero(K)): every one, but for the single frame in the
    # denominator graphs, whose units take two frames from an initial to a final state.  So the single frame is checked in numbers on
    # the small and the wide-row graph, the two-frame utterance and the batch's odd one everywhere.
    ok = np.isfinite(t_ref)
    assert ok.tolist() == [not (name.startswith("den") and L < 2) for L in lens], (name, t_ref)
    worst = check_gamma(gam[ok], g_ref[ok], lens[ok])
    print(name, form, N, "worst log-posterior error / bar:", worst, "ttl error:", np.abs(ttl[ok] - t_ref[ok]).max())
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=1e-4)
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()
    gam2, ttl2 = bf.pdfposteriors(Vd, ld)
    torch.cuda.synchronize()
    assert np.array_equal(gam2.cpu().numpy(), gam) and np.array_equal(ttl2.cpu().numpy(), ttl, equal_nan=True)
