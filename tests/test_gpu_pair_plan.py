"""GPU tests of the pair and team kernels on forms whose rows of 33 .. 44 arcs stay on one lane (the packer tries every even
cap up to the register window, tests/test_pair_plan.py): the float32 kernels alone against the float64 oracle, with the
accuracy bar of test_gpu_parity.py.  Small shapes: an odd batch (the last pair runs one utterance twice), an odd number of
frames (the agents' cut is not the middle), lengths down to one frame."""
import os

import numpy as np
import pytest

import graphs
from test_gpu_parity import _with_env, check_gamma

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def run_and_check(mm, wl, oracle, g, B, N, lens, kernel, env=None):
    o, oc = oracle
    rng = np.random.default_rng(B * 100 + N)
    V = rng.standard_normal((B, N, g.P)).astype(np.float32)
    lens = np.asarray(lens, dtype=np.int32)
    g_ref, t_ref = oc.batch_shared(graphs.to_oracle(o, g), g.state2pdf, g.P, V, lens, dtype=np.float64, nthreads=4)
    cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    bf = _with_env(env, lambda: mm.batch(*([cf] * B))) if env else mm.batch(*([cf] * B))
    assert kernel in bf.kernels(), bf.kernels()
    gam, ttl = bf.pdfposteriors(V, lens)
    gam, ttl = np.asarray(gam.cpu() if hasattr(gam, "cpu") else gam), np.asarray(ttl.cpu() if hasattr(ttl, "cpu") else ttl)
    assert bf.last_redo_count() == 0
    ok = np.isfinite(t_ref)  # (a length no path through the graph has: Z = 0, gamma = 0 and ttl = zero(K))
    assert ok[0]
    print(g.name, B, N, "worst log-posterior error / bar:", check_gamma(gam[ok], g_ref[ok], lens[ok]),
          "ttl error:", np.abs(ttl[ok] - t_ref[ok]).max())
    assert np.allclose(ttl[ok], t_ref[ok], rtol=1e-5, atol=1e-4)
    assert (gam[~ok] == 0).all() and np.isneginf(ttl[~ok]).all()


@pytest.mark.parametrize("B,N,lens", [(3, 41, (41, 17, 1)), (2, 8, (8, 5))])
def test_pair_kernels_on_long_single_lane_rows(mm, wl, oracle, torch, B, N, lens):
    """lfmmi_denominator(600, 40, seed=5): backward rows of 33 .. 41 arcs (+ the self loop), the rows whose lanes changed."""
    run_and_check(mm, wl, oracle, wl.lfmmi_denominator(600, 40, seed=5), B, N, lens, "mm_fbp_kernel")


@pytest.mark.parametrize("which", ["wsj_den", "wide"])
def test_team_kernels_on_the_new_plans(mm, wl, oracle, torch, which):
    """Teams of 2 (their forms keep the old cap list, RowPackOpts::every_cap = false, through the restructured plan search): the
    reference's WSJ denominator, which runs on them by itself, and the wide-row graph forced onto them."""
    if which == "wsj_den":
        g, N, lens, env = wl.load_npz_graph(os.path.join(HERE, "golden", "den_fsm_wsj.npz")), 12, (12, 7), None
    else:
        g, N, lens, env = wl.wide_row_fsm(), 10, (10, 6), {"MM_DEBUG": "1", "MM_KERNEL": "split"}
    run_and_check(mm, wl, oracle, g, 2, N, lens, "mm_fbs_kernel", env)
