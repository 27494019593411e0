#!/usr/bin/env python3
"""Posteriors with per-frame arc-class scores (mm_scoredposteriors_f32) next to the two entries a call without scores replaces --
arcclassposteriors followed by the item kernel's pdfposteriors of the same batch (MM_KERNEL=item) --, timed in the same run: ms
per call for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).  Two
class layouts: loop_exit_classes (every arc, C = 2 P) and boundary marks on ~3 % of the arcs (the arcs that enter another pdf's
states, thinned to 3 %, one class per pdf entered).  Per combination: the call with U = N(0, 1), the call with U NULL, the pair,
and the ratio of the U NULL call to the pair.  Prints one JSON line.
    python tools/bench_scoredposteriors.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def timed(fn, K=10, W=3):
    for _ in range(W):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in ev]))


def item_batch(cf, B):
    """the same batch with pdfposteriors forced onto the item kernel (the switches are read when a batch is made)"""
    old = {k: os.environ.get(k) for k in ("MM_DEBUG", "MM_KERNEL")}
    os.environ.update(MM_DEBUG="1", MM_KERNEL="item")
    try:
        return mm.batch(*([cf] * B))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def layouts(g, f):
    s2p = np.concatenate([np.asarray(g.state2pdf), [g.P]])
    marks = mm.boundary_classes(f, s2p[:-1])  # an arc that enters a state of another pdf
    on = np.flatnonzero(marks >= 0)
    keep = on[:: max(1, int(round(on.size / (0.03 * f.nnz))))]  # thinned to ~3 % of the entries
    sparse = np.full(f.nnz, -1, dtype=np.int32)
    sparse[keep] = marks[keep]
    le, C = mm.loop_exit_classes(f, g.state2pdf, g.P)
    return [("loop / exit per pdf", le, C), ("boundary marks", sparse, g.P)]


golden = os.path.join(ROOT, "tests", "golden")
rows = []
for name, g, B, N in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
                      ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                      ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
    f = wl.to_fsm(mm, g)
    cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    bf = mm.batch(*([cf] * B))
    bi = item_batch(cf, B)
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    gam = torch.empty(B, N, g.P, device="cuda")
    t_item = timed(lambda: bi.pdfposteriors(V, lens, out=gam))
    for lname, cls, C in layouts(g, f):
        bf.set_arc_classes(cls, C)
        U = torch.randn(B, N, C, device="cuda")
        t_cls = timed(lambda: bf.arcclassposteriors(V, lens))
        t_u = timed(lambda: bf.scoredposteriors(V, U, lens, out=gam))
        t_0 = timed(lambda: bf.scoredposteriors(V, None, lens, out=gam))
        t_x = timed(lambda: bf.scoredposteriors(V, U, lens, want_gamma=False))
        rows.append(dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, layout=lname, C=int(C), classified=int((cls >= 0).sum()),
                         scoredposteriors_ms=round(t_u, 3), scoredposteriors_no_scores_ms=round(t_0, 3), scoredposteriors_xi_only_ms=round(t_x, 3),
                         arcclassposteriors_ms=round(t_cls, 3), pdfposteriors_item_ms=round(t_item, 3), pair_ms=round(t_cls + t_item, 3),
                         ratio_no_scores_to_pair=round(t_0 / (t_cls + t_item), 3), ratio_scores_to_no_scores=round(t_u / t_0, 3),
                         class_cap=bf.info(scored=True)["score_class_cap"], kernels=bf.kernels("scored")))
        print(rows[-1], flush=True)
        del U
    del bf, bi, V, gam
line = json.dumps(dict(source_hash=source_hash(), rows=rows))
print(line, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(line + "\n")
