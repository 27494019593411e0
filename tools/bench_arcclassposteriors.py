#!/usr/bin/env python3
"""Per-frame arc-class posteriors (mm_arcclassposteriors_f32) next to arcposteriors and the item kernel's pdfposteriors of the
same batch (MM_KERNEL=item), timed in the same run: ms per call for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128,
T = 700) and the WSJ numerator x 128 (T = 700).  Three class layouts: boundary marks on ~3 % of the arcs (the arcs that enter
another pdf's states, thinned to 3 %, one class per pdf entered), the destination's pdf (every arc, C = P + 1), and one class
per arc (the numerator graph only: C = nnz rows per frame).  Prints one JSON line.
    python tools/bench_arcclassposteriors.py [out.json]      (GPU box)"""
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


def layouts(g, f, per_arc):
    s2p = np.concatenate([np.asarray(g.state2pdf), [g.P]])
    dst = mm.arc_classes_by_destination(f, s2p)
    marks = mm.boundary_classes(f, s2p[:-1])  # an arc that enters a state of another pdf
    on = np.flatnonzero(marks >= 0)
    keep = on[:: max(1, int(round(on.size / (0.03 * f.nnz))))]  # thinned to ~3 % of the entries
    sparse = np.full(f.nnz, -1, dtype=np.int32)
    sparse[keep] = marks[keep]
    out = [("boundary marks", sparse, g.P), ("destination pdf", dst, g.P + 1)]
    if per_arc:
        out.append(("one class per arc", np.arange(f.nnz, dtype=np.int32), f.nnz))
    return out


golden = os.path.join(ROOT, "tests", "golden")
rows = []
for name, g, B, N, per_arc in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500, False),
                               ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700, False),
                               ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700, True)):
    f = wl.to_fsm(mm, g)
    cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    bf = mm.batch(*([cf] * B))
    bi = item_batch(cf, B)
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    gam = torch.empty(B, N, g.P, device="cuda")
    t_arcs = timed(lambda: bf.arcposteriors(V, lens, want_init=True))
    t_item = timed(lambda: bi.pdfposteriors(V, lens, out=gam))
    for lname, cls, C in layouts(g, f, per_arc):
        bf.set_arc_classes(cls, C)
        t = timed(lambda: bf.arcclassposteriors(V, lens))
        rows.append(dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, layout=lname, C=int(C), classified=int((cls >= 0).sum()),
                         arcclassposteriors_ms=round(t, 3), arcposteriors_ms=round(t_arcs, 3), pdfposteriors_item_ms=round(t_item, 3),
                         ratio_to_arcposteriors=round(t / t_arcs, 3), ratio_to_pdfposteriors_item=round(t / t_item, 3),
                         cap=bf.info()["arcclass_cap"], kernels=bf.kernels("arcclass")))
        print(rows[-1], flush=True)
    del bf, bi, V, gam
line = json.dumps(dict(source_hash=source_hash(), rows=rows))
print(line, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(line + "\n")
