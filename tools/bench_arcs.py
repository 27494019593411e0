#!/usr/bin/env python3
"""Arc posteriors (mm_arcposteriors_f32) next to the item kernel's pdfposteriors of the same batch (MM_KERNEL=item): ms per call
for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).  Prints one JSON
line.
    python tools/bench_arcs.py [out.json]      (GPU box)"""
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


golden = os.path.join(ROOT, "tests", "golden")
rows = []
for name, g, B, N in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
                      ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                      ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
    cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    bf = mm.batch(*([cf] * B))
    bi = item_batch(cf, B)
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    gam = torch.empty(B, N, g.P, device="cuda")
    t_arcs = timed(lambda: bf.arcposteriors(V, lens, want_init=True))
    t_item = timed(lambda: bi.pdfposteriors(V, lens, out=gam))
    rows.append(dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, arcposteriors_ms=round(t_arcs, 3),
                     pdfposteriors_item_ms=round(t_item, 3), ratio=round(t_arcs / t_item, 3), kernels=bf.kernels("arcs")))
    del bf, bi, V, gam
line = json.dumps(dict(source_hash=source_hash(), rows=rows))
print(line, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(line + "\n")
