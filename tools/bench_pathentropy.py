#!/usr/bin/env python3
"""Posterior path entropy (mm_pathentropy_f32), the full call and the value-only call, next to the two calls of the same batch
nearest to it -- the item kernel's pdfposteriors (MM_KERNEL=item) and expectedcost --: ms per call, device events after warm-up,
one process, the calls alternating, for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ
numerator x 128 (T = 700).  Prints one JSON line.
    python tools/bench_pathentropy.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


# (the two helpers of tools/bench_expectedcost.py, restated: that tool runs its benchmark when it is imported)
def timed_alternating(fns, K=8, W=2):
    """mean and spread (min, max) in ms of each call of `fns`, the calls taking turns: round r runs every call once"""
    for _ in range(W):
        for fn in fns.values():
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)] for k in fns}
    torch.cuda.synchronize()
    for r in range(K):
        for k, fn in fns.items():
            a, b = ev[k][r]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = {k: [a.elapsed_time(b) for a, b in ev[k]] for k in fns}
    return {k: (float(np.mean(v)), float(np.min(v)), float(np.max(v))) for k, v in t.items()}


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


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    rows = []
    for name, g, B, N in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
                          ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                          ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
        cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        bi = item_batch(cf, B)
        V = torch.randn(B, N, g.P, device="cuda")
        cost = torch.zeros(B, N, g.P, device="cuda")
        cost.scatter_(2, torch.randint(0, g.P, (B, N, 1), device="cuda"), -1.0)
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        gam = torch.empty(B, N, g.P, device="cuda")
        fns = {"pathentropy_ms": lambda: bf.pathentropy(V, lens),
               "pathentropy_value_only_ms": lambda: bf.pathentropy(V, lens, want_grad=False),
               "pdfposteriors_item_ms": lambda: bi.pdfposteriors(V, lens, out=gam),
               "expectedcost_ms": lambda: bf.expectedcost(V, cost, lens)}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, **{k: round(v[0], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
        row["over_pdfposteriors_item"] = round(t["pathentropy_ms"][0] / t["pdfposteriors_item_ms"][0], 3)
        row["over_expectedcost"] = round(t["pathentropy_ms"][0] / t["expectedcost_ms"][0], 3)
        row["value_only_over_full"] = round(t["pathentropy_value_only_ms"][0] / t["pathentropy_ms"][0], 3)
        row["kernels"] = bf.kernels("entropy")
        rows.append(row)
        del bf, bi, V, cost, gam
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
