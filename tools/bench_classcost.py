#!/usr/bin/env python3
"""Expected arc-class cost (mm_classcost_f32) next to the two calls of the same batch it is made of -- expectedcost (the same
recursion without the class term) and arcclassposteriors (the same class plan) --: ms per call, device events, 10 timed calls after
warm-up, the calls alternating, for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128
(T = 700); each with boundary marks on ~3 % of the arcs (one class, the other arcs unclassified) and with loop / exit classes on
every arc (fsm.loop_exit_classes, 2 P classes).  A = N(0, 1), D = -onehot of a random pdf per frame (what the kernels do does not
depend on the costs' values).  The comparison to record is the ratio to expectedcost: the class term is all the entry adds.
Prints one JSON line.
    python tools/bench_classcost.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def timed_alternating(fns, K=10, W=2):
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


golden = os.path.join(ROOT, "tests", "golden")
rows = []
for name, g, B, N in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
                      ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                      ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
    f = wl.to_fsm(mm, g)
    cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    bf = mm.batch(*([cf] * B))
    V = torch.randn(B, N, g.P, device="cuda")
    D = torch.zeros(B, N, g.P, device="cuda")
    D.scatter_(2, torch.randint(0, g.P, (B, N, 1), device="cuda"), -1.0)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    marks = np.full(f.nnz, -1, dtype=np.int32)
    marks[np.random.default_rng(0).random(f.nnz) < 0.03] = 0
    for layout, (cls, nc) in (("boundary marks on 3 % of the arcs", (marks, 1)), ("loop / exit classes on every arc", mm.loop_exit_classes(f, g.state2pdf, g.P))):
        bf.set_arc_classes(cls, nc)
        A = torch.randn(B, N, nc, device="cuda")
        fns = {"classcost_ms": lambda: bf.classcost(V, A, lens),
               "classcost_D_ms": lambda: bf.classcost(V, A, lens, D=D),
               "expectedcost_ms": lambda: bf.expectedcost(V, D, lens),
               "arcclassposteriors_ms": lambda: bf.arcclassposteriors(V, lens)}
        t = timed_alternating(fns, K=10, W=2)
        row = dict(workload=name, classes=layout, C=int(nc), classified=int((np.asarray(cls) >= 0).sum()), states=g.S, arcs=g.n_arcs, B=B, T=N,
                   **{k: round(v[0], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
        row["over_expectedcost"] = round(t["classcost_ms"][0] / t["expectedcost_ms"][0], 3)
        row["D_over_expectedcost"] = round(t["classcost_D_ms"][0] / t["expectedcost_ms"][0], 3)
        row["over_arcclassposteriors"] = round(t["classcost_ms"][0] / t["arcclassposteriors_ms"][0], 3)
        row["kernels"] = bf.kernels("classcost")
        row["cost_class_cap"] = bf.info(classcost=True)["cost_class_cap"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del A
    del bf, V, D
line = json.dumps(dict(source_hash=source_hash(), rows=rows))
print(line, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(line + "\n")
