#!/usr/bin/env python3
"""Posterior path sampling (mm_samplepaths_f32) at K = 1, 8, 64 next to the two calls that share its forward half on the same
batch -- arcposteriors and the item kernel's pdfposteriors (MM_KERNEL=item) --: ms per call, device events after warm-up, the
calls alternating, for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128
(T = 700).  Also the same sampling calls with the alpha~ rows gathered from global memory instead of staged in LDS
(MM_SAMPLE_NOSTAGE).  Prints one JSON line.
    python tools/bench_samplepaths.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")
KS = (1, 8, 64)


def timed_alternating(fns, K=8, W=2):
    """mean ms of each call of `fns`, the calls taking turns: round r runs every call once"""
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
    return {k: float(np.mean([a.elapsed_time(b) for a, b in ev[k]])) for k in fns}


def debug_batch(cf, B, **env):
    """the same batch made under debug switches (they are read when a batch is made)"""
    env = dict(MM_DEBUG="1", **env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
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
    bi = debug_batch(cf, B, MM_KERNEL="item")
    bg = debug_batch(cf, B, MM_SAMPLE_NOSTAGE="1")
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    gam = torch.empty(B, N, g.P, device="cuda")
    fns = {"arcposteriors_ms": lambda: bf.arcposteriors(V, lens, want_init=True),
           "pdfposteriors_item_ms": lambda: bi.pdfposteriors(V, lens, out=gam)}
    for k in KS:
        fns[f"samplepaths_K{k}_ms"] = lambda k=k: bf.samplepaths(V, lens, nsamples=k, seed=1, want_logprob=True)
        fns[f"samplepaths_global_K{k}_ms"] = lambda k=k: bg.samplepaths(V, lens, nsamples=k, seed=1, want_logprob=True)
    t = timed_alternating(fns)
    row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, **{k: round(v, 3) for k, v in t.items()})
    row["K1_over_arcposteriors"] = round(t["samplepaths_K1_ms"] / t["arcposteriors_ms"], 3)
    row["K1_over_pdfposteriors_item"] = round(t["samplepaths_K1_ms"] / t["pdfposteriors_item_ms"], 3)
    row["K64_over_K1"] = round(t["samplepaths_K64_ms"] / t["samplepaths_K1_ms"], 3)
    row["kernels"] = bf.kernels("sample")
    rows.append(row)
    del bf, bi, bg, V, gam
line = json.dumps(dict(source_hash=source_hash(), rows=rows))
print(line, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(line + "\n")
