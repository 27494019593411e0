#!/usr/bin/env python3
"""Posteriors with call-time arc weights (mm_weightedposteriors_f32) with one shared weight vector, with a vector per utterance and
with both weight arguments NULL, next to what the same batch costs today for the same outputs -- arcposteriors alone, and
arcposteriors followed by the item kernel's pdfposteriors (MM_KERNEL=item), which runs the forward pass twice --: ms per call,
device events after warm-up, one process, the calls alternating over 8 rounds, min / median / max, for config 3 (B = 256,
T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).  Prints one JSON line.
    python tools/bench_weightedposteriors.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def timed_alternating(fns, K=8, W=2):
    """(min, median, max) in ms of each call of `fns`, the calls taking turns: round r runs every call once"""
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
    return {k: (float(np.min(v)), float(np.median(v)), float(np.max(v))) for k, v in t.items()}


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
        f = wl.to_fsm(mm, g)
        cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        bi = item_batch(cf, B)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        gam = torch.empty(B, N, g.P, device="cuda")
        W1 = torch.from_numpy(np.asarray(f.nzval, dtype=np.float32)).cuda()
        WB = (W1[None, :] + 0.1 * torch.randn(B, f.nnz, device="cuda")).contiguous()

        def pair():
            bf.arcposteriors(V, lens)
            bi.pdfposteriors(V, lens, out=gam)

        fns = {"weighted_shared_ms": lambda: bf.weightedposteriors(V, W1, None, lens, out=gam),
               "weighted_per_utterance_ms": lambda: bf.weightedposteriors(V, WB, None, lens, out=gam),
               "weighted_null_ms": lambda: bf.weightedposteriors(V, None, None, lens, out=gam),
               "arcposteriors_ms": lambda: bf.arcposteriors(V, lens),
               "arcs_then_pdfposteriors_item_ms": pair}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, entries=f.nnz, B=B, T=N, **{k: round(v[1], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[0], 3), round(v[2], 3)] for k, v in t.items()})
        med = {k: v[1] for k, v in t.items()}
        row["shared_over_pair"] = round(med["weighted_shared_ms"] / med["arcs_then_pdfposteriors_item_ms"], 3)
        row["per_utterance_over_pair"] = round(med["weighted_per_utterance_ms"] / med["arcs_then_pdfposteriors_item_ms"], 3)
        row["null_over_pair"] = round(med["weighted_null_ms"] / med["arcs_then_pdfposteriors_item_ms"], 3)
        row["null_over_arcposteriors"] = round(med["weighted_null_ms"] / med["arcposteriors_ms"], 3)
        row["prologue_share_shared"] = round((med["weighted_shared_ms"] - med["weighted_null_ms"]) / med["weighted_shared_ms"], 4)
        row["prologue_share_per_utterance"] = round((med["weighted_per_utterance_ms"] - med["weighted_null_ms"]) / med["weighted_per_utterance_ms"], 4)
        row["kernels"] = bf.kernels("weighted")
        rows.append(row)
        del bf, bi, V, gam, WB
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
