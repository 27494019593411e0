#!/usr/bin/env python3
"""Leaky-HMM pdf posteriors (mm_leakyposteriors_f32, leak = 1e-5) next to the item kernel's pdfposteriors of the same batch
(MM_KERNEL=item; with atomics, and in its deterministic mode, whose two barriers per backward step the leaky backward kernel
shares): ms per call, device events after warm-up, the calls alternating, one process per workload -- config 3 (B = 256,
T = 1500), config 3 at the chunk length T = 150, the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).
Prints one JSON line.
    python tools/bench_leakyposteriors.py [out.json]      (GPU box)"""
import importlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = ("config3", "config3_chunk", "wsj_den", "wsj_num")


def run_one(which):
    import numpy as np
    import __graft_entry__ as ge
    import torch
    mm = ge.load_package()
    wl = importlib.import_module(mm.__name__ + ".workloads")
    golden = os.path.join(ROOT, "tests", "golden")
    name, g, B, N = {
        "config3": lambda: ("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
        "config3_chunk": lambda: ("config 3, chunks of 150 frames", wl.lfmmi_denominator(2000, 84, seed=0), 256, 150),
        "wsj_den": lambda: ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
        "wsj_num": lambda: ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700),
    }[which]()

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

    cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
    bf = mm.batch(*([cf] * B))
    bi, bd = item_batch(cf, B), item_batch(cf, B).set_deterministic(True)
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    gam = torch.empty(B, N, g.P, device="cuda")
    fns = {"leakyposteriors_ms": lambda: bf.leakyposteriors(V, lens, leak=1e-5, out=gam),
           "pdfposteriors_item_ms": lambda: bi.pdfposteriors(V, lens, out=gam),
           "pdfposteriors_item_deterministic_ms": lambda: bd.pdfposteriors(V, lens, out=gam)}
    t = timed_alternating(fns)
    row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, leak=1e-5, **{k: round(v[0], 3) for k, v in t.items()},
               **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
    row["over_pdfposteriors_item"] = round(t["leakyposteriors_ms"][0] / t["pdfposteriors_item_ms"][0], 3)
    row["over_pdfposteriors_item_deterministic"] = round(t["leakyposteriors_ms"][0] / t["pdfposteriors_item_deterministic_ms"][0], 3)
    row["deterministic_over_item"] = round(t["pdfposteriors_item_deterministic_ms"][0] / t["pdfposteriors_item_ms"][0], 3)
    row["kernels"] = bf.kernels("leaky")
    print("ROW " + json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        run_one(sys.argv[2])
        sys.exit(0)
    from srchash import source_hash
    rows = []
    for w in WORKLOADS:  # a fresh process per workload: no workspace, cache or clock state of one reaches the next
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", w], check=True, capture_output=True, text=True, timeout=900).stdout
        rows.append(json.loads([l for l in out.splitlines() if l.startswith("ROW ")][-1][4:]))
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")
