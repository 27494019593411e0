#!/usr/bin/env python3
"""Segment posteriors (mm_segmentposteriors_f32) and the two-pass driver BatchedFSM.chunkedposteriors next to the one closed
windowposteriors call of the same batch: ms per call, device events after warm-up, one process, the calls alternating, 8 rounds,
median [min, max], for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).
The segment call ends every utterance on a carried end vector (one item pass and one vector more than the closed window); the
driver runs at chunk = T / 10; mm_batch_workspace_bytes at N = T and at N = chunk stands beside them.  No threshold: the figures
are written down.  Prints one JSON line.
    python tools/bench_segmentposteriors.py [out.json]      (GPU box)"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")
lib = importlib.import_module(mm.__name__ + "._lib").lib


def timed_alternating(fns, K=8, W=2):
    """median and spread (min, max) in ms of each call of `fns`, the calls taking turns: round r runs every call once"""
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
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in t.items()}


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    rows = []
    for name, g, B, N in (("config 3 (lfmmi_den)", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500),
                          ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                          ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
        cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        chunk = N // 10
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        ones = torch.ones(B, dtype=torch.int32, device="cuda")
        twos = torch.full((B,), 2, dtype=torch.int32, device="cuda")
        gam = torch.empty(B, N, g.P, device="cuda")
        state = torch.empty(bf.total_states, device="cuda")
        end = torch.log(torch.rand(bf.total_states, device="cuda"))
        end_out = torch.empty(bf.total_states, device="cuda")
        fns = {"windowposteriors_closed_ms": lambda: bf.windowposteriors(V, lens, closed=ones, out=gam, want_state=state),
               "segmentposteriors_carried_ms": lambda: bf.segmentposteriors(V, lens, end_mode=twos, end=end, out=gam, want_end=end_out),
               "chunkedposteriors_ms": lambda: bf.chunkedposteriors(V, lens, chunk=chunk, out=gam)}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, chunk=chunk, **{k: round(v[0], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
        row["segment_over_window_closed"] = round(t["segmentposteriors_carried_ms"][0] / t["windowposteriors_closed_ms"][0], 3)
        row["chunked_over_window_closed"] = round(t["chunkedposteriors_ms"][0] / t["windowposteriors_closed_ms"][0], 3)
        row["workspace_bytes_T"] = int(lib.mm_batch_workspace_bytes(bf._h, N))
        row["workspace_bytes_chunk"] = int(lib.mm_batch_workspace_bytes(bf._h, chunk))
        row["kernels"] = bf.kernels("segment")
        rows.append(row)
        del bf, V, gam, state, end, end_out
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
