#!/usr/bin/env python3
"""Fixed-lag smoothing posteriors (mm_windowposteriors_f32), closed and open, next to the two existing calls of the same batch nearest
to it -- leakyposteriors(leak = 0) and the item kernel's pdfposteriors (MM_KERNEL=item) --: ms per call, device events after
warm-up, one process, the calls alternating, for config 3 (B = 256, T = 1500), the WSJ denominator (B = 128, T = 700) and the WSJ
numerator x 128 (T = 700); and the streaming shape: config 3's graph, B = 256, streaming.FixedLagSmoother with lag 25 pushed 50
frames at a time, next to streaming.ForwardFilter on the same chunks.  Prints one JSON line.
    python tools/bench_windowposteriors.py [out.json]      (GPU box)"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from bench_pathentropy import item_batch, timed_alternating
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    den3 = wl.lfmmi_denominator(2000, 84, seed=0)
    rows = []
    for name, g, B, N in (("config 3 (lfmmi_den)", den3, 256, 1500),
                          ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                          ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
        cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        bi = item_batch(cf, B)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        ones = torch.ones(B, dtype=torch.int32, device="cuda")
        gam = torch.empty(B, N, g.P, device="cuda")
        state = torch.empty(bf.total_states, device="cuda")
        fns = {"windowposteriors_closed_ms": lambda: bf.windowposteriors(V, lens, closed=ones, out=gam, want_state=state),
               "windowposteriors_open_ms": lambda: bf.windowposteriors(V, lens, out=gam, want_state=state),
               "leakyposteriors_leak0_ms": lambda: bf.leakyposteriors(V, lens, leak=0.0, out=gam),
               "pdfposteriors_item_ms": lambda: bi.pdfposteriors(V, lens, out=gam)}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, **{k: round(v[0], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
        for k in ("closed", "open"):
            row[k + "_over_leakyposteriors_leak0"] = round(t[f"windowposteriors_{k}_ms"][0] / t["leakyposteriors_leak0_ms"][0], 3)
            row[k + "_over_pdfposteriors_item"] = round(t[f"windowposteriors_{k}_ms"][0] / t["pdfposteriors_item_ms"][0], 3)
        row["kernels"] = bf.kernels("window")
        rows.append(row)
        del bf, bi, V, gam, state
    # the streaming shape: one push = one open window over lag + chunk frames and the smoother's bookkeeping on the device
    B, chunk, lag = 256, 50, 25
    cf = mm.compile(wl.to_fsm(mm, den3), mm.statemap(den3.state2pdf, den3.P))
    bf = mm.batch(*([cf] * B))
    sm, ff = mm.FixedLagSmoother(bf, lag), mm.ForwardFilter(bf)
    V = torch.randn(B, chunk, den3.P, device="cuda")
    Vw = torch.randn(B, lag + chunk, den3.P, device="cuda")
    wlen = torch.full((B,), lag + chunk, dtype=torch.int32, device="cuda")
    commit = torch.full((B,), chunk, dtype=torch.int32, device="cuda")
    state = torch.zeros(bf.total_states, device="cuda")
    t = timed_alternating({"smoother_push_ms": lambda: sm.push(V), "filter_push_ms": lambda: ff.push(V),
                           "window_call_alone_ms": lambda: bf.windowposteriors(Vw, wlen, commit=commit, want_state=state)})
    row = dict(workload="config 3 graph, streaming", states=den3.S, B=B, chunk=chunk, lag=lag, **{k: round(v[0], 3) for k, v in t.items()},
               **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
    row["smoother_push_over_filter_push"] = round(t["smoother_push_ms"][0] / t["filter_push_ms"][0], 3)
    rows.append(row)
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
