#!/usr/bin/env python3
"""Forward filtering posteriors (mm_filterposteriors_f32), with filt and likelihood only, next to the two existing calls of the
same batch nearest to it -- the item kernel's pdfposteriors (MM_KERNEL=item) and the value-only pathentropy (a forward kernel
alone) --: ms per call, device events after warm-up, one process, the calls alternating, for config 3 (B = 256, T = 1500), config 3
at T = 150 (a streaming chunk), the WSJ denominator (B = 128, T = 700) and the WSJ numerator x 128 (T = 700).  Prints one JSON line.
    python tools/bench_filterposteriors.py [out.json]      (GPU box)"""
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
                          ("config 3, T = 150", den3, 256, 150),
                          ("WSJ denominator", wl.load_npz_graph(os.path.join(golden, "den_fsm_wsj.npz")), 128, 700),
                          ("WSJ numerator x128", wl.load_npz_graph(os.path.join(golden, "num_fsm_wsj.npz")), 128, 700)):
        cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        bi = item_batch(cf, B)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        gam = torch.empty(B, N, g.P, device="cuda")
        state = torch.empty(bf.total_states, device="cuda")
        fns = {"filterposteriors_ms": lambda: bf.filterposteriors(V, lens, out=gam, want_state=state),
               "filterposteriors_no_filt_ms": lambda: bf.filterposteriors(V, lens, want_state=state, want_filt=False),
               "pdfposteriors_item_ms": lambda: bi.pdfposteriors(V, lens, out=gam),
               "pathentropy_value_only_ms": lambda: bf.pathentropy(V, lens, want_grad=False)}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, **{k: round(v[0], 3) for k, v in t.items()},
                   **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})
        row["over_pdfposteriors_item"] = round(t["filterposteriors_ms"][0] / t["pdfposteriors_item_ms"][0], 3)
        row["over_pathentropy_value_only"] = round(t["filterposteriors_ms"][0] / t["pathentropy_value_only_ms"][0], 3)
        row["no_filt_over_full"] = round(t["filterposteriors_no_filt_ms"][0] / t["filterposteriors_ms"][0], 3)
        row["kernels"] = bf.kernels("filter")
        rows.append(row)
        del bf, bi, V, gam, state
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
