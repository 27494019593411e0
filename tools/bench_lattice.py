#!/usr/bin/env python3
"""Beam-pruned best-path lattices (mm_lattice_f32) next to mm_maxstateposteriors_f32 of the same batch in the same run -- the two
tropical recursions are common to both, so the ratio is the cost of the new passes over the arcs --: ms per call for the count-only
call and for the full call, device events after warm-up, one process, the calls alternating; kept arcs per frame.  Config 5's
lexicon graph (5000 states, T = 1000, B = 128) and config 3's graph (B = 256, T = 1500) as tropical FSMs, standard-normal V, beams
4, 8 and 16.  The entry is called through the C ABI into buffers made once (BatchedFSM.lattice with max_arcs None reads the total
back between its two calls: that synchronisation is not part of the figures).  Where the records of a beam exceed RECORD_LIMIT the
full call runs with cap = RECORD_LIMIT (the write pass still evaluates every arc and writes the first cap records); the row says so.
Prints one JSON line.
    python tools/bench_lattice.py [out.json]      (GPU box)"""
import ctypes as C
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from bench_pathentropy import timed_alternating
from bench_viterbiwindow import spread
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")
lib = importlib.import_module(mm.__name__ + "._lib")
RECORD_LIMIT = 1 << 30  # records (8 GB of arc + score)


def main():
    rows = []
    for name, g, B, N in (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                          ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500)):
        f = wl.to_fsm(mm, g, semiring="tropical")
        bf = mm.batch(*([mm.compile(f, mm.statemap(g.state2pdf, g.P))] * B))
        torch.manual_seed(0)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        counts = torch.empty((B, N), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        best = torch.empty(B, device="cuda")
        mu = torch.empty((N + 1, bf.total_states), device="cuda")
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(beam, arc, score, cap):
            lib.check(lib.lib.mm_lattice_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, beam.data_ptr(), counts.data_ptr(), N,
                                             total.data_ptr(), best.data_ptr(), arc.data_ptr() if arc is not None else None,
                                             score.data_ptr() if score is not None else None, cap, st()))

        def maxstate():
            lib.check(lib.lib.mm_maxstateposteriors_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, mu.data_ptr(), mu.stride(0), st()))

        for bm in (4.0, 8.0, 16.0):
            beam = torch.full((B,), bm, device="cuda")
            call(beam, None, None, 0)
            n = int(total.item())
            cap = min(n, RECORD_LIMIT)
            arc = torch.empty(cap, dtype=torch.int32, device="cuda")
            score = torch.empty(cap, dtype=torch.float32, device="cuda")
            fns = {"lattice_count_only_ms": lambda: call(beam, None, None, 0), "lattice_full_ms": lambda: call(beam, arc, score, cap),
                   "maxstateposteriors_ms": maxstate}
            t = timed_alternating(fns)
            row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, beam=bm, records=n, cap=cap, full_call_truncated=cap < n,
                       kept_arcs_per_frame=round(n / float(B * N), 2), **spread(t))
            for k in ("count_only", "full"):
                row[k + "_over_maxstateposteriors"] = round(t[f"lattice_{k}_ms"][0] / t["maxstateposteriors_ms"][0], 3)
            row["kernels"] = bf.kernels("lattice")
            rows.append(row)
            del arc, score
            torch.cuda.empty_cache()
        del bf, V, mu
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
