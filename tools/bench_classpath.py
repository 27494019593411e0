#!/usr/bin/env python3
"""Best paths with arc classes (mm_classpath_f32) next to the like-for-like call of the same batch -- mm_viterbi_f32 with
caller-supplied int32 back-pointers: the item kernel and mm_backtrace_kernel --: ms per call, device events after warm-up, one
process, the calls alternating.  Config 5's lexicon graph (5000 states, T = 1000, B = 128) and config 3's graph (B = 256, T = 1500)
as tropical FSMs; U NULL and U given; two class layouts: boundary marks on ~3 % of the arcs (three classes, the rest
unclassified) and every arc by its destination's pdf.  Prints one JSON line.
    python tools/bench_classpath.py [out.json]      (GPU box)"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import numpy as np
import torch
from bench_pathentropy import timed_alternating
from bench_viterbiwindow import spread
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def layouts(g, f):
    """(name, cls, C): boundary marks on ~3 % of the entries in three classes; every entry by its destination's pdf."""
    S1 = f.colptr.size - 1
    j = np.repeat(np.arange(S1), np.diff(np.asarray(f.colptr)))
    marks = np.full(f.nnz, -1, dtype=np.int32)
    pick = np.random.default_rng(0).random(f.nnz) < 0.03
    marks[pick] = np.arange(f.nnz)[pick] % 3
    dst = np.concatenate([np.asarray(g.state2pdf), [g.P]])[j].astype(np.int32)
    return [("boundary marks, 3 %", marks, 3), ("destination pdf", dst, g.P + 1)]


def main():
    rows = []
    for name, g, B, N in (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                          ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500)):
        f = wl.to_fsm(mm, g, semiring="tropical")
        bf = mm.batch(*([mm.compile(f, mm.statemap(g.state2pdf, g.P))] * B))
        torch.manual_seed(0)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        for lname, cls, nc in layouts(g, f):
            bf.set_path_classes(cls, nc)
            U = torch.randn(B, N, nc, device="cuda")
            fns = {"classpath_u_null_ms": lambda: bf.classpath(V, None, lens),
                   "classpath_u_given_ms": lambda: bf.classpath(V, U, lens),
                   "classpath_no_classes_out_ms": lambda: bf.classpath(V, None, lens, want_classes=False),
                   "viterbi_with_backpointers_ms": lambda: bf.viterbi(V, lens, return_backpointers=True)}
            t = timed_alternating(fns)
            row = dict(workload=name, layout=lname, classes=nc, states=g.S, arcs=g.n_arcs, B=B, T=N, **spread(t))
            for k in ("u_null", "u_given", "no_classes_out"):
                row[k + "_over_viterbi_with_backpointers"] = round(t[f"classpath_{k}_ms"][0] / t["viterbi_with_backpointers_ms"][0], 3)
            row["kernels"] = bf.kernels("classpath")
            row["viterbi_kernels"] = bf.kernels("tropical")
            rows.append(row)
            del U
        del bf, V
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
