#!/usr/bin/env python3
"""Windowed best paths (mm_viterbiwindow_f32) next to the like-for-like call of the same batch -- mm_viterbi_f32 with caller-supplied
int32 back-pointers: the item kernel and mm_backtrace_kernel --: ms per call, device events after warm-up, one process, the calls
alternating.  Whole-utterance closed (and open) windows on config 5's lexicon graph (5000 states, T = 1000, B = 128) and on config
3's graph (B = 256, T = 1500) as tropical FSMs, and the streaming shape on both: streaming.OnlineViterbi with max_pending 25 pushed
50 frames at a time, the window call of 75 frames alone, and viterbi over the same 75 frames.  Each row carries the mean
len - converged of the run: the trace kernel's set work is proportional to it.  Prints one JSON line.
    python tools/bench_viterbiwindow.py [out.json]      (GPU box)"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import torch
from bench_pathentropy import timed_alternating
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")


def spread(t):
    return dict(**{k: round(v[0], 3) for k, v in t.items()}, **{k.replace("_ms", "_min_max_ms"): [round(v[1], 3), round(v[2], 3)] for k, v in t.items()})


def main():
    rows = []
    for name, g, B, N in (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                          ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500)):
        cf = mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        torch.manual_seed(0)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        ones = torch.ones(B, dtype=torch.int32, device="cuda")
        state = torch.empty(bf.total_states, device="cuda")
        fns = {"viterbiwindow_closed_ms": lambda: bf.viterbiwindow(V, lens, closed=ones, want_state=state),
               "viterbiwindow_open_converged_ms": lambda: bf.viterbiwindow(V, lens, commit_converged=True, want_state=state),
               "viterbi_with_backpointers_ms": lambda: bf.viterbi(V, lens, return_backpointers=True)}
        t = timed_alternating(fns)
        row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, **spread(t))
        for k in ("closed", "open_converged"):
            row[k + "_over_viterbi_with_backpointers"] = round(t[f"viterbiwindow_{k}_ms"][0] / t["viterbi_with_backpointers_ms"][0], 3)
        for k, cl in (("closed", ones), ("open", None)):
            conv = bf.viterbiwindow(V, lens, closed=cl)[2]
            row[f"mean_len_minus_converged_{k}"] = round(float((lens - conv).float().mean()), 2)
        row["kernels"] = bf.kernels("vitwindow")
        row["viterbi_kernels"] = bf.kernels("tropical")
        rows.append(row)
        # the streaming shape: one push = one open window over pending + chunk frames and the decoder's bookkeeping on the device
        chunk, pend = 50, 25
        dec = mm.OnlineViterbi(bf, pend)
        Vc = torch.randn(B, chunk, g.P, device="cuda")
        Vw = torch.randn(B, pend + chunk, g.P, device="cuda")
        wlen = torch.full((B,), pend + chunk, dtype=torch.int32, device="cuda")
        commit = torch.full((B,), chunk, dtype=torch.int32, device="cuda")
        t = timed_alternating({"decoder_push_ms": lambda: dec.push(Vc),
                               "window_call_alone_ms": lambda: bf.viterbiwindow(Vw, wlen, commit=commit, commit_converged=True, want_state=state),
                               "viterbi_with_backpointers_ms": lambda: bf.viterbi(Vw, wlen, return_backpointers=True)})
        row = dict(workload=name + ", streaming", states=g.S, B=B, chunk=chunk, max_pending=pend, **spread(t))
        row["push_over_viterbi_with_backpointers"] = round(t["decoder_push_ms"][0] / t["viterbi_with_backpointers_ms"][0], 3)
        row["window_call_over_viterbi_with_backpointers"] = round(t["window_call_alone_ms"][0] / t["viterbi_with_backpointers_ms"][0], 3)
        conv = bf.viterbiwindow(Vw, wlen)[2]
        row["mean_len_minus_converged_open"] = round(float((wlen - conv).float().mean()), 2)
        row["mean_npending_after"] = round(float(dec.npending.float().mean()), 2)
        row["mean_nforced_per_push"] = round(float(dec.nforced.float().mean()) / 10, 2)  # (2 warm-up + 8 timed pushes)
        rows.append(row)
        del bf, dec, V, Vc, Vw, state
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
