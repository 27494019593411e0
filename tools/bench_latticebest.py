#!/usr/bin/env python3
"""Lattice best paths (mm_latticebest_f32) next to mm_latticeposteriors_f32 without gamma on the same lattice, in the same run: ms
per call with and without rec / path, device events after warm-up, one process, the calls alternating; the ratio to the posteriors
(three passes and fixed-point sums per step there, one pass of adds and integer maxima here); microseconds per step; records per
second.  The four lattices of tools/bench_latticeposteriors.py: config 5's lexicon graph (5000 states, T = 1000, B = 128) and config
3's graph (B = 256, T = 1500) as tropical FSMs, standard-normal V, beams 4 and 8, whole.  The kernel's workgroup of 256, 512 and 1024
threads (MM_LATPOST_NT under MM_DEBUG, read when a batch is made) side by side, rec / path included: what the default is judged by.
Prints one JSON line.
    python tools/bench_latticebest.py [out.json]      (GPU box)"""
import ctypes as C
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge
import numpy as np
import torch
from bench_latticeposteriors import NTS, batch_with_nt
from bench_pathentropy import timed_alternating
from bench_viterbiwindow import spread
from srchash import source_hash
mm = ge.load_package()
wl = importlib.import_module(mm.__name__ + ".workloads")
lib = importlib.import_module(mm.__name__ + "._lib")


def main():
    rows = []
    for name, g, B, N in (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                          ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500)):
        f = wl.to_fsm(mm, g, semiring="tropical")
        cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        variants = {nt: batch_with_nt(cf, B, nt) for nt in NTS}
        torch.manual_seed(0)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        counts = torch.empty((B, N), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        lbest = torch.empty(B, device="cuda")
        best = torch.empty(B, device="cuda")
        logz = torch.empty(B, device="cuda")
        rec = torch.empty((B, N), dtype=torch.int64, device="cuda")
        path = torch.empty((B, N), dtype=torch.int32, device="cuda")
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def lattice(beam, arc, score, cap):
            lib.check(lib.lib.mm_lattice_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, beam.data_ptr(), counts.data_ptr(), N,
                                             total.data_ptr(), lbest.data_ptr(), arc.data_ptr() if arc is not None else None,
                                             score.data_ptr() if score is not None else None, cap, st()))

        for bm in (4.0, 8.0):
            beam = torch.full((B,), bm, device="cuda")
            lattice(beam, None, None, 0)
            n = int(total.item())
            arc = torch.empty(n, dtype=torch.int32, device="cuda")
            lscore = torch.empty(n, dtype=torch.float32, device="cuda")
            lattice(beam, arc, lscore, n)
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)])
            out = torch.empty(n, dtype=torch.float32, device="cuda")  # (score here, post there: the calls alternate)

            def latbest(h, want_path):
                lib.check(lib.lib.mm_latticebest_f32(h._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                     None, best.data_ptr(), out.data_ptr(), rec.data_ptr() if want_path else None, N,
                                                     path.data_ptr() if want_path else None, N, st()))

            def latpost(h):
                lib.check(lib.lib.mm_latticeposteriors_f32(h._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                           None, out.data_ptr(), logz.data_ptr(), None, 0, 0, st()))

            latpost(bf)  # (the arc table goes up outside the timed calls; so does the variants')
            for h in variants.values():
                latbest(h, True)
            latbest(bf, True)
            torch.cuda.synchronize()
            # on the lattice's own V the through-scores are the lattice's up to the rounding of the sums, and the path's are 0
            dev = float((out - lscore).abs().max().item())
            on_path = float(out[rec.reshape(-1)].abs().max().item())
            same_best = float((best - lbest).abs().max().item())
            default_nt = int(bf.kernels("latticebest").split("mm_latbest_kernel<")[1].split(">")[0])
            few = n > (1 << 30)  # (fewer rounds on the largest lattice)
            t = timed_alternating({"latticebest_ms": lambda: latbest(bf, True), "latticebest_no_path_ms": lambda: latbest(bf, False),
                                   "latticeposteriors_no_gamma_ms": lambda: latpost(bf)}, K=4 if few else 10, W=1 if few else 3)
            tv = timed_alternating({f"latticebest_nt{nt}_ms": (lambda h=h: latbest(h, True)) for nt, h in variants.items()}, K=4 if few else 10, W=1 if few else 3)
            row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, beam=bm, records=n, kept_arcs_per_frame=round(n / float(B * N), 2),
                       default_threads=default_nt, **spread(t), **spread(tv))
            row["records_per_second"] = round(n / (t["latticebest_ms"][0] * 1e-3))
            row["us_per_step"] = round(t["latticebest_ms"][0] * 1e3 / (2 * N), 3)  # (a forward and a backward step per frame; the utterances run side by side)
            row["us_per_step_no_path"] = round(t["latticebest_no_path_ms"][0] * 1e3 / (2 * N), 3)
            row["latticebest_over_latticeposteriors_no_gamma"] = round(t["latticebest_ms"][0] / t["latticeposteriors_no_gamma_ms"][0], 3)
            row["latticebest_no_path_over_latticeposteriors_no_gamma"] = round(t["latticebest_no_path_ms"][0] / t["latticeposteriors_no_gamma_ms"][0], 3)
            row["max_abs_score_minus_lattice_score"] = dev
            row["max_abs_score_on_the_path"] = on_path
            row["max_abs_best_minus_lattice_best"] = same_best
            row["kernels"] = bf.kernels("latticebest")
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del arc, lscore, out, offsets
            torch.cuda.empty_cache()
        del bf, variants, V
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
