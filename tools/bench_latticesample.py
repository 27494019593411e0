#!/usr/bin/env python3
"""Lattice path sampling (mm_latticesample_f32) at K = 1, 8, 64 and 256 samples per utterance next to mm_latticebest_f32 with rec / path
and mm_latticeposteriors_f32 without gamma on the same lattice, in the same run: ms per call, device events after warm-up, one
process, the calls alternating.  The yardstick the design is judged by is latticeposteriors' forward pass plus one latticebest-style
backward scan per 64 samples: the forward pass's share of a call and the time per step of either kernel come from the device times
of the two kernels, read off one profiled pass per K (torch.profiler; null where the profiler names no kernel).  The four lattices
of tools/bench_latticebest.py: config 5's lexicon graph (5000 states, T = 1000, B = 128) and config 3's graph (B = 256, T = 1500) as
tropical FSMs, standard-normal V, beams 4 and 8, whole.  Prints one JSON line.
    python tools/bench_latticesample.py [out.json]      (GPU box)"""
import ctypes as C
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
lib = importlib.import_module(mm.__name__ + "._lib")
KS = (1, 8, 64, 256)


def kernel_times(fn, rounds=3):
    """Mean device ms of the forward pass and of the draw over `rounds` profiled calls of fn: (fwd, draw), or None."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(rounds):
                fn()
            torch.cuda.synchronize()
        fwd = draw = None
        for e in prof.key_averages():
            total = getattr(e, "device_time_total", None)
            total = getattr(e, "cuda_time_total", 0.0) if total is None else total
            if "mm_latsample_fwd_kernel" in e.key:
                fwd = total / e.count * 1e-3
            elif "mm_latsample_kernel" in e.key:
                draw = total / e.count * 1e-3
        return None if fwd is None or draw is None else (fwd, draw)
    except Exception as err:  # (a measurement aid: the call times above stand without it)
        print(f"kernel_times: {err!r}", file=sys.stderr)
        return None


def main():
    rows = []
    for name, g, B, N in (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                          ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500)):
        f = wl.to_fsm(mm, g, semiring="tropical")
        cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
        bf = mm.batch(*([cf] * B))
        torch.manual_seed(0)
        V = torch.randn(B, N, g.P, device="cuda")
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        counts = torch.empty((B, N), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        lbest = torch.empty(B, device="cuda")
        best = torch.empty(B, device="cuda")
        logz = torch.empty(B, device="cuda")
        rec1 = torch.empty((B, N), dtype=torch.int64, device="cuda")
        path1 = torch.empty((B, N), dtype=torch.int32, device="cuda")
        Kmax = max(KS)
        rec = torch.empty((B, Kmax, N), dtype=torch.int64, device="cuda")
        path = torch.empty((B, Kmax, N), dtype=torch.int32, device="cuda")
        logprob = torch.empty((B, Kmax), device="cuda")
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
            del lscore
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)])
            out = torch.empty(n, dtype=torch.float32, device="cuda")  # (fwd here, score and post there: the calls alternate)

            def sample(K):
                lib.check(lib.lib.mm_latticesample_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                       None, K, 1, out.data_ptr(), rec.data_ptr(), Kmax * N, N, path.data_ptr(), Kmax * N, N, logprob.data_ptr(),
                                                       Kmax, logz.data_ptr(), st()))

            def latbest():
                lib.check(lib.lib.mm_latticebest_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                     None, best.data_ptr(), out.data_ptr(), rec1.data_ptr(), N, path1.data_ptr(), N, st()))

            def latpost():
                lib.check(lib.lib.mm_latticeposteriors_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                           None, out.data_ptr(), logz.data_ptr(), None, 0, 0, st()))

            latpost()  # (the arc table goes up outside the timed calls)
            zpost = logz.clone()
            sample(Kmax)
            torch.cuda.synchronize()
            same_logz = bool((logz == zpost).all().item())
            valid = bool((rec >= 0).all().item()) and bool((path >= 0).all().item())
            mean_logprob = float(logprob.mean().item())
            few = n > (1 << 30)  # (fewer rounds on the largest lattice)
            fns = {f"latticesample_k{K}_ms": (lambda K=K: sample(K)) for K in KS}
            fns.update(latticebest_ms=latbest, latticeposteriors_no_gamma_ms=latpost)
            t = timed_alternating(fns, K=4 if few else 10, W=1 if few else 3)
            row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, beam=bm, records=n, kept_arcs_per_frame=round(n / float(B * N), 2), **spread(t))
            for K in KS:
                ms = t[f"latticesample_k{K}_ms"][0]
                row[f"latticesample_k{K}_over_latticeposteriors_no_gamma"] = round(ms / t["latticeposteriors_no_gamma_ms"][0], 3)
                row[f"latticesample_k{K}_over_latticebest"] = round(ms / t["latticebest_ms"][0], 3)
                row[f"us_per_step_k{K}"] = round(ms * 1e3 / (2 * N), 3)  # (a forward and a backward step per frame)
                kt = kernel_times(lambda K=K: sample(K))
                row[f"kernel_ms_k{K}"] = None if kt is None else dict(forward=round(kt[0], 3), draw=round(kt[1], 3), forward_share=round(kt[0] / (kt[0] + kt[1]), 3),
                                                                      forward_us_per_step=round(kt[0] * 1e3 / N, 3), draw_us_per_step=round(kt[1] * 1e3 / N, 3))
            row["samples_per_second_k256"] = round(B * 256 / (t["latticesample_k256_ms"][0] * 1e-3))
            row["logz_equals_latticeposteriors_bitwise"] = same_logz
            row["every_sample_complete"] = valid
            row["mean_logprob_k256"] = round(mean_logprob, 3)
            row["kernels"] = bf.kernels("latticesample")
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del arc, out, offsets
            torch.cuda.empty_cache()
        del bf, V
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
