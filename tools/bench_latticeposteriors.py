#!/usr/bin/env python3
"""Lattice posteriors (mm_latticeposteriors_f32) next to the full mm_lattice_f32 call that produced their input, in the same run:
ms per call with and without gamma, device events after warm-up, one process, the calls alternating; records per second; the ratio
to the lattice call.  Config 5's lexicon graph (5000 states, T = 1000, B = 128) and config 3's graph (B = 256, T = 1500) as
tropical FSMs, standard-normal V, beams 4 and 8: the lattices of profiles/lattice_bench.json, whole (no record limit).  The
forward-backward kernel's workgroup of 256, 512 and 1024 threads (MM_LATPOST_NT under MM_DEBUG, read when a batch is made) side by
side, gamma included: what the default was chosen by.  And what exists without the entry for the same result: decode.lattice_fsm +
compile + batch + pdfposteriors of ONE utterance of the batch, host time included (wall clock around the four steps, the device
synchronised; the lattice of the batch already on the host is not part of it).  Prints one JSON line.
    python tools/bench_latticeposteriors.py [out.json]      (GPU box)"""
import ctypes as C
import importlib, json, os, sys, time
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
NTS = (256, 512, 1024)
TODAY_RECORD_LIMIT = 1500000  # records of the one utterance that goes the host road


def batch_with_nt(cf, B, nt):
    """the same batch with the forward-backward's workgroup of nt threads (the switches are read when a batch is made)"""
    old = {k: os.environ.get(k) for k in ("MM_DEBUG", "MM_LATPOST_NT")}
    os.environ.update(MM_DEBUG="1", MM_LATPOST_NT=str(nt))
    try:
        return mm.batch(*([cf] * B))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def one_utterance_today(bf, lat_host, V, b, P):
    """decode.lattice_fsm + compile + batch + pdfposteriors of utterance b: seconds of wall clock, and its log-sum"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lf, s2p = mm.decode.lattice_fsm(bf, lat_host, b)
    lb = mm.batch(mm.compile(lf.with_semiring("log"), mm.statemap(s2p, P)))
    _, ttl = lb.pdfposteriors(V[b : b + 1])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(ttl[0])


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
        best = torch.empty(B, device="cuda")
        logz = torch.empty(B, device="cuda")
        gamma = torch.empty((B, N, g.P), device="cuda")
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def lattice(beam, arc, score, cap):
            lib.check(lib.lib.mm_lattice_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, beam.data_ptr(), counts.data_ptr(), N,
                                             total.data_ptr(), best.data_ptr(), arc.data_ptr() if arc is not None else None,
                                             score.data_ptr() if score is not None else None, cap, st()))

        for bm in (4.0, 8.0):
            beam = torch.full((B,), bm, device="cuda")
            lattice(beam, None, None, 0)
            n = int(total.item())
            arc = torch.empty(n, dtype=torch.int32, device="cuda")
            score = torch.empty(n, dtype=torch.float32, device="cuda")
            lattice(beam, arc, score, n)
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)])
            post = torch.empty(n, dtype=torch.float32, device="cuda")

            def latpost(h, want_gamma):
                lib.check(lib.lib.mm_latticeposteriors_f32(h._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n,
                                                           None, post.data_ptr(), logz.data_ptr(), gamma.data_ptr() if want_gamma else None,
                                                           gamma.stride(0) if want_gamma else 0, gamma.stride(1) if want_gamma else 0, st()))

            latpost(bf, True)  # (the arc table goes up outside the timed calls; so does the variants')
            for h in variants.values():
                latpost(h, True)
            default_nt = int(bf.kernels("latticeposteriors").split("mm_latpost_fb_kernel<")[1].split(">")[0])
            few = n > (1 << 30)  # (seconds per call: fewer rounds)
            t = timed_alternating({"lattice_full_ms": lambda: lattice(beam, arc, score, n), "latticeposteriors_ms": lambda: latpost(bf, True),
                                   "latticeposteriors_no_gamma_ms": lambda: latpost(bf, False)}, K=3 if few else 8, W=1 if few else 2)
            tv = timed_alternating({f"latticeposteriors_nt{nt}_ms": (lambda h=h: latpost(h, True)) for nt, h in variants.items()}, K=3 if few else 8, W=1 if few else 2)
            latpost(bf, True)
            torch.cuda.synchronize()
            z = logz.cpu().numpy()
            row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, beam=bm, records=n, kept_arcs_per_frame=round(n / float(B * N), 2),
                       default_threads=default_nt, **spread(t), **spread(tv))
            row["records_per_second"] = round(n / (t["latticeposteriors_ms"][0] * 1e-3))
            row["records_per_second_no_gamma"] = round(n / (t["latticeposteriors_no_gamma_ms"][0] * 1e-3))
            row["us_per_step_no_gamma"] = round(t["latticeposteriors_no_gamma_ms"][0] * 1e3 / (2 * N), 3)  # (a forward and a backward step per frame; the utterances run side by side)
            for k in ("latticeposteriors", "latticeposteriors_no_gamma"):
                row[k + "_over_lattice_full"] = round(t[k + "_ms"][0] / t["lattice_full_ms"][0], 3)
            row["logz_minus_best_mean"] = round(float(np.mean(z - best.cpu().numpy())), 4)
            # what exists today, for one utterance (twice: the second run has every lazily built piece in place) -- where its
            # lattice is small enough to be built as a Python FSM in reasonable time
            n0 = int(offsets[N].item())
            row["today_utterance_records"] = n0
            if n0 <= TODAY_RECORD_LIMIT:
                lat_host = mm.Lattice(counts.cpu().numpy(), offsets.cpu().numpy(), arc[:n0].cpu().numpy(), score[:n0].cpu().numpy(), best.cpu().numpy())
                secs = [one_utterance_today(bf, lat_host, V, 0, g.P) for _ in range(2)]
                row["today_one_utterance_ms"] = round(min(s for s, _ in secs) * 1e3, 1)
                row["today_one_utterance_logz"] = round(secs[0][1], 3)
                row["this_entry_logz_of_that_utterance"] = round(float(z[0]), 3)
                row["batch_over_today_one_utterance"] = round(t["latticeposteriors_ms"][0] / row["today_one_utterance_ms"], 4)
            else:
                row["today_one_utterance_ms"] = None  # (not run: a Python FSM of that many arcs)
            row["kernels"] = bf.kernels("latticeposteriors")
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del arc, score, post, offsets
            torch.cuda.empty_cache()
        del bf, variants, V, gamma
        torch.cuda.empty_cache()
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
