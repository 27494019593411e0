#!/usr/bin/env python3
"""Lattice expected cost (mm_latticecost_f32) next to mm_latticeposteriors_f32 with gamma on the same lattice, in the same run: ms
per call with and without grad, device events after warm-up, the calls alternating; the ratio to the posteriors call; the time per
step of the forward-backward (the call without grad is that kernel alone; with grad minus without is the per-pdf kernel).  The four
lattices of profiles/latticeposteriors_bench.json: config 5's lexicon graph (5000 states, T = 1000, B = 128) and config 3's graph
(B = 256, T = 1500) as tropical FSMs, standard-normal V, beams 4 and 8, whole; standard-normal costs.  Every lattice is measured
in a child process of its own under a time limit of its own; a child that fails or runs out of time ends the run.  Prints one
JSON line.
    python tools/bench_latticecost.py [out.json]      (GPU box)"""
import ctypes as C
import importlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS = [(w, bm) for w in (0, 1) for bm in (4.0, 8.0)]
LIMIT_S = 420  # of one child: graph, lattice and 3 x 10 calls of at most 0.3 s


def measure(which, bm):
    import __graft_entry__ as ge
    import torch
    from bench_pathentropy import timed_alternating
    from bench_viterbiwindow import spread
    mm = ge.load_package()
    wl = importlib.import_module(mm.__name__ + ".workloads")
    lib = importlib.import_module(mm.__name__ + "._lib")
    name, g, B, N = (("config 5 (lexicon5000)", wl.lexicon_fsm(5000, 84, seed=0), 128, 1000),
                     ("config 3 graph (lfmmi_den), tropical", wl.lfmmi_denominator(2000, 84, seed=0), 256, 1500))[which]
    bf = mm.batch(*([mm.compile(wl.to_fsm(mm, g, semiring="tropical"), mm.statemap(g.state2pdf, g.P))] * B))
    torch.manual_seed(0)
    V = torch.randn(B, N, g.P, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    counts = torch.empty((B, N), dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    best, logz, risk = (torch.empty(B, device="cuda") for _ in range(3))
    grad, gamma = (torch.empty((B, N, g.P), device="cuda") for _ in range(2))
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    beam = torch.full((B,), bm, device="cuda")

    def lattice(arc, score, cap):
        lib.check(lib.lib.mm_lattice_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, beam.data_ptr(), counts.data_ptr(), N,
                                         total.data_ptr(), best.data_ptr(), arc.data_ptr() if arc is not None else None,
                                         score.data_ptr() if score is not None else None, cap, st()))

    lattice(None, None, 0)
    n = int(total.item())
    arc = torch.empty(n, dtype=torch.int32, device="cuda")
    score = torch.empty(n, dtype=torch.float32, device="cuda")
    lattice(arc, score, n)
    del score
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)])
    post, diff = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    cost = torch.randn(n, device="cuda")

    def latpost():
        lib.check(lib.lib.mm_latticeposteriors_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n, None,
                                                   post.data_ptr(), logz.data_ptr(), gamma.data_ptr(), gamma.stride(0), gamma.stride(1), st()))

    def latcost(want_grad):
        lib.check(lib.lib.mm_latticecost_f32(bf._h, V.data_ptr(), V.stride(0), V.stride(1), lens.data_ptr(), N, offsets.data_ptr(), arc.data_ptr(), n, None,
                                             cost.data_ptr(), risk.data_ptr(), diff.data_ptr(), post.data_ptr(), logz.data_ptr(),
                                             grad.data_ptr() if want_grad else None, None, grad.stride(0) if want_grad else 0, grad.stride(1) if want_grad else 0, st()))

    latpost()  # (the arc table goes up outside the timed calls)
    few = n > (1 << 30)  # (a tenth of a second and more per call: fewer rounds)
    t = timed_alternating({"latticecost_ms": lambda: latcost(True), "latticecost_no_grad_ms": lambda: latcost(False), "latticeposteriors_ms": latpost},
                          K=3 if few else 8, W=1 if few else 2)
    latcost(True)
    torch.cuda.synchronize()
    row = dict(workload=name, states=g.S, arcs=g.n_arcs, B=B, T=N, beam=bm, records=n, kept_arcs_per_frame=round(n / float(B * N), 2), **spread(t))
    row["latticecost_over_latticeposteriors"] = round(t["latticecost_ms"][0] / t["latticeposteriors_ms"][0], 3)
    row["latticecost_no_grad_over_latticeposteriors"] = round(t["latticecost_no_grad_ms"][0] / t["latticeposteriors_ms"][0], 3)
    row["us_per_step_no_grad"] = round(t["latticecost_no_grad_ms"][0] * 1e3 / (2 * N), 3)  # (a forward and a backward step per frame)
    row["grad_kernel_ms"] = round(t["latticecost_ms"][0] - t["latticecost_no_grad_ms"][0], 3)
    row["records_per_second"] = round(n / (t["latticecost_ms"][0] * 1e-3))
    row["risk_mean"] = round(float(risk.mean()), 4)
    if not few:  # (the identity risk = sum exp(post) cost on the device's own outputs, summed in double)
        owner = torch.repeat_interleave(torch.arange(B, device="cuda"), offsets[N::N] - offsets[:-1:N])
        want = torch.zeros(B, dtype=torch.float64, device="cuda").index_add_(0, owner, (torch.exp(post) * cost).double())
        row["risk_minus_sum_post_cost_max"] = float((risk.double() - want).abs().max())
    row["kernels"] = bf.kernels("latticecost")
    return row


def main():
    from srchash import source_hash
    rows = []
    for i, (which, bm) in enumerate(ROWS):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(i)], capture_output=True, text=True, timeout=LIMIT_S)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            sys.exit(f"row {i} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps(dict(source_hash=source_hash(), rows=rows))
    print(line, flush=True)
    out = [a for a in sys.argv[1:] if not a.startswith("--")]
    if out:
        open(out[0], "w").write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--row":
        print(json.dumps(measure(*ROWS[int(sys.argv[2])])), flush=True)
    else:
        main()
