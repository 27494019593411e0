"""The float32 floor of the expected class-cost recursion, on the CPU: tests/classcost_reference.py's float32 mode (r', t', the class
term and every sum over them in float32, the offsets in float64) against its float64 mode, on the very inputs of
tests/test_gpu_classcost.py (its case functions, with D given and with D NULL) and on the classcost inputs of
tests/test_gpu_class_entries.py (classcost_cases: class counts at the block size, the 70 000-state graph, wide rows, P at the block size).  The worst |grad_f32 - grad_f64| / G_b it prints is
classcost_reference.GRAD_F32_FLOOR; 10 x that (capped at 1e-4) is the absolute part of the gradient's bar.  No GPU involved: the
kernel is never the source of its own tolerance.

    python tools/measure_classcost_floor.py [--json profiles/classcost_floor.json] [--cap C]

The class count of the class-cap case is BatchedFSM.info(classcost=True)["cost_class_cap"] of that test's batch.  A batch needs a
device: with one the tool asks it; without one it takes --cap, else the count the committed table was measured at
(profiles/classcost_floor.json).  tests/test_gpu_classcost.py::test_class_cap compares the table's count with the device's, so a
changed LDS plan of the cost kernels shows there and not as a stale number here.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def cap_of_the_cap_case(mm, wl, given):
    if given:
        return given
    try:
        import torch

        if torch.cuda.is_available():
            g = wl.random_fsm(20, 4, 3.0, seed=1)
            cf = mm.compile(wl.to_fsm(mm, g), mm.statemap(g.state2pdf, g.P))
            return int(mm.batch(cf, cf).info(classcost=True)["cost_class_cap"])
    except ImportError:
        pass
    with open(os.path.join(ROOT, "profiles", "classcost_floor.json")) as fh:
        return int(json.load(fh)["cap"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--cap", type=int, default=0)
    args = ap.parse_args()
    import __graft_entry__ as ge
    import importlib

    mm = ge.load_package()
    wl = importlib.import_module(mm.__name__ + ".workloads")
    import classcost_reference as ccr
    import test_gpu_class_entries as tce
    import test_gpu_classcost as t

    rows, worst = [], 0.0
    cap = cap_of_the_cap_case(mm, wl, args.cap)
    for name, _, _, _, gs, clss, nc, V, lens in t.all_cases(mm, wl, cap) + tce.classcost_cases(mm, wl):
        fs = {id(g): wl.to_fsm(mm, g) for g in gs}
        N = V.shape[1]
        A, D = t._costs(40, len(gs), N, nc, V.shape[2])
        for with_d in (True, False):
            case_worst = 0.0
            for b in range(len(gs)):
                L = int(lens[b])
                a = (gs[b], fs[id(gs[b])], clss[b], V[b].astype(np.float64), A[b].astype(np.float64), D[b].astype(np.float64) if with_d else None, L, N)
                r64 = ccr.reference(*a)
                if not np.isfinite(r64[3]):
                    continue
                r32 = ccr.reference(*a, dtype=np.float32)
                G = float(np.abs(r64[1]).max())
                ge_ = float(np.abs(r32[1] - r64[1]).max() / G) if G > 0 else 0.0
                bar = 1e-4 * r64[4] + 1e-6 * L * max(float(np.abs(A[b, :L]).max()) if L else 0.0, float(np.abs(D[b, :L]).max()) if (with_d and L) else 0.0)
                rows.append({"case": name, "D": with_d, "utterance": int(b), "len": L, "risk": r64[0], "G": G, "grad_err_over_G": ge_,
                             "risk_err": abs(r32[0] - r64[0]), "risk_bar": bar})
                case_worst = max(case_worst, ge_)
                print(f"{name:24s} D={'given' if with_d else 'NULL ':5s} b={b} len={L:4d} risk={r64[0]:11.5f} G={G:9.4g} |grad32-grad64|/G={ge_:.3g} "
                      f"|risk32-risk64|={abs(r32[0] - r64[0]):.3g} (bar {bar:.3g})", flush=True)
            worst = max(worst, case_worst)
    print(f"worst |grad_f32 - grad_f64| / G_b = {worst:.3g}  ->  a = min(10 x, 1e-4) = {min(10 * worst, 1e-4):.3g}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"worst_grad_err_over_G": worst, "a": min(10 * worst, 1e-4), "cap": cap, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
