"""The float32 floor of the path-entropy recursion, on the CPU: tests/entropy_reference.py's float32 mode (Hf and Hb carried centred
in float32, the offsets in float64) against its float64 mode, on the very inputs of tests/test_gpu_pathentropy.py.  The worst
|H_f32 - H_f64| / len and |grad_f32 - grad_f64| / G_b it prints are entropy_reference.H_F32_FLOOR and GRAD_F32_FLOOR; 10 x them
(the gradient's capped at 1e-4) are the absolute parts of the bars.  No GPU involved: the kernel is never the source of its own
tolerance.

    python tools/measure_entropy_floor.py [--json profiles/pathentropy_floor.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    import importlib

    mm = ge.load_package()
    o, oc = ge.load_oracle()
    wl = importlib.import_module(mm.__name__ + ".workloads")
    import entropy_reference as er
    import test_gpu_pathentropy as t

    cases = [("random40", lambda: t.case_random40(wl)), ("four distinct graphs", lambda: t.case_distinct(wl)),
             ("config3 T=1500 randn", lambda: t.case_config3(wl, False)), ("config3 T=500 log_softmax(10x)", lambda: t.case_config3(wl, True)),
             ("wsj den T=700", lambda: t.case_wsj(wl, "den_fsm_wsj")), ("wsj num T=700", lambda: t.case_wsj(wl, "num_fsm_wsj")),
             ("12500 states", lambda: t.case_bigv(wl))]
    rows, worst_h, worst_g = [], 0.0, 0.0
    for name, make in cases:
        gs, V, lens, idx = make()
        fs = {id(g): wl.to_fsm(mm, g) for g in gs}
        N = V.shape[1]
        for b in (range(len(gs)) if idx is None else idx):
            L = int(lens[b])
            a = (o, oc, gs[b], fs[id(gs[b])], V[b].astype(np.float64), L, N)
            r64 = er.reference(*a)
            if not np.isfinite(r64[3]):
                continue
            er.assert_inputs_test_something(r64, L)
            r32 = er.reference(*a, dtype=np.float32)
            G = float(np.abs(r64[1]).max())
            ge_ = float(np.abs(r32[1] - r64[1]).max() / G) if G > 0 else 0.0
            he = abs(r32[0] - r64[0]) / L
            rows.append({"case": name, "utterance": int(b), "len": L, "H": r64[0], "G": G, "H_err_per_frame": he, "grad_err_over_G": ge_})
            worst_h, worst_g = max(worst_h, he), max(worst_g, ge_)
            print(f"{name:32s} b={b} len={L:5d} H={r64[0]:11.5f} G={G:9.4g} |H32-H64|/len={he:.3g} |grad32-grad64|/G={ge_:.3g}", flush=True)
    print(f"worst |H_f32 - H_f64| / len = {worst_h:.3g}  ->  h = 10 x = {10 * worst_h:.3g} nats per frame")
    print(f"worst |grad_f32 - grad_f64| / G_b = {worst_g:.3g}  ->  a = min(10 x, 1e-4) = {min(10 * worst_g, 1e-4):.3g}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"worst_H_err_per_frame": worst_h, "h": 10 * worst_h, "worst_grad_err_over_G": worst_g, "a": min(10 * worst_g, 1e-4),
                       "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
