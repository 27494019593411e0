"""The float32 floor of the expected-cost recursion, on the CPU: tests/cost_reference.py's float32 mode (r and s carried centred in
float32, the offsets in float64) against its float64 mode, on the very inputs of tests/test_gpu_expectedcost.py and tests/test_gpu_itemform.py.  The worst
|grad_f32 - grad_f64| / G_b it prints is cost_reference.GRAD_F32_FLOOR; 10 x that (capped at 1e-4) is the absolute part of the
gradient's bar.  No GPU involved: the kernel is never the source of its own tolerance.

    python tools/measure_cost_floor.py [--json profiles/expectedcost_floor.json]
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
    import cost_reference as cr
    import test_gpu_expectedcost as t

    cases = [("random40", lambda: t.case_random40(wl)), ("config3 T=1500 randn", lambda: t.case_config3(wl, False)),
             ("config3 T=500 log_softmax(10x)", lambda: t.case_config3(wl, True)), ("wsj den T=700", lambda: t.case_wsj(wl, "den_fsm_wsj")),
             ("wsj num T=700", lambda: t.case_wsj(wl, "num_fsm_wsj")), ("four distinct graphs", lambda: t.case_distinct(wl)),
             ("12500 states", lambda: t.case_bigv(wl))]
    import test_gpu_itemform as ti

    # the item-form cases (tests/test_gpu_itemform.py): streamed-only instances, beyond 16-bit state indices, boundaries, wide rows
    cases += [("lfmmi600", lambda: ti.case_lfmmi600(wl)), ("70000 states", lambda: ti.case_random_big(wl)),
              ("70000 + 40 states", lambda: ti.case_mixed(wl, True)), ("40 + 70000 states", lambda: ti.case_mixed(wl, False)),
              ("65530 states", lambda: ti.case_random_big(wl, 65530)), ("65531 states", lambda: ti.case_random_big(wl, 65531)),
              ("5062 states", lambda: ti.case_random_big(wl, ti.PREDICTED_LDS_BOUNDARY["cost"])),
              ("5063 states", lambda: ti.case_random_big(wl, ti.PREDICTED_LDS_BOUNDARY["cost"] + 1)),
              ("wide rows", lambda: ti.case_wide(wl, "wide")), ("ergodic300", lambda: ti.case_wide(wl, "ergodic300")),
              ("lexicon3000", lambda: ti.case_wide(wl, "lexicon"))]
    rows, worst = [], 0.0
    for name, make in cases:
        gs, V, cost, lens, idx = make()
        fs = {id(g): wl.to_fsm(mm, g) for g in gs}
        N = V.shape[1]
        for b in (range(len(gs)) if idx is None else idx):
            L = int(lens[b])
            a = (o, oc, gs[b], fs[id(gs[b])], V[b].astype(np.float64), cost[b].astype(np.float64), L, N)
            r64 = cr.reference(*a)
            if not np.isfinite(r64[3]):
                continue
            r32 = cr.reference(*a, dtype=np.float32)
            G = float(np.abs(r64[1]).max())
            ge_ = float(np.abs(r32[1] - r64[1]).max() / G) if G > 0 else 0.0
            c = np.abs(cost[b, :L].astype(np.float64))
            bar = 1e-4 * float(np.sum(r64[2][:L] * c)) + 1e-6 * L * float(c.max())
            rows.append({"case": name, "utterance": int(b), "len": L, "risk": r64[0], "G": G, "grad_err_over_G": ge_,
                         "risk_err": abs(r32[0] - r64[0]), "risk_bar": bar})
            worst = max(worst, ge_)
            print(f"{name:32s} b={b} len={L:5d} risk={r64[0]:12.5f} G={G:9.4g} |grad32-grad64|/G={ge_:.3g} |risk32-risk64|={abs(r32[0] - r64[0]):.3g} (bar {bar:.3g})", flush=True)
    print(f"worst |grad_f32 - grad_f64| / G_b = {worst:.3g}  ->  a = min(10 x, 1e-4) = {min(10 * worst, 1e-4):.3g}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"worst_grad_err_over_G": worst, "a": min(10 * worst, 1e-4), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
