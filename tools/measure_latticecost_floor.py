"""The float32 floor of the lattice expected-cost recursion, on the CPU: tests/latcost_reference.py's float32 mode (ca and cb carried
centred in float32, the offsets in float64, diff against the cell's own posterior mean) against its float64 mode, on the inputs of
tests/test_gpu_latticecost.py as tests/test_latticecost.floor_cases builds them (the lattices by tests/lattice_reference.py).  The
worst |x_f32 - x_f64| / G_b over diff and grad it prints is latcost_reference.F32_FLOOR; 10 x that (capped at 1e-4) is the absolute
part of the bars of diff and grad.  The shift case is judged as the device is: costs + 64 in float32 against the float64 reference
of the unshifted costs.  No GPU involved: the kernel is never the source of its own tolerance.

    python tools/measure_latticecost_floor.py [--json profiles/latticecost_floor.json]
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
    wl = importlib.import_module(mm.__name__ + ".workloads")
    import latcost_reference as lc
    import test_latticecost as t

    rows, worst, unshifted = [], 0.0, None
    for what, fs, gs, V, lens, offsets, arc, extra, cost in t.floor_cases(mm, wl):
        B, N = V.shape[0], V.shape[1]
        shifted = "+ 64" in what
        r64 = unshifted if shifted else lc.reference(fs, gs, V, lens, offsets, arc, cost, extra)
        if what.startswith("shift") and not shifted:
            unshifted = r64
        r32 = lc.reference(fs, gs, V, lens, offsets, arc, cost, extra, dtype=np.float32)
        L = np.full(B, N) if lens is None else np.clip(np.asarray(lens), 0, N)
        want_risk = r64.risk + (t.SHIFT * L * np.isfinite(r64.logz) if shifted else 0.0)
        own = lc.owners(offsets, arc.size, B, N)
        p = np.where(np.isfinite(r64.post), np.exp(np.where(np.isfinite(r64.post), r64.post, 0.0)), 0.0)
        ac = np.abs(cost.astype(np.float64))
        risk_err, risk_bar = 0.0, np.inf
        for b in range(B):
            live = (own == b) & (p > 0)
            bar = 1e-4 * float((p[live] * ac[live]).sum()) + 1e-6 * int(L[b]) * (float(ac[live].max()) if live.any() else 0.0)
            e = abs(float(r32.risk[b] - want_risk[b]))
            if np.isfinite(r64.logz[b]) and e - bar >= risk_err - risk_bar:
                risk_err, risk_bar = e, bar
        rd, rg = t.floor_ratio_diff(r64, r32, offsets), t.floor_ratio(r64, r32, offsets)
        risk_bar = risk_bar if np.isfinite(risk_bar) else 0.0
        rows.append({"case": what, "records": int(arc.size), "diff_err_over_G": rd, "grad_err_over_G": rg, "risk_err": risk_err, "risk_bar": risk_bar})
        worst = max(worst, rd, rg)
        print(f"{what:56s} records={arc.size:6d} |diff32-diff64|/G={rd:.3g} |grad32-grad64|/G={rg:.3g} |risk32-risk64|={risk_err:.3g} (bar {risk_bar:.3g})", flush=True)
    print(f"worst |x_f32 - x_f64| / G_b = {worst:.3g}  ->  a = min(10 x, 1e-4) = {min(10 * worst, 1e-4):.3g}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"worst_err_over_G": worst, "a": min(10 * worst, 1e-4), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
