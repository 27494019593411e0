"""The float32 floor of the forward filter at shifted emission levels, on the CPU: tests/filter_reference.py's float32 mode on the
inputs of tests/test_gpu_filterposteriors.py's config-3 cases -- V and the copies V + 100, V - 150 as the test rounds them to
float32 -- against the float64 reference of the UNSHIFTED V, which is what the test compares the kernel with.  Prints, per case, the
worst error over each of the project's bars (filt: absolute / 2e-5 and log-relative / 1e-4; incr and ttl; state_out).  A figure
above 1 is a bar float32 arithmetic alone cannot meet.  No GPU involved: the kernel is never the source of its own tolerance.

    python tools/measure_filter_floor.py [--json profiles/filterposteriors_floor.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import importlib

    import __graft_entry__ as ge
    from srchash import source_hash

    mm = ge.load_package()
    wl = importlib.import_module(mm.__name__ + ".workloads")
    import filter_reference as fr
    import test_gpu_filterposteriors as t

    rows = []
    for sharp in (False, True):
        gs, V, lens = t.case_config3(wl, sharp)
        N = V.shape[1]
        for b in range(len(gs)):
            L = int(lens[b])
            f64, i64, z64, s64 = fr.reference(gs[b], V[b].astype(np.float64), L, N)
            m = f64 > 1e-30
            ms = s64 > np.log(1e-30)
            for shift in (0.0,) + t.SHIFTS:
                Vs = t.shifted(V[b], shift) if shift else V[b]
                f32, i32, z32, s32 = fr.reference(gs[b], Vs.astype(np.float64), L, N, dtype=np.float32)
                with np.errstate(divide="ignore"):
                    lrel = np.abs(np.log(f32[m]) - np.log(f64[m])) / (1e-4 * np.maximum(np.abs(np.log(f64[m])), 1.0))
                ie = np.abs(i32[:L] - (i64[:L] + shift)) / (1e-4 + 1e-5 * np.abs(i64[:L] + shift))
                row = {"case": "config 3, " + ("log_softmax(10 randn)" if sharp else "randn"), "utterance": b, "len": L, "shift": shift,
                       "filt_abs_err": float(np.abs(f32 - f64).max()), "filt_abs_over_bar": float(np.abs(f32 - f64).max() / 2e-5),
                       "filt_log_over_bar": float(lrel.max()), "incr_over_bar": float(ie.max()),
                       "ttl_over_bar": float(abs(z32 - (z64 + shift * L)) / (1e-4 + 1e-5 * abs(z64 + shift * L))),
                       "state_over_bar": float((np.abs(s32[ms] - s64[ms]) / (1e-4 * np.maximum(np.abs(s64[ms]), 1.0))).max())}
                rows.append(row)
                print(" ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    keys = ("filt_abs_err", "filt_abs_over_bar", "filt_log_over_bar", "incr_over_bar", "ttl_over_bar", "state_over_bar")
    worst = {k: max(r[k] for r in rows) for k in keys}
    print("worst:", worst)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"source_hash": source_hash(), "worst": worst, "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
