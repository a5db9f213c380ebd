#!/usr/bin/env python
"""scripts/timeseries_probe.py -- what the time-series smoothers cost on one MI355X; writes profiles/timeseries_probe.txt.

    python scripts/timeseries_probe.py            # needs the GPU
    python scripts/timeseries_probe.py --bounds   # profiles/timeseries_bounds.txt: the tolerances at the test inputs (no GPU)
    python scripts/timeseries_probe.py --out DIR  # write the probe's file into DIR instead of profiles/

float32 rows resident in HBM, three shapes (trajectories x frames x features): 28 x 10,000 x 512 (the bench's width),
1 x 1,000,000 x 4 (one long narrow trajectory: only the time axis has any parallelism) and 2,000 x 5,000 x 20 (many short
ones).  Per estimator: the median time of ``transform`` over the list (a host clock around a call that ends in a device
synchronise, after a warm-up call), its ratio to the floor of reading X once and writing Y once at 8.0 TB/s (the HBM3E
specification), and the time with one segment per trajectory (MSM_TS_SEGMENT=0), the recurrence serial in time.
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(28, 10000, 512), (1, 1000000, 4), (2000, 5000, 20)]
HBM_PEAK = 8.0e12   # bytes / s, specification
REPEATS = 5


def timed(est, seqs, segment):
    import torch
    if segment is None:
        os.environ.pop("MSM_TS_SEGMENT", None)
    else:
        os.environ["MSM_TS_SEGMENT"] = str(segment)
    out = est.transform(seqs)   # warm-up: code objects, the library's scratch, torch's allocator
    del out
    ts = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = est.transform(seqs)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    os.environ.pop("MSM_TS_SEGMENT", None)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.bounds:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_timeseries_ref
        test_timeseries_ref.write_profile(os.path.join(args.out, "timeseries_bounds.txt"))
        return
    import torch
    from msmbuilder_amd import _lib
    from msmbuilder_amd import timeseries as TS
    _lib.ensure_device(0)
    lines = ["Time-series smoothers on one MI355X, float32 rows resident in HBM; written by scripts/timeseries_probe.py on %s."
             % datetime.date.today().isoformat(),
             "ms: median of %d transform() calls over the whole list (min .. max), host clock around a synchronised call."
             % REPEATS,
             "floor: X read once + Y written once (float32 out for Butterworth, float64 out for the EWMAs) at %.1f TB/s."
             % (HBM_PEAK / 1e12),
             "S: the segment the rule chose (frames of a pass; 0: one segment per trajectory); one-seg: MSM_TS_SEGMENT=0.",
             "%-22s %-34s %6s %9s %20s %9s %8s %10s" % ("shape", "estimator", "S", "ms", "(min .. max)", "floor ms", "x floor",
                                                      "one-seg ms")]
    ests = [("Butterworth(width=5, order=3)", TS.Butterworth(width=5, order=3), 4),
            ("Butterworth(width=101, order=3)", TS.Butterworth(width=101, order=3), 4),
            ("EWMA(span=20)", TS.EWMA(span=20), 8),
            ("DoubleEWMA(span=20)", TS.DoubleEWMA(span=20), 8)]
    for n_traj, n, F in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn((n_traj * n, F), generator=g, device="cuda", dtype=torch.float32).cumsum(0).mul_(0.01).add_(100.0)
        seqs = list(X.view(n_traj, n, F).unbind(0))
        for name, est, out_bytes in ests:
            floor_ms = n_traj * n * F * (4 + out_bytes) / HBM_PEAK * 1e3
            if isinstance(est, TS.Butterworth):
                S = TS._segment_for(est._denom, n + 2 * (est.width - 1) + 6 * (est.order + 1))
            else:
                S = TS._segment_for([1.0, -(1.0 - est._alpha())], n)
            med, lo, hi = timed(est, seqs, None)
            one = timed(est, seqs, 0)[0]
            lines.append("%-22s %-34s %6d %9.3f %20s %9.4f %8.1f %10.3f" % ("%d x %d x %d" % (n_traj, n, F), name, S, med,
                                                                         "(%.3f .. %.3f)" % (lo, hi), floor_ms, med / floor_ms, one))
            print(lines[-1], flush=True)
        del X, seqs
        torch.cuda.empty_cache()
    with open(os.path.join(args.out, "timeseries_probe.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
