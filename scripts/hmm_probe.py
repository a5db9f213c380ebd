#!/usr/bin/env python
"""scripts/hmm_probe.py -- what the Gaussian HMM E-step costs on one MI355X; writes profiles/hmm_probe.txt.

    python scripts/hmm_probe.py            # the timings (needs the GPU); --quick: fewer runs, no whole fit of the largest shape
    python scripts/hmm_probe.py --bounds   # profiles/hmm_bounds.txt: the rounding bound at the test shapes (no GPU)

Three shapes with the rows resident in device memory: 28 x 10,000 x 10 at K = 6, 1 x 1,000,000 x 4 at K = 4 and
2,000 x 5,000 x 20 at K = 20.  Per shape: the E-step (wall clock around a call that ends in a stream synchronise: parameter
upload, four launches, results back), frames per second, the call against the floor of reading X twice at the measured
device-memory rate, the same E-step with the longest segment the plan allows, the forward half (score) at the default
segment and with the segment set to the trajectory length -- the serial-in-time form, which only the forward half can take:
the E-step's fused pass keeps alpha for a whole segment in LDS and refuses a longer one --, Viterbi, and a whole default fit.
Per figure: one warm-up call, then the median of the timed calls.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_bounds(path):
    import hmm_ref as R
    import test_hmm_ref as TR
    lines = ["Rounding bound of the HMM E-step at the test shapes (tests/hmm_ref.py: bound), written by scripts/hmm_probe.py --bounds",
             "rel: relative to each sum's scale (post: N, trans: N - n_traj, obs: sum |x|, obs**2: sum x^2); must stay below "
             "sqrt(2^-53) = %.3e" % R.SQRT_U,
             "%-26s %6s %6s %4s %4s %10s %10s %10s %10s %12s" % ("case", "N", "T_max", "K", "F", "E", "rho", "logspace", "rel", "max logprob")]
    for name, seqs, mdl in TR.CASES:
        lines.append(R.bounds_line(name, R.bound(seqs, *mdl)))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def timed(fn, runs):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def hbm_rate():
    """Bytes per second of a device-to-device copy of 1 GiB (read + write counted)."""
    import torch
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    med, _, _ = timed(lambda: b.copy_(a), 5)
    return 2 * a.numel() * 4 / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    if args.bounds:
        write_bounds(os.path.join(ROOT, "profiles", "hmm_bounds.txt"))
        return
    import torch
    import hmm_ref as R
    from msmbuilder_amd import _lib
    from msmbuilder_amd.hmm import GaussianHMM, gaussian as G
    _lib.ensure_device(0)
    runs = 3 if args.quick else 6
    rate = hbm_rate()
    out = ["Gaussian HMM E-step on one MI355X (msm_hmm_estep_f32; DESIGN), written by scripts/hmm_probe.py on %s" % time.strftime("%Y-%m-%d"),
           "every time is the wall clock around a CALL that ends in a stream synchronise (parameter upload, launches, results "
           "back), not a kernel time; no counters were taken.  One warm-up call, then the median of %d timed calls." % runs,
           "device-memory rate (1 GiB device-to-device copy, read + write): %.2f TB/s" % (rate / 1e12)]
    for n_traj, T, F, K in ((28, 10000, 10, 6), (1, 1000000, 4, 4), (2000, 5000, 20, 20)):
        mdl = R.model(K, F, 3, spread=2.0)
        rs = np.random.RandomState(5)
        hidden = rs.randint(K, size=(n_traj * T // 50 + 1)).repeat(50)[:n_traj * T]
        X = torch.as_tensor((mdl[0][hidden] + rs.randn(n_traj * T, F) * np.sqrt(mdl[1][hidden])).astype(np.float32), device="cuda")
        rows = G._Rows(X, [T] * n_traj)
        p = G.plan(K)
        N = n_traj * T
        floor = 2 * N * F * 4 / rate
        out.append("--- %d x %d x %d float32 at K = %d (N = %d); plan %s" % (n_traj, T, F, K, N, p))
        med, lo, hi = timed(lambda: G.estep(rows, *mdl), runs)
        out.append("E-step, segment %d (default): median %.2f ms (min %.2f, max %.2f) -> %.3e frames/s; floor of reading X twice "
                   "%.3f ms: %.1f x the floor" % (p['segment'], med * 1e3, lo * 1e3, hi * 1e3, N / med, floor * 1e3, med / floor))
        med2, lo2, hi2 = timed(lambda: G.estep(rows, *mdl, segment=p['segment_max']), runs)
        out.append("E-step, segment %d (the longest the plan allows): median %.2f ms (min %.2f, max %.2f)"
                   % (p['segment_max'], med2 * 1e3, lo2 * 1e3, hi2 * 1e3))
        med3, lo3, hi3 = timed(lambda: G.score(rows, *mdl), runs)
        out.append("score (operators + stitch): median %.2f ms (min %.2f, max %.2f)" % (med3 * 1e3, lo3 * 1e3, hi3 * 1e3))
        med5, lo5, hi5 = timed(lambda: G.score(rows, *mdl, segment=T), max(2, runs // 2))
        out.append("score, segment %d = the trajectory length (the forward half serial in time, one workgroup per trajectory): "
                   "median %.2f ms (min %.2f, max %.2f) = %.1f x the time-parallel forward half"
                   % (T, med5 * 1e3, lo5 * 1e3, hi5 * 1e3, med5 / med3))
        med4, lo4, hi4 = timed(lambda: G.viterbi(rows, *mdl), max(2, runs // 2))
        out.append("Viterbi (one wave per trajectory, sequential in time; states back to the host): median %.2f ms (min %.2f, max %.2f)"
                   " -> %.3e frames/s" % (med4 * 1e3, lo4 * 1e3, hi4 * 1e3, N / med4))
        if not (args.quick and N > 2000000):
            seqs = list(X.view(n_traj, T, F).unbind(0))
            t0 = time.perf_counter()
            est = GaussianHMM(n_states=K, random_state=0).fit(seqs)
            out.append("GaussianHMM.fit, defaults (n_init = 10 x n_iter = 10): %.2f s; last log probability %.6e"
                       % (time.perf_counter() - t0, est.fit_logprob_[-1]))
        del X, rows
    text = "\n".join(out) + "\n"
    with open(os.path.join(ROOT, "profiles", "hmm_probe.txt"), "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
