#!/usr/bin/env python
"""scripts/vmhmm_probe.py -- what the von Mises HMM costs on one MI355X; writes profiles/vmhmm_probe.txt.

    python scripts/vmhmm_probe.py            # the timings (needs the GPU); --quick: fewer runs, no whole fit of the largest shape
    python scripts/vmhmm_probe.py --bounds   # profiles/vmhmm_bounds.txt: tau measured on the device (needs the GPU) and
                                             # the rounding bound at the test shapes

The three shapes of scripts/hmm_probe.py with float32 angles resident in device memory: 28 x 10,000 x 10 at K = 6,
1 x 1,000,000 x 4 at K = 4 and 2,000 x 5,000 x 20 at K = 20.  Per shape: (a) the image kernel (msm_hmm_trig_f32) against
its floor of reading N F itemsize and writing 16 N F bytes at the measured device-memory rate; (b) one linear E-step over
the image against one GAUSSIAN E-step on D = 2 F float64 columns at the same K (the image itself handed to
msm_hmm_estep_f64: the same operator, stitch and reduce passes, a longer emission and contraction); (c) a default fit.
Every time is the wall clock around a call that ends in a stream synchronise; one warm-up call, then the median of the
timed calls.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from hmm_probe import timed, hbm_rate  # noqa: E402


def measure_tau():
    """The largest error of the device's image over the arguments of the image test, in units of u."""
    import torch
    import vmhmm_ref as V
    from msmbuilder_amd.hmm import gaussian as G, vonmises as VM
    worst = 0.0
    for dn in ('f32', 'f64'):
        for n in V.IMAGE_N:
            for F in V.IMAGE_F:
                X = V.image_arguments(n, F, dn)
                Z = VM.trig(G._Rows(torch.as_tensor(X, device="cuda"), [n])).X.cpu().numpy()
                worst = max(worst, V.image_error(Z, X))
    return worst


def write_bounds(path):
    import vmhmm_ref as V
    from msmbuilder_amd.hmm import gaussian as G
    text = V.bounds_text(G.plan, measure_tau())
    with open(path, "w") as fh:
        fh.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounds", action="store_true")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    import torch
    from msmbuilder_amd import _lib
    _lib.ensure_device(0)
    if args.bounds:
        write_bounds(os.path.join(ROOT, "profiles", "vmhmm_bounds.txt"))
        return
    import vmhmm_ref as V
    from msmbuilder_amd.hmm import VonMisesHMM, gaussian as G, vonmises as VM
    runs = 3 if args.quick else 6
    rate = hbm_rate()
    out = ["von Mises HMM on one MI355X (msm_hmm_trig_f32, msm_hmm_lin_estep; DESIGN), written by scripts/vmhmm_probe.py on %s"
           % time.strftime("%Y-%m-%d"),
           "every time is the wall clock around a CALL that ends in a stream synchronise, not a kernel time; no counters were "
           "taken.  One warm-up call, then the median of %d timed calls." % runs,
           "device-memory rate (1 GiB device-to-device copy, read + write): %.2f TB/s" % (rate / 1e12)]
    for n_traj, T, F, K in ((28, 10000, 10, 6), (1, 1000000, 4, 4), (2000, 5000, 20, 20)):
        mdl = V.model(K, F, 3, kappa=(2.0, 10.0))
        rs = np.random.RandomState(5)
        N = n_traj * T
        hidden = rs.randint(K, size=(N // 50 + 1)).repeat(50)[:N]
        X = torch.as_tensor(V.wrap(rs.vonmises(mdl[0][hidden], mdl[1][hidden])).astype(np.float32), device="cuda")
        rows = G._Rows(X, [T] * n_traj)
        p = G.plan(K)
        out.append("--- %d x %d x %d float32 angles at K = %d (N = %d, D = %d); plan %s" % (n_traj, T, F, K, N, 2 * F, p))
        floor = (N * F * 4 + 16 * N * F) / rate   # (the rate counts every byte a copy reads and every byte it writes)
        med, lo, hi = timed(lambda: VM.trig(rows), runs)
        out.append("(a) image (msm_hmm_trig_f32, output allocated in the call): median %.3f ms (min %.3f, max %.3f); floor of "
                   "reading %d and writing %d bytes %.3f ms: %.1f x the floor"
                   % (med * 1e3, lo * 1e3, hi * 1e3, N * F * 4, 16 * N * F, floor * 1e3, med / floor))
        img = VM.trig(rows)
        lin = VM.linear_form(mdl[0], mdl[1]) + (mdl[2], mdl[3])
        med1, lo1, hi1 = timed(lambda: VM.lin_estep(img, *lin), runs)
        out.append("(b) linear E-step over the image, segment %d: median %.2f ms (min %.2f, max %.2f) -> %.3e frames/s"
                   % (p['segment'], med1 * 1e3, lo1 * 1e3, hi1 * 1e3, N / med1))
        gm = (np.hstack([np.cos(mdl[0]), np.sin(mdl[0])]), np.hstack([1.0 / mdl[1]] * 2), mdl[2], mdl[3])
        med2, lo2, hi2 = timed(lambda: G.estep(img, *gm), runs)
        out.append("    Gaussian E-step on the same %d float64 columns (msm_hmm_estep_f64): median %.2f ms (min %.2f, max %.2f); "
                   "linear / Gaussian = %.3f" % (2 * F, med2 * 1e3, lo2 * 1e3, hi2 * 1e3, med1 / med2))
        med3, lo3, hi3 = timed(lambda: VM.lin_score(img, *lin), runs)
        out.append("    linear score (operators + stitch): median %.2f ms (min %.2f, max %.2f)" % (med3 * 1e3, lo3 * 1e3, hi3 * 1e3))
        del img
        if not (args.quick and N > 2000000):
            seqs = list(X.view(n_traj, T, F).unbind(0))
            t0 = time.perf_counter()
            est = VonMisesHMM(n_states=K, random_state=0).fit(seqs)
            out.append("(c) VonMisesHMM.fit, defaults (n_init = 10 x n_iter = 10): %.2f s; %d E-steps recorded by the kept run; "
                       "last log probability %.6e" % (time.perf_counter() - t0, len(est.fit_logprob_), est.fit_logprob_[-1]))
        del X, rows
    text = "\n".join(out) + "\n"
    with open(os.path.join(ROOT, "profiles", "vmhmm_probe.txt"), "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
