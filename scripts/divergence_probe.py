#!/usr/bin/env python
"""scripts/divergence_probe.py -- accuracy of the device's float64 log and the cost of the divergence tile kernel.

Writes two files into --out (default: profiles/):

divergence_bounds.txt   the largest error of the device's log, in units in the last place of the correctly rounded result,
                        against numpy's longdouble log over the arguments the kernel meets: ratios in (0, 2] (dense near
                        1, where the result is small) and log-uniform arguments in (0, 1e300].  tests/divergence_ref.py
                        uses the figure with a factor 2 for the arguments not sampled.
divergence_probe.txt    js_metric pdist at n = m = 1,024 / 4,096 / 16,384, a full MVCA.from_msm at the same sizes, and a
                        log-only loop whose rate gives the floor of the pdist: the same number of logs and nothing else.

Usage:  python scripts/divergence_probe.py [--out DIR] [--sizes 1024,4096,16384]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_log(x, reps=1):
    from msmbuilder_amd import _lib
    _lib.ensure_device()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    ms = C.c_float(0)
    _lib.check(_lib.lib().msm_divergence_log_probe(x.ctypes.data, len(x), int(reps), out.ctypes.data, C.byref(ms)))
    return out, ms.value


def ulp_error(got, x):
    """|got - log(x)| in units of the spacing of float64 at the correctly rounded result."""
    want = np.log(x.astype(np.longdouble))
    w64 = want.astype(np.float64)
    spacing = np.spacing(np.abs(w64))
    ok = w64 != 0
    err = np.zeros(len(x), dtype=np.longdouble)
    err[ok] = np.abs(got[ok].astype(np.longdouble) - want[ok]) / spacing[ok]
    zero_ok = np.all(got[~ok] == 0)
    return err, zero_ok


def accuracy(lines):
    rs = np.random.RandomState(0)
    n = 1 << 21
    sets = {
        "ratio (0, 2] uniform": rs.rand(n) * 2.0 + 2.0 ** -60,
        "ratio 1 +- 2^-k, k in [1, 52]": np.concatenate([1.0 + s * 2.0 ** -rs.uniform(1, 52, n // 2) for s in (1.0, -1.0)]),
        "ratio 2^-k (1 + x), k in [0, 1074]": np.ldexp(1.0 + rs.rand(n), -rs.randint(0, 1075, n)),
        "log-uniform (1e-300, 1e300]": 10.0 ** rs.uniform(-300, 300, n),
        "subnormal arguments": np.ldexp(rs.rand(n), -1022) + 5e-324,
    }
    worst = 0.0
    for name, x in sets.items():
        got, _ = device_log(x)
        err, zero_ok = ulp_error(got, x)
        k = int(np.argmax(err))
        worst = max(worst, float(err.max()))
        lines.append("%-36s n = %d   max error %.4f ulp at x = %r   log(1) == 0: %s" % (name, len(x), float(err.max()), float(x[k]), zero_ok))
    one, _ = device_log(np.array([1.0]))
    lines.append("log(1.0) = %r" % float(one[0]))
    lines.append("LOG_ULP_MEASURED = %.4f" % worst)
    return worst


def timed(fn, repeat=3):
    import torch
    fn()
    torch.cuda.synchronize()
    best = np.inf
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sizes", default="1024,4096,16384")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)

    lines = ["device float64 log against numpy longdouble (scripts/divergence_probe.py)"]
    accuracy(lines)
    with open(os.path.join(args.out, "divergence_bounds.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)

    import torch
    import divergence_ref as R
    from msmbuilder_amd import MVCA, MarkovStateModel
    from msmbuilder_amd.utils import divergence as D

    out = ["divergence tile kernel and MVCA (scripts/divergence_probe.py); times are the best of 3, seconds"]
    # the floor: logs per second of a loop that does nothing else
    x = np.random.RandomState(1).rand(1 << 22) + 0.5
    reps = 512
    device_log(x, reps)
    ms = min(device_log(x, reps)[1] for _ in range(3))
    rate = len(x) * reps / (ms * 1e-3)
    out.append("log-only loop: %d elements x %d logs in %.3f ms -> %.4g logs/s" % (len(x), reps, ms, rate))
    path = os.path.join(args.out, "divergence_probe.txt")
    for n in [int(s) for s in args.sizes.split(",")]:
        T = R.gen(n, max(n // 64, 2), n)
        Td = torch.as_tensor(T, device="cuda")
        t_pd = timed(lambda: D.divergence_pdist(Td, "js_metric"))
        logs = n * (n - 1) // 2 * n * 2           # two logs per pair element where no entry is zero
        nz = T != 0
        both = (nz.astype(np.float32) @ nz.T.astype(np.float32))   # columns where both rows are nonzero: two logs; one nonzero: one
        one = nz.sum(1)[:, None] + nz.sum(1)[None, :] - 2 * both
        iu = np.triu_indices(n, 1)
        logs_done = float((2 * both + one)[iu].sum())
        floor_all, floor_done = logs / rate, logs_done / rate
        out.append("n = m = %6d  js_metric pdist %.4f s   floor at 2 logs per pair element %.4f s (x %.2f)   floor at the %.4g "
                   "logs of non-skipped terms %.4f s (x %.2f)" % (n, t_pd, floor_all, t_pd / floor_all, logs_done, floor_done, t_pd / floor_done))
        msm = MarkovStateModel(verbose=False)
        msm.transmat_, msm.populations_, msm.mapping_ = T, np.full(n, 1.0 / n), dict(zip(range(n), range(n)))
        msm.countsmat_, msm.n_states_ = T, n
        t_mv = timed(lambda: MVCA.from_msm(msm, n_macrostates=max(n // 64, 2)), repeat=1 if n > 4096 else 3)
        t_ln = timed(lambda: MVCA.from_msm(msm, n_macrostates=max(n // 64, 2), n_landmarks=n // 8), repeat=1 if n > 4096 else 3)
        out.append("n = m = %6d  MVCA.from_msm %.4f s   with n_landmarks = n / 8 %.4f s" % (n, t_mv, t_ln))
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")
        print(out[-2], out[-1], sep="\n", flush=True)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
