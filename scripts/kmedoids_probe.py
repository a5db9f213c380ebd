"""Times the k-medoids loop on the GPU: KMedoids.fit at N = 20,000 (K = 100, euclidean on 10-column float64 rows, one
pass), and one MiniBatchKMedoids step at the defaults (8 centres + 100 rows) on both paths.

    python scripts/kmedoids_probe.py > profiles/kmedoids_probe.txt                      (on the GPU)
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/kmedoids_probe.py trace   (the kernels of ONE fit, a run of its own)
    python scripts/kmedoids_probe.py stats OUT/..._results.db >> profiles/kmedoids_probe.txt   (per-kernel table of that trace)
    python scripts/kmedoids_probe.py cpu                                                (the numpy reference loop at N = 4,000, CPU)

Rows: device-resident hubs-plus-noise generated from a seed.  Times are host clocks around calls that end in a device
synchronisation, best of 3 after a warm-up.  The mini-batch step is a window of a fraction of a millisecond (best of 20):
at that size the figure is mostly launch and synchronisation overhead, which is what the two paths differ in.  The cost kernel must read the whole condensed matrix once per iteration
through both triangles, N^2 * 8 bytes; its per-iteration time comes from the kernel trace (`stats` reads the trace's
SQLite file: total time of km_cost_kernel over its calls), next to those bytes over the HBM rate.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

HBM_BYTES_PER_S = 8.0e12   # MI355X peak HBM3E rate


def rows(n, m, seed):
    rs = np.random.RandomState(seed)
    hubs = rs.randn(100, m) * 3.0
    return np.ascontiguousarray(hubs[rs.randint(0, 100, n)] + rs.randn(n, m))


def best_of(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3, out


def fit_probe(n=20000, K=100, reps=3):
    import torch
    from msmbuilder_amd import libdistance
    from msmbuilder_amd.cluster.kmedoids import _KMedoids, last_stats
    X = torch.as_tensor(rows(n, 10, 0), device="cuda")
    ms, est = best_of(lambda: _KMedoids(n_clusters=K, random_state=0).fit(X), reps)
    st = last_stats()
    pd_ms, _ = best_of(lambda: libdistance.pdist(X, "euclidean"), reps)
    need = float(n) * n * 8
    print("KMedoids.fit %d x 10 float64, K = %d, 1 pass: %.1f ms (%d iterations, %d snapshots, path %s); pdist alone %.1f ms"
          % (n, K, ms, st["iterations"], st["snapshots"], "small" if st["small"] else "general", pd_ms))
    print("  per iteration (fit minus pdist, over the iterations): %.2f ms; the matrix pass must read N^2 * 8 B = %.2f GB = %.2f ms"
          " at %.1f TB/s" % ((ms - pd_ms) / st["iterations"], need / 1e9, need / HBM_BYTES_PER_S * 1e3, HBM_BYTES_PER_S / 1e12))
    print("  inertia %.17g" % est.inertia_)


def step_probe():
    import torch
    from msmbuilder_amd._lib import Arr
    from msmbuilder_amd.cluster.kmedoids import kmedoids_fit, last_stats
    X = torch.as_tensor(rows(100000, 10, 1), device="cuda")
    rs = np.random.RandomState(0)
    idx = rs.randint(0, 100000, 108)
    init = np.concatenate([np.arange(8), rs.randint(0, 8, 100)])
    ax = Arr(X)
    for small in ("1", "0"):
        os.environ["MSM_KMEDOIDS_SMALL"] = small
        ms, out = best_of(lambda: kmedoids_fit(ax, "euclidean", 8, 0, init, X_indices=idx), 20)
        st = last_stats()
        print("MiniBatchKMedoids step (8 + 100 rows of 100,000 x 10 float64, device-resident), MSM_KMEDOIDS_SMALL=%s: %.3f ms "
              "(%d iterations, path %s; best of 20 of a sub-millisecond window: mostly launch and synchronisation overhead)"
              % (small, ms, st["iterations"], "small" if st["small"] else "general"))
    del os.environ["MSM_KMEDOIDS_SMALL"]


def cpu_probe(n=4000, K=100):
    import kmedoids_ref as R
    X = rows(n, 10, 0)
    D = R._oracle().pdist(X, "euclidean")
    init = R.random_assignments(np.random.RandomState(0), n, K, 1)
    t = time.perf_counter()
    ids, err, found, info = R.kmedoids(K, D, 1, None, init)
    dt = time.perf_counter() - t
    print("numpy reference loop (tests/kmedoids_ref.py, one CPU thread) %d x 10, K = %d: %.2f s, %d iterations = %.1f ms per "
          "iteration" % (n, K, dt, info["iterations"], dt / info["iterations"] * 1e3))


def trace_stats(db_path, n=20000):
    """Per-kernel table of a `rocprofv3 --kernel-trace` run of the `trace` mode, from its SQLite output."""
    import sqlite3
    cur = sqlite3.connect(db_path).cursor()
    rows = list(cur.execute("select name, count(*), sum(duration), min(duration), max(duration) from kernels "
                            "where name like '%km_%' or name like '%pdist%' group by name order by sum(duration) desc"))
    print("\nKernels of one fit under rocprofv3 --kernel-trace (a run of its own; its calls include the warm-up fit):")
    for name, calls, total, lo, hi in rows:
        print("  %-58s calls %3d  total %9.1f us  min %8.1f  max %8.1f us" % (name[:58], calls, total / 1e3, lo / 1e3, hi / 1e3))
    for name, calls, total, lo, hi in rows:
        if "km_cost_kernel" in name:
            sec = total / calls / 1e9
            need = float(n) * n * 8
            print("  km_cost_kernel: %.2f ms per iteration for N^2 * 8 B = %.2f GB -> %.2f TB/s = %.0f %% of the %.1f TB/s HBM peak"
                  % (sec * 1e3, need / 1e9, need / sec / 1e12, need / sec / HBM_BYTES_PER_S * 100, HBM_BYTES_PER_S / 1e12))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "gpu"
    if mode == "cpu":
        cpu_probe()
    elif mode == "trace":
        fit_probe(reps=1)
    elif mode == "stats":
        trace_stats(sys.argv[2])
    else:
        fit_probe()
        step_probe()
        cpu_probe()
