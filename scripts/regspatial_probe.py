"""Times RegularSpatial.fit on device-resident rows beside libdistance.assign_nearest of the same rows against the final
centres (the same N x K exact distances WITHOUT the early exit: the screen cannot need more arithmetic than that call).

    python scripts/regspatial_probe.py > profiles/regspatial_probe.txt          (on the GPU)
    python scripts/regspatial_probe.py cpu                                      (the reference loop's per-row cost, CPU)

Shapes: 10M x 10 float64 (the bench's clustering shape: 1,000 trajectories of 10,000 frames of a 10-component
projection) and 2M x 171 float32 (contact features), both time-ordered Ornstein-Uhlenbeck trajectories generated from a
seed; d_min is bisected with the fit itself until K is near 200.  Times are host clocks around calls that end in a device
synchronisation, best of 3 after a warm-up; the stats line is msm_regspatial_last_stats.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trajectories_host(n_traj, frames, m, seed, slow=None):
    """[n_traj * frames, m] float64: every trajectory an OU process per slow coordinate (relaxation times 500 / (1 + j)
    frames, scales 3 .. 0.4); m > slow: mixed into m features plus white noise (contact-like)."""
    rs = np.random.RandomState(seed)
    k = slow or m
    a = np.exp(-1.0 / (500.0 / (1.0 + np.arange(k))))
    z = np.empty((frames, n_traj, k))
    z[0] = rs.randn(n_traj, k)
    s = np.sqrt(1.0 - a * a)
    for t in range(1, frames):
        z[t] = a * z[t - 1] + s * rs.randn(n_traj, k)
    z = np.ascontiguousarray(z.transpose(1, 0, 2)).reshape(n_traj * frames, k) * np.linspace(3.0, 0.4, k)
    if k == m:
        return z
    return z @ rs.randn(k, m) + 0.3 * rs.randn(n_traj * frames, m)


def trajectories_device(n_traj, frames, m, seed, dtype, slow=None):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = slow or m
    a = torch.exp(-1.0 / (500.0 / (1.0 + torch.arange(k, dtype=torch.float64, device="cuda"))))
    s = torch.sqrt(1.0 - a * a)
    z = torch.empty(frames, n_traj, k, dtype=torch.float64, device="cuda")
    z[0] = torch.randn(n_traj, k, dtype=torch.float64, device="cuda", generator=g)
    for t in range(1, frames):
        z[t] = a * z[t - 1] + s * torch.randn(n_traj, k, dtype=torch.float64, device="cuda", generator=g)
    z = z.permute(1, 0, 2).reshape(n_traj * frames, k) * torch.linspace(3.0, 0.4, k, dtype=torch.float64, device="cuda")
    if k != m:
        W = torch.randn(k, m, dtype=torch.float64, device="cuda", generator=g)
        z = z @ W + 0.3 * torch.randn(n_traj * frames, m, dtype=torch.float64, device="cuda", generator=g)
    return z.to(dtype).contiguous()


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


def probe(n_traj, frames, m, dtype, lo, hi, slow=None):
    import torch
    from msmbuilder_amd import libdistance
    from msmbuilder_amd.cluster.regularspatial import _RegularSpatial, last_stats
    X = trajectories_device(n_traj, frames, m, 0, dtype, slow)
    n = X.shape[0]
    print("%d x %d %s (%d trajectories of %d frames)" % (n, m, str(dtype).replace("torch.", ""), n_traj, frames))
    d_min, est = None, None
    for _ in range(12):   # K falls as d_min grows
        d_min = 0.5 * (lo + hi)
        est = _RegularSpatial(d_min).fit(X)
        print("  bisect: d_min %.4f -> K = %d" % (d_min, est.n_clusters_))
        if 180 <= est.n_clusters_ <= 220:
            break
        if est.n_clusters_ > 220:
            lo = d_min
        else:
            hi = d_min
    t_fit, est = best_of(lambda: _RegularSpatial(d_min).fit(X))
    st = last_stats()
    centers = est.cluster_centers_
    t_assign, _ = best_of(lambda: libdistance.assign_nearest(X, centers, "euclidean"))
    print("  fit            %9.3f ms   d_min %.4f, K = %d, stats %s" % (t_fit, d_min, est.n_clusters_, st))
    print("  assign_nearest %9.3f ms   (%d x %d exact distances, no early exit)   fit / assign = %.2f"
          % (t_assign, n, est.n_clusters_, t_fit / t_assign))
    sys.stdout.flush()
    del X
    torch.cuda.empty_cache()


def cpu_reference(rows=200_000):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import regularspatial_ref as R
    X = trajectories_host(rows // 10_000, 10_000, 10, 0)
    for d_min in (7.2812, 4.375):   # the GPU probe's final d_min (K near 200 on 10M rows) and a denser one
        t = time.perf_counter()
        ids = R.ref_fit(X, d_min)
        dt = time.perf_counter() - t
        print("reference loop (CPU, one thread), %d x 10 float64, d_min %.4g: K = %d, %.2f s = %.2f us per row; "
              "EXTRAPOLATED to 10M rows at this K: %.0f s" % (rows, d_min, len(ids), dt, dt / rows * 1e6, dt / rows * 1e7))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cpu":
        cpu_reference()
    else:
        import torch
        from msmbuilder_amd import _lib
        _lib.ensure_device(0)
        probe(1000, 10_000, 10, torch.float64, 0.5, 16.0)
        probe(200, 10_000, 171, torch.float32, 4.0, 80.0, slow=6)
