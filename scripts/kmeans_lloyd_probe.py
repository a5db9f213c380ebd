"""Times one Lloyd iteration of KMeans against the label pass alone, on device-resident rows (HIP events).

    python scripts/kmeans_lloyd_probe.py > profiles/kmeans_lloyd_probe.txt

Shapes: 10M x 10 float64 and 1.25M x 512 float32, K = 1000.  The label pass is msm_mbk_label on the same rows and centres;
an iteration is (time of 10 queued iterations - time of 2) / 8, which cancels the set-up and the final labelling; the
update is the difference of the two, and its GB/s counts one read of the rows.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmbuilder_amd import _lib  # noqa: E402
from msmbuilder_amd._lib import Arr, check  # noqa: E402
from msmbuilder_amd.cluster.kmeans import lloyd_plan, lloyd_run  # noqa: E402


def timed(fn, reps):
    L = _lib.lib()
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(L.msm_event_create(C.byref(e0)))
    check(L.msm_event_create(C.byref(e1)))
    best = float("inf")
    for _ in range(reps):
        check(L.msm_event_record(e0))
        fn()
        check(L.msm_event_record(e1))
        _lib.synchronize()
        ms = C.c_float(0)
        check(L.msm_event_elapsed_ms(e0, e1, C.byref(ms)))
        best = min(best, ms.value)
    L.msm_event_destroy(e0)
    L.msm_event_destroy(e1)
    return best


def probe(n, m, K, dtype):
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(n, m, dtype=tdt, device="cuda", generator=g)
    centers = X[torch.randperm(n, device="cuda", generator=g)[:K]].cpu().numpy()
    ax = Arr(X)
    L = _lib.lib()
    h = C.c_void_p()
    check((L.msm_mbk_create_f64 if dtype == np.float64 else L.msm_mbk_create)(C.byref(h), K, m))
    zero = np.zeros(K, dtype=dtype)
    check(L.msm_mbk_set(h, centers.ctypes.data, zero.ctypes.data))
    labels = torch.empty(n, dtype=torch.int32, device="cuda")

    def label():
        check(L.msm_mbk_label(h, ax.vp, n, C.c_void_p(labels.data_ptr()), None, 1))
    label()
    t_label = timed(label, 5)
    L.msm_mbk_destroy(h)
    lloyd_run(X, centers, 2, 0.0)
    t2 = timed(lambda: lloyd_run(X, centers, 2, 0.0), 3)
    t10 = timed(lambda: lloyd_run(X, centers, 10, 0.0), 3)
    t_iter = (t10 - t2) / 8.0
    t_upd = t_iter - t_label
    gb = n * m * np.dtype(dtype).itemsize / 1e9
    print("%d x %d %s, K = %d: plan %s" % (n, m, np.dtype(dtype).name, K, lloyd_plan(n, m, K, dtype)))
    print("  label pass alone     %8.3f ms" % t_label)
    print("  whole iteration      %8.3f ms   (%.2f x the label pass; 2 iterations %.3f ms, 10 iterations %.3f ms)"
          % (t_iter, t_iter / t_label, t2, t10))
    print("  update (difference)  %8.3f ms   %.0f GB/s over one read of the %.2f GB of rows" % (t_upd, gb / (t_upd * 1e-3), gb))
    sys.stdout.flush()


if __name__ == "__main__":
    _lib.ensure_device(0)
    probe(10_000_000, 10, 1000, np.float64)
    probe(1_250_000, 512, 1000, np.float32)
