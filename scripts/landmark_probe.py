"""Times LandmarkAgglomerative on the GPU beside the numpy / scipy restatement on the same machine: fit and predict at
280,000 x 10 float32 rows, 2,000 stride landmarks, K = 200, average and ward linkage.

    python scripts/landmark_probe.py > profiles/landmark_probe.txt            (on the GPU)
    python scripts/landmark_probe.py tiny                                      (any size check of the script itself)

GPU times are host clocks around calls that end in a device synchronisation (fit reads Z, predict returns host labels),
best of 3 after a warm-up, on device-resident rows; the pieces of fit (pdist + linkage, within-cluster sums) and the
predict kernel alone (labels left on the device) are timed the same way.  The CPU side, one run each on one thread:
scipy's linkage of the same condensed matrix (what the reference calls through fastcluster), the restatement's own
linkage loop, the within-cluster sums and the pooled predict of tests/landmark_ref.py over the C oracle's cdist, in row
blocks of 20,000 so that the N x L matrix (4.5 GB) is never held at once.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def rows(n, m, seed):
    rs = np.random.RandomState(seed)
    hubs = rs.randn(200, m) * 3.0
    return np.ascontiguousarray((hubs[rs.randint(0, 200, n)] + rs.randn(n, m)).astype(np.float32))


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


def once(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def gpu_probe(X, L, K, lk):
    import torch
    from msmbuilder_amd._lib import Arr
    from msmbuilder_amd.cluster import agglomerative as A
    Xd = torch.as_tensor(X, device="cuda")
    fit_ms, est = best_of(lambda: A._LandmarkAgglomerative(n_clusters=K, n_landmarks=L, linkage=lk).fit(Xd))
    pred_ms, labels = best_of(lambda: est.predict(Xd))
    idx = A.landmark_indices(len(X), L)
    link_ms, _ = best_of(lambda: A.linkage_fit(Arr(Xd), "euclidean", lk, idx))
    within_ms, _ = best_of(lambda: A.within_cluster(None, L, est.landmark_labels_, K))
    perm, off = A.permute_by_cluster(est.landmark_labels_, K)
    lm = np.ascontiguousarray(est.landmarks_[perm])
    kern_ms, _ = best_of(lambda: A.pooled_predict(Arr(Xd), lm, off, est.squared_distances_within_cluster_, "euclidean", lk))
    n, m = X.shape
    print("GPU  %-7s fit %8.1f ms (pdist + linkage of %d landmarks, %d queued launches: %.1f ms; within-cluster sums %.2f ms; "
          "the rest is fcluster, bincount and the centres on the host)" % (lk, fit_ms, L, 3 * (L - 1) + 1, link_ms, within_ms))
    print("GPU  %-7s predict %6.1f ms for %d x %d float32 rows against %d landmarks (labels to the host); the kernel call alone "
          "%.1f ms = %.1f G distance terms/s" % (lk, pred_ms, n, m, L, kern_ms, n * float(L) * m / kern_ms / 1e6))
    return est, labels


def cpu_probe(X, L, K, lk, est, labels, block=20000):
    import landmark_ref as R
    from scipy.cluster.hierarchy import linkage
    idx = R.landmark_indices(len(X), L)
    lm = np.ascontiguousarray(X[idx])
    pd_ms, D = once(lambda: R._oracle().pdist(lm, "euclidean"))
    sp_ms, Zs = once(lambda: linkage(D, method=lk))
    re_ms, Z = once(lambda: R.linkage(D, lk))
    ll = R.labels_from_linkage(Z, K)
    wi_ms, intra = once(lambda: R.within(D, ll, K))

    def predict():
        out = np.empty(len(X), dtype=np.int64)
        for a in range(0, len(X), block):
            out[a:a + block] = R.pooled_predict(R.exact_cdist(X[a:a + block], lm, "euclidean"), ll, K, lk, intra)[0]
        return out
    pr_ms, want = once(predict)
    same_tree = bool(np.array_equal(Z[:, :2], Zs[:, :2]))
    print("CPU  %-7s pdist (C oracle) %.0f ms; scipy linkage %.0f ms; restatement linkage loop %.0f ms; within-cluster sums "
          "%.0f ms; pooled predict in blocks of %d rows %.0f ms" % (lk, pd_ms, sp_ms, re_ms, wi_ms, block, pr_ms))
    print("     %-7s same merges as scipy: %s; landmark labels equal to the GPU fit's: %s; predicted labels equal: %d of %d"
          % (lk, same_tree, bool(np.array_equal(ll, est.landmark_labels_)), int(np.sum(want == labels)), len(want)))


if __name__ == "__main__":
    tiny = len(sys.argv) > 1 and sys.argv[1] == "tiny"
    n, L, K = (3000, 100, 10) if tiny else (280000, 2000, 200)
    X = rows(n, 10, 0)
    print("# python scripts/landmark_probe.py on an MI355X, %s: %d x 10 float32, %d stride landmarks, K = %d"
          % (time.strftime("%Y-%m-%d"), n, L, K))
    for lk in ("average", "ward"):
        est, labels = gpu_probe(X, L, K, lk)
        cpu_probe(X, L, K, lk, est, labels)
