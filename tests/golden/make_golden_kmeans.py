"""Captures tests/golden/kmeans_golden.npz from scikit-learn's KMeans (run with scikit-learn 1.7.2).  The inputs are
regenerated from seeds by tests/kmeans_lloyd_ref.golden_inputs; only scikit-learn's results are stored."""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_lloyd_ref as LR  # noqa: E402


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in LR.GOLDEN_NAMES:
        X, kw = LR.golden_inputs(name)
        km = KMeans(algorithm="lloyd", **kw).fit(X)
        out[name + "_centers"] = km.cluster_centers_
        out[name + "_labels"] = km.labels_.astype(np.int32)
        out[name + "_inertia"] = np.array(km.inertia_)
        out[name + "_n_iter"] = np.array(km.n_iter_)
    np.savez_compressed(os.path.join(HERE, "kmeans_golden.npz"), **out)


if __name__ == "__main__":
    main()
