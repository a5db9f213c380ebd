#!/usr/bin/env python
"""tests/golden/make_golden_landmark.py -- generate landmark_golden.npz.

Runs ONLY where the reference tree is present (like make_golden.py, whose loader it uses): the reference's own
cluster/agglomerative.py is imported *by file path* over the reference's libdistance headers compiled in oracle/_ref --
nothing of the reference is copied into this repository -- and its outputs are stored next to this script.  The inputs
are regenerated from seeds (tests/landmark_ref.py) by this script and by the tests alike.

THE LINKAGE UNDER THESE GOLDENS IS SCIPY'S, NOT FASTCLUSTER'S.  The reference imports ``fastcluster.linkage``, which is not
installed where this script runs; a stub ``fastcluster`` module whose ``linkage`` is ``scipy.cluster.hierarchy.linkage``
(scipy ported the same algorithms from fastcluster) stands in for it.  Two more stand-ins let the file load on current
libraries: ``np.infty = np.inf`` where numpy no longer has it, and ``pdist`` added to the fake ``msmbuilder.libdistance``
module (the compiled reference headers).  Everything else -- landmark choice, fcluster, the loop over all pairs, the
pooling functions and the label selection of predict -- is the reference estimator's own code.

Stored, per case of ``landmark_ref.GOLDEN_CASES`` (a 3,000 x 5 random walk, 120 landmarks, 7 clusters; 300 rows where every
row is a landmark): landmark_labels_, cardinality_, cluster_centers_, squared_distances_within_cluster_ and the predicted
labels of the training rows; the seed of the random-landmark cases (the lowest that draws no row twice); and for a ragged
list of four trajectories through the sequence mixin the same attributes and labels.

Usage:  python tests/golden/make_golden_landmark.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (the loader recipe)
import landmark_ref as R  # noqa: E402


def load():
    _, _, ref = make_golden.load_reference()
    import scipy.cluster.hierarchy
    fc = types.ModuleType("fastcluster")
    fc.linkage = scipy.cluster.hierarchy.linkage
    sys.modules["fastcluster"] = fc
    if not hasattr(np, "infty"):
        np.infty = np.inf
    sys.modules["msmbuilder.libdistance"].pdist = ref.pdist
    return make_golden._load("msmbuilder.cluster.agglomerative",
                             os.path.join(make_golden.REF, "cluster", "agglomerative.py"), "msmbuilder.cluster")


def store(g, p, m, labels):
    g[p + "landmark_labels"] = np.asarray(m.landmark_labels_).astype(np.int16)
    g[p + "cardinality"] = np.asarray(m.cardinality_).astype(np.int64)
    g[p + "centers"] = m.cluster_centers_
    g[p + "within"] = np.asarray(m.squared_distances_within_cluster_, dtype=np.float64)
    g[p + "predict"] = np.asarray(labels).astype(np.int8)


def main():
    warnings.simplefilter("ignore")
    mod = load()
    g = {}
    seed = R.random_seed_without_duplicate()
    g["random_seed"] = np.int64(seed)
    for name, lk, dn, strategy, n_landmarks, rows, ward_predictor in R.GOLDEN_CASES:
        X = R.walk(dt=R.DT[dn])[:rows]
        m = mod._LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=n_landmarks, linkage=lk, landmark_strategy=strategy,
                                       random_state=seed, ward_predictor=ward_predictor).fit(X)
        labels = m.predict(X)
        store(g, name + "_", m, labels)
        print(name, "cardinality", m.cardinality_.tolist(), "label counts", np.bincount(labels, minlength=R.GOLDEN_K).tolist())
    seqs = R.golden_sequences()
    m = mod.LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage="average").fit(seqs)
    store(g, "seq_", m, np.concatenate(m.predict(seqs)))
    g["seq_fit_predict"] = np.concatenate(
        mod.LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage="ward").fit_predict(seqs)).astype(np.int8)
    np.savez_compressed(os.path.join(HERE, "landmark_golden.npz"), **g)
    print("landmark_golden.npz:", len(g), "arrays,", os.path.getsize(os.path.join(HERE, "landmark_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
