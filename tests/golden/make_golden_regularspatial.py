#!/usr/bin/env python
"""tests/golden/make_golden_regularspatial.py -- generate regularspatial_golden.npz.

Runs ONLY where the reference tree is present (like make_golden.py, whose loader it uses): the reference's own
cluster/regularspatial.py is imported *by file path* over the reference's libdistance headers compiled in oracle/_ref --
nothing of the reference is copied into this repository -- and its outputs are stored next to this script.  The inputs
are regenerated from seeds (tests/regularspatial_ref.py) by this script and by the tests alike.

Stored, per metric and dtype on a 3,000 x 5 walk (rounded for hamming / jaccard): d_min, ids, centres, predicted labels;
for a ragged list of four trajectories: the (trajectory, frame) pairs, labels, n_clusters_ and the summarize() text.

Usage:  python tests/golden/make_golden_regularspatial.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (the loader recipe)
import regularspatial_ref as R  # noqa: E402


def small_input(metric, dt):
    X = R.walk(3000, 5, seed=1)
    if metric in ("hamming", "jaccard"):
        X = np.rint(X)
    return np.ascontiguousarray(X.astype(dt))


def main():
    warnings.simplefilter("ignore")
    _, _, ref = make_golden.load_reference()
    mod = make_golden._load("msmbuilder.cluster.regularspatial",
                            os.path.join(make_golden.REF, "cluster", "regularspatial.py"), "msmbuilder.cluster")
    g = {}
    for metric in R.METRICS:
        for dn, dt in (("f32", np.float32), ("f64", np.float64)):
            X = small_input(metric, dt)
            # a d_min that gives a few dozen centres whatever the metric's scale: a quarter of the median distance to row 0,
            # moved off the attained values for the two metrics that only take multiples of 1 / m
            with np.errstate(all="ignore"):
                d0 = ref.dist(X, X[0], metric)
            d_min = float(np.nanmedian(d0)) * 0.25
            if metric in ("hamming", "jaccard"):
                d_min = 0.7
            m = mod._RegularSpatial(d_min=d_min, metric=metric).fit(X)
            p = "%s_%s_" % (metric, dn)
            g[p + "d_min"] = np.float64(d_min)
            g[p + "ids"] = np.array(m.cluster_center_indices_, dtype=np.int64)
            g[p + "centers"] = m.cluster_centers_
            g[p + "predict"] = m.predict(X)
            assert m.n_clusters_ == len(g[p + "ids"])
            print(p, "d_min %.4g" % d_min, "K", m.n_clusters_)
    seqs = R.golden_sequences()
    m = mod.RegularSpatial(d_min=0.9).fit(seqs)
    g["seq_d_min"] = np.float64(0.9)
    g["seq_pairs"] = np.asarray(m.cluster_center_indices_)
    g["seq_centers"] = m.cluster_centers_
    g["seq_n_clusters"] = np.int64(m.n_clusters_)
    g["seq_predict"] = np.concatenate(m.predict(seqs))
    g["seq_summarize"] = np.array(m.summarize())
    print("ragged list: K", m.n_clusters_, "pairs", g["seq_pairs"][:4].tolist())
    np.savez_compressed(os.path.join(HERE, "regularspatial_golden.npz"), **g)
    print("regularspatial_golden.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
