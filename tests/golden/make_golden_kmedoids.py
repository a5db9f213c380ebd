#!/usr/bin/env python
"""tests/golden/make_golden_kmedoids.py -- generate kmedoids_golden.npz.

Runs ONLY where the reference tree is present (like make_golden.py, whose loader it uses).  The reference's
cluster/_kmedoids.pyx and cluster/src/kmedoids.cc are compiled with the local Cython and C++ compiler into a TEMPORARY
directory outside this repository, and its cluster/kmedoids.py and cluster/minibatchkmedoids.py are imported *by file
path* over that extension and the reference's libdistance headers compiled in oracle/_ref -- nothing of the reference,
neither text nor anything compiled from it, is copied into this repository.  Only outputs are stored; the inputs are
regenerated from seeds (tests/kmedoids_ref.py) by this script and by the tests alike.

Two flags the build needs: ``-DPyInt_AsLong=PyLong_AsLong`` (numpy 2 no longer supplies that name) and ``-O0`` (the
reference's initialize_numpy is a non-void function without a return: optimised, it falls through and the process
dies in randomassign).

Stored: for raw loop cases clusterid / error / ifound; for KMedoids per metric and dtype labels_, cluster_ids_,
cluster_centers_, inertia_, predict and the generator's next draw; for MiniBatchKMedoids the same; for a ragged list of
four trajectories the (trajectory, frame) pairs, labels and the summarize() texts.

Usage:  python tests/golden/make_golden_kmedoids.py
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (the loader recipe)
import kmedoids_ref as R  # noqa: E402


def build_extension(tmp):
    """The reference's _kmedoids extension, built in tmp; returns the loaded module."""
    clu = os.path.join(make_golden.REF, "cluster")
    cpp = os.path.join(tmp, "_kmedoids.cpp")
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", os.path.join(clu, "_kmedoids.pyx"), "-o", cpp])
    so = os.path.join(tmp, "_kmedoids" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O0", "-shared", "-fPIC", "-w", "-DPyInt_AsLong=PyLong_AsLong",
                           "-DNPY_NO_DEPRECATED_API=0", "-I", sysconfig.get_paths()["include"], "-I", np.get_include(),
                           "-I", clu, cpp, os.path.join(clu, "src", "kmedoids.cc"), "-o", so])
    spec = importlib.util.spec_from_file_location("msmbuilder.cluster._kmedoids", so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["msmbuilder.cluster._kmedoids"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    warnings.simplefilter("ignore")
    _, _, ref = make_golden.load_reference()
    sys.modules["msmbuilder.libdistance"].pdist = ref.pdist
    with tempfile.TemporaryDirectory() as tmp:
        ext = build_extension(tmp)
        sys.modules["msmbuilder.cluster"]._kmedoids = ext
        km = make_golden._load("msmbuilder.cluster.kmedoids", os.path.join(make_golden.REF, "cluster", "kmedoids.py"),
                               "msmbuilder.cluster")
        mb = make_golden._load("msmbuilder.cluster.minibatchkmedoids",
                               os.path.join(make_golden.REF, "cluster", "minibatchkmedoids.py"), "msmbuilder.cluster")
        g = {}
        for case in R.GOLDEN_LOOP:
            n, K, npass, seed, metric = case
            D, start, rs = R.loop_case(*case)
            ids, error, ifound = ext.kmedoids(K, D, npass, start, random_state=rs)
            p = "loop_%d_%d_%d_%d_" % (n, K, npass, seed)
            g[p + "ids"] = np.asarray(ids, dtype=np.int64)
            g[p + "error"] = np.float64(error)
            g[p + "ifound"] = np.int64(ifound)
            g[p + "next"] = np.float64(rs.random_sample())
            print(p, "error", error, "ifound", ifound)
        for metric, dn, n, m, seed, K, npasses in R.GOLDEN_KMEDOIDS:
            X = R.cloud(n, m, seed, R.DT[dn], metric)
            rs = np.random.RandomState(seed)
            est = km._KMedoids(n_clusters=K, n_passes=npasses, metric=metric, random_state=rs).fit(X)
            p = "km_%s_%s_" % (metric, dn)
            g[p + "labels"] = np.asarray(est.labels_, dtype=np.int64)
            g[p + "cluster_ids"] = np.asarray(est.cluster_ids_, dtype=np.int64)
            g[p + "centers"] = est.cluster_centers_
            g[p + "inertia"] = np.float64(est.inertia_)
            g[p + "predict"] = np.asarray(est.predict(X[::-1].copy()), dtype=np.int64)
            g[p + "next"] = np.float64(rs.random_sample())
            print(p, "n", n, "K", K, "passes", npasses, "inertia", est.inertia_)
        for metric, dn, n, m, seed, kw in R.GOLDEN_MINIBATCH:
            X = R.cloud(n, m, seed, R.DT[dn], metric)
            rs = np.random.RandomState(seed)
            est = mb._MiniBatchKMedoids(metric=metric, random_state=rs, **kw).fit(X)
            p = "mb_%s_%s_" % (metric, dn)
            g[p + "labels"] = np.asarray(est.labels_, dtype=np.int64)
            g[p + "cluster_ids"] = np.asarray(est.cluster_ids_, dtype=np.int64)
            g[p + "centers"] = est.cluster_centers_
            g[p + "inertia"] = np.float64(est.inertia_)
            g[p + "next"] = np.float64(rs.random_sample())
            print(p, "n", n, kw, "inertia", est.inertia_)
        seqs = R.golden_sequences()
        est = km.KMedoids(n_clusters=5, n_passes=2, random_state=3).fit(seqs)
        g["seq_km_pairs"] = np.asarray(est.cluster_ids_)
        g["seq_km_labels"] = np.concatenate(est.labels_).astype(np.int64)
        g["seq_km_centers"] = est.cluster_centers_
        g["seq_km_inertia"] = np.float64(est.inertia_)
        g["seq_km_predict"] = np.concatenate(est.predict(seqs)).astype(np.int64)
        g["seq_km_summarize"] = np.array(est.summarize())
        est = mb.MiniBatchKMedoids(n_clusters=5, batch_size=40, random_state=3).fit(seqs)
        g["seq_mb_pairs"] = np.asarray(est.cluster_ids_)
        g["seq_mb_labels"] = np.concatenate(est.labels_).astype(np.int64)
        g["seq_mb_centers"] = est.cluster_centers_
        g["seq_mb_inertia"] = np.float64(est.inertia_)
        g["seq_mb_summarize"] = np.array(est.summarize())
    np.savez_compressed(os.path.join(HERE, "kmedoids_golden.npz"), **g)
    print("kmedoids_golden.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
