#!/usr/bin/env python
"""tests/golden/make_golden_mvca.py -- generate mvca_golden.npz.

Runs ONLY where the reference tree is present.  The reference's own ``utils/divergence.py``, ``cluster/agglomerative.py``
and ``lumping/mvca.py`` are imported *by file path* over the stub modules of make_golden_msm.py (nothing of the reference
is copied into this repository) and their outputs are stored next to this script.  The inputs are regenerated from seeds
(tests/divergence_ref.py) by this script and by the tests alike.

THE LINKAGE UNDER THESE GOLDENS IS SCIPY'S, NOT FASTCLUSTER'S: a stub ``fastcluster`` module whose ``linkage`` is
``scipy.cluster.hierarchy.linkage`` stands in for the missing package, as in make_golden_landmark.py.  ``np.infty`` is
restored where numpy no longer has it, and ``msmbuilder.libdistance`` is an empty stub (MVCA's callable metric never
reaches it).  The MLE under the four-state system is make_golden_msm.mle_numpy, as for msm_golden.npz.

Stored:
  pair_<kind>_rows / _scalar / _array   the reference's pair functions on ``divergence_ref.golden_pair_rows()``: per row
                                        (scalar=False; kl_divergence only -- the reference's compound kinds fail or
                                        concatenate on the lists that form returns), summed (scalar=True), and
                                        ``<kind>_array(A, B, 2)``
  <system>_transmat (four only), _mapping, _mapping_fit_only, _pairwise, _linkage, _elbow
                                        the reference's MVCA on the four-state system (through ``fit``) and on the
                                        generated systems of 33 and 65 states (through ``from_msm(get_linkage=True)``)

Usage:  python tests/golden/make_golden_mvca.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_msm as M  # noqa: E402  (the loader recipe)
import divergence_ref as R  # noqa: E402


def load():
    MSM = M.load_reference_msm()
    import scipy.cluster.hierarchy
    fc = types.ModuleType("fastcluster")
    fc.linkage = scipy.cluster.hierarchy.linkage
    sys.modules["fastcluster"] = fc
    if not hasattr(np, "infty"):
        np.infty = np.inf
    sys.modules["msmbuilder.libdistance"] = types.ModuleType("msmbuilder.libdistance")
    sys.modules["msmbuilder"].libdistance = sys.modules["msmbuilder.libdistance"]
    sys.modules["msmbuilder.msm"].MarkovStateModel = MSM
    utils = sys.modules["msmbuilder.utils"]
    val = sys.modules["msmbuilder.utils.validation"]
    utils.check_iter_of_sequences = val.check_iter_of_sequences
    utils.array2d = val.array2d
    div = M._load("msmbuilder.utils.divergence", os.path.join(M.REF, "utils", "divergence.py"), "msmbuilder.utils")
    clu = types.ModuleType("msmbuilder.cluster")
    clu.__path__ = [os.path.join(M.REF, "cluster")]
    sys.modules["msmbuilder.cluster"] = clu
    base = M._load("msmbuilder.cluster.base", os.path.join(M.REF, "cluster", "base.py"), "msmbuilder.cluster")
    clu.MultiSequenceClusterMixin = base.MultiSequenceClusterMixin
    agg = M._load("msmbuilder.cluster.agglomerative", os.path.join(M.REF, "cluster", "agglomerative.py"), "msmbuilder.cluster")
    clu.LandmarkAgglomerative = agg.LandmarkAgglomerative
    lump = types.ModuleType("msmbuilder.lumping")
    lump.__path__ = [os.path.join(M.REF, "lumping")]
    sys.modules["msmbuilder.lumping"] = lump
    mvca = M._load("msmbuilder.lumping.mvca", os.path.join(M.REF, "lumping", "mvca.py"), "msmbuilder.lumping")
    return MSM, div, mvca.MVCA


def main():
    warnings.simplefilter("ignore")
    MSM, div, MVCA = load()
    g = {}
    A, B = R.golden_pair_rows()
    with np.errstate(all="ignore"):
        for kind in R.KINDS:
            fn = getattr(div, kind)
            if kind == "kl_divergence":   # (the reference's compound kinds do arithmetic on the LISTS scalar=False returns)
                g["pair_%s_rows" % kind] = np.asarray(fn(A, B, scalar=False), dtype=np.float64)
            g["pair_%s_scalar" % kind] = np.float64(fn(A, B))
            g["pair_%s_array" % kind] = np.asarray(getattr(div, kind + "_array")(A, B, 2), dtype=np.float64)

    def store(name, lumped, fit_only_lumped, linked):
        g[name + "_mapping"] = np.asarray(lumped.microstate_mapping_).astype(np.int16)
        g[name + "_mapping_fit_only"] = np.asarray(fit_only_lumped.microstate_mapping_).astype(np.int16)
        g[name + "_pairwise"] = np.asarray(linked.pairwise_dists, dtype=np.float64)
        g[name + "_linkage"] = np.asarray(linked.linkage, dtype=np.float64)
        g[name + "_elbow"] = np.asarray(linked.elbow_data, dtype=np.float64)
        print(name, "mapping", np.bincount(g[name + "_mapping"]).tolist(), "fit_only", np.bincount(g[name + "_mapping_fit_only"]).tolist())

    seq = [R.four_state_labels()]
    m = MVCA(n_macrostates=2, verbose=False).fit(seq)
    g["four_transmat"] = m.transmat_
    store("four", m, MVCA(n_macrostates=2, fit_only=True, verbose=False).fit(seq), MVCA.from_msm(MSM(verbose=False).fit(seq), 2, get_linkage=True))
    for name, (n, blocks, seed) in R.GOLDEN_GEN.items():
        msm = MSM(verbose=False)
        msm.transmat_, msm.populations_ = R.gen(n, blocks, seed), np.full(n, 1.0 / n)
        msm.mapping_, msm.countsmat_, msm.n_states_ = dict(zip(range(n), range(n))), None, n
        linked = MVCA.from_msm(msm, blocks, get_linkage=True)
        store(name, linked, MVCA.from_msm(msm, blocks, fit_only=True), linked)
    path = os.path.join(HERE, "mvca_golden.npz")
    np.savez_compressed(path, **g)
    print("mvca_golden.npz:", len(g), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
