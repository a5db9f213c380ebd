#!/usr/bin/env python
"""tests/golden/make_golden_nystroem.py -- generate nystroem_golden.npz.

Runs ONLY where the reference tree is present (like make_golden_landmark.py, whose loader recipe it uses): the reference's
own decomposition/base.py, kernel_approximation.py and ktica.py are imported *by file path* -- nothing of the reference is
copied into this repository -- and their outputs are stored next to this script.  One stand-in lets the files load on a
current Python: ``collections.Sequence = collections.abc.Sequence``.  The inputs are regenerated from seeds
(tests/nystroem_ref.py) by this script and by the tests alike; only the landmarks of the random-basis case are stored.

Stored:
  * per estimator case ``<kernel>_<F>_<L>`` of ``nystroem_ref.EST_CASES`` (LandmarkNystroem over standard-normal landmarks,
    float64): ``normalization_`` and the features of 50 rows;
  * ``nys_*``: ``Nystroem(n_components=20, random_state=3)`` over three trajectories: component_indices_, components_,
    normalization_, the features;
  * ``kt_*``: ``KernelTICA`` (rbf, 24 landmarks, lag 3, 4 components) on three double-well trajectories, plain and with
    kinetic mapping: eigenvalues, the projections, ``score`` of a fourth trajectory.

The maker ASSERTS that the goldens are decidable at the project's standing tolerances: the reference's top 4 eigenvalues
move by less than rtol 1e-5 when its input is rounded to float32, and by less than rtol 1e-10 under a relative
perturbation of 2^-45 (256 float64 roundoffs) of its input; and that every basis kernel has sigma_min / sigma_max > 1e-6.

Usage:  python tests/golden/make_golden_nystroem.py
"""
import collections
import collections.abc
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (the loader recipe)
import nystroem_ref as R  # noqa: E402


def load():
    make_golden.load_reference()
    if not hasattr(collections, "Sequence"):
        collections.Sequence = collections.abc.Sequence
    dec = os.path.join(make_golden.REF, "decomposition")
    make_golden._load("msmbuilder.decomposition.base", os.path.join(dec, "base.py"), "msmbuilder.decomposition")
    ka = make_golden._load("msmbuilder.decomposition.kernel_approximation", os.path.join(dec, "kernel_approximation.py"),
                           "msmbuilder.decomposition")
    kt = make_golden._load("msmbuilder.decomposition.ktica", os.path.join(dec, "ktica.py"), "msmbuilder.decomposition")
    return ka, kt


def main():
    warnings.simplefilter("ignore")
    ka, kt = load()
    g = {}
    for kernel, cases in R.EST_CASES.items():
        for F, L in cases:
            X, Lm = R.data(R.est_seed(kernel, F, L), 50, F, L)
            m = ka.LandmarkNystroem(landmarks=Lm, **R.params(kernel)).fit([X])
            ratio, _ = R.condition(R.kernel_values(Lm, Lm, **R.params(kernel)))
            assert ratio > 1e-6, (kernel, F, L, ratio)
            p = "%s_%d_%d_" % (kernel, F, L)
            g[p + "normalization"] = m.normalization_
            g[p + "features"] = m.transform([X])[0]
            print(p, "sigma_min/sigma_max %.3g, max|normalization_| %.3g" % (ratio, np.abs(m.normalization_).max()))

    seqs = R.nystroem_sequences()
    m = ka.Nystroem(n_components=20, random_state=3, **R.params("rbf")).fit(seqs)
    g["nys_indices"] = np.asarray(m.component_indices_, dtype=np.int64)
    g["nys_components"] = m.components_
    g["nys_normalization"] = m.normalization_
    g["nys_features"] = np.concatenate(m.transform(seqs))

    seqs, lm = R.ktica_sequences()
    test = R.double_well(999, 300)

    def fit(seqs_, lm_, **kw):
        model = kt.KernelTICA(landmarks=lm_, **dict(R.KTICA_KW, **kw))
        model.fit(seqs_)
        return model

    base = fit(seqs, lm)
    ev = base.eigenvalues_
    r32 = fit([s.astype(np.float32).astype(np.float64) for s in seqs], lm.astype(np.float32).astype(np.float64)).eigenvalues_
    rs = np.random.RandomState(0)
    pert = fit([s * (1 + 2.0 ** -45 * rs.uniform(-1, 1, s.shape)) for s in seqs], lm).eigenvalues_
    print("eigenvalues", ev, "\n float32-rounded input: rel. change", np.abs(r32 - ev) / np.abs(ev),
          "\n 2^-45 perturbation: rel. change", np.abs(pert - ev) / np.abs(ev))
    assert (np.abs(r32 - ev) < 1e-5 * np.abs(ev)).all(), "not decidable at rtol 1e-5"
    assert (np.abs(pert - ev) < 1e-10 * np.abs(ev)).all(), "not decidable at rtol 1e-10"
    ratio, _ = R.condition(R.kernel_values(lm, lm, R.KTICA_KW["kernel"], R.KTICA_KW["gamma"]))
    assert ratio > 1e-6, ratio
    g["kt_eigenvalues"] = ev
    g["kt_eigenvalues_f32_input"] = r32
    g["kt_normalization"] = base._nystroem.normalization_
    g["kt_transform"] = np.concatenate(base.transform(seqs))
    g["kt_score"] = np.float64(base.score([test]))
    kin = fit(seqs, lm, kinetic_mapping=True)
    g["kt_transform_kinetic"] = np.concatenate(kin.transform(seqs))
    print("score", g["kt_score"], "basis sigma_min/sigma_max %.3g" % ratio)
    out = os.path.join(HERE, "nystroem_golden.npz")
    np.savez_compressed(out, **g)
    print("nystroem_golden.npz:", len(g), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
