#!/usr/bin/env python
"""tests/golden/make_golden_vmhmm.py -- generate vmhmm_golden.npz.

Runs ONLY where the reference tree is present.  The recipe of make_golden_hmm.py: the reference's hmm/vonmises.pyx is
cythonised and compiled with hmm/src/VonMisesHMMFitter.cpp and the cephes files its Bessel function needs (i0.c,
chbevl.c, mtherr.c) by the local Cython and compilers into a TEMPORARY directory outside this repository, and loaded by
file path over the same stub modules.  Nothing of the reference, neither text nor anything compiled from it, is copied
into this repository.  Only outputs are stored; the inputs are regenerated from seeds (tests/vmhmm_ref.py) by this
script and by the tests alike.

The start of every fit is fixed through a Python subclass whose ``_init`` calls ``__setstate__`` with the reference's
7-tuple.  Stored per case of vmhmm_ref.GOLDEN: fit_logprob_, means_, kappas_, transmat_, populations_, timescales_,
overlap_, score and predict on other data, summarize() with the time masked -- and ``dist_*``: the distance of each from
the longdouble restatement of the same fit (it also absorbs the reference's single-precision cos / sin of float32 rows),
and ``amp_*``: the measured amplification of an error in the E-step's sums into each quantity.

Usage:  python tests/golden/make_golden_vmhmm.py
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

import make_golden_hmm as G  # noqa: E402
import vmhmm_ref as V  # noqa: E402

REF = G.REF


def build_extension(tmp):
    """The reference's hmm.vonmises extension, built in tmp; returns the loaded module."""
    hmm = os.path.join(REF, "hmm")
    cpp = os.path.join(tmp, "vonmises.cpp")
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", os.path.join(hmm, "vonmises.pyx"), "-o", cpp])
    pyinc = sysconfig.get_paths()["include"]
    objs = []
    for name in ("i0", "chbevl", "mtherr"):
        obj = os.path.join(tmp, name + ".o")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-w", "-c", "-I", pyinc, "-I", np.get_include(), "-I", os.path.join(hmm, "cephes"),
                               os.path.join(hmm, "cephes", name + ".c"), "-o", obj])
        objs.append(obj)
    so = os.path.join(tmp, "vonmises" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-w", "-DNPY_NO_DEPRECATED_API=0", "-I", pyinc, "-I", np.get_include(),
                           "-I", os.path.join(hmm, "src", "include"), "-I", os.path.join(hmm, "src"),
                           "-I", os.path.join(hmm, "cephes"), "-I", tmp, cpp, os.path.join(hmm, "src", "VonMisesHMMFitter.cpp")]
                          + objs + ["-o", so])
    spec = importlib.util.spec_from_file_location("msmbuilder.hmm.vonmises", so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["msmbuilder.hmm.vonmises"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    warnings.simplefilter("ignore")
    G.stubs()
    mle = V.H.mle_solver()
    with tempfile.TemporaryDirectory() as tmp:
        ext = build_extension(tmp)

        class Fixed(ext.VonMisesHMM):
            def _init(self, sequences):
                starts = V.golden_starts(2)
                k = getattr(self, "_run", 0)
                self._run = k + 1
                means, kappas, transmat, pops = starts[k % len(starts)]
                self.__setstate__((means.copy(), kappas.copy(), transmat.copy(), pops.copy(), None, 0.0, means.shape[1]))

        g = {}
        for name, dn, kw, ragged, tight in V.GOLDEN:
            fit, other = V.golden_data(V.DT[dn], ragged=ragged, tight=tight)
            est = Fixed(n_states=3, **dict(dict(n_init=1), **kw)).fit(fit)
            lp, paths = est.predict(other)
            out = {"fit_logprob": np.asarray(est.fit_logprob_), "means": np.asarray(est.means_), "kappas": np.asarray(est.kappas_),
                   "transmat": np.asarray(est.transmat_), "populations": np.asarray(est.populations_),
                   "timescales": np.asarray(est.timescales_), "overlap": np.asarray(est.overlap_),
                   "score": np.float64(est.score(other)),
                   "predict_logprob": np.float64(lp), "predict_states": np.concatenate(paths).astype(np.int32),
                   "fit_states": np.concatenate(est.predict(fit)[1]).astype(np.int32)}
            (m, k, T, p), logs = V.golden_fit(fit, kw, mle, dt=np.longdouble, form='direct')
            lsp = np.tile(1.0 / 3, 3)
            yard = {"fit_logprob": logs, "means": m, "kappas": k, "transmat": T, "populations": p,
                    "overlap": V.overlap(m, k, in_place=True),   # (the reference's loop normalises in place)
                    "score": V.estep(other, m, k, T, lsp)["logprob"],
                    "predict_logprob": sum(V.viterbi(X, m, k, T, lsp)[0] for X in other)}
            for key, val in out.items():
                g[name + "_" + key] = val
            for key, val in yard.items():
                a = np.asarray(out[key], dtype=np.float64)
                b = np.asarray(val, dtype=np.float64)
                assert a.shape == b.shape, (name, key, a.shape, b.shape)
                # (the reference's overlap_ overflows to inf / nan where a concentration is above ~355: finite entries only)
                d = np.abs(a - b)[np.isfinite(a)]
                g[name + "_dist_" + key] = np.float64(d.max()) if d.size else np.float64(0.0)
            for key, val in V.golden_amplification(fit, other, kw, mle).items():
                g[name + "_amp_" + key] = np.float64(val)
            g[name + "_summarize"] = np.array(G.mask_time(est.summarize()))
            print(name, "iterations recorded", len(out["fit_logprob"]), "logprob", out["fit_logprob"][-1], "kappa max",
                  out["kappas"].max(), "dist", {k_: float(g[name + "_dist_" + k_]) for k_ in yard},
                  "amp", {k_: float(g[name + "_amp_" + k_]) for k_ in V.AMP_KEYS})
    np.savez_compressed(os.path.join(HERE, "vmhmm_golden.npz"), **g)
    print("vmhmm_golden.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
