#!/usr/bin/env python
"""tests/golden/make_golden_hmm.py -- generate hmm_golden.npz.

Runs ONLY where the reference tree is present.  The reference's hmm/gaussian.pyx is cythonised and compiled with
hmm/src/GaussianHMMFitter.cpp by the local Cython and C++ compiler into a TEMPORARY directory outside this repository
(the recipe of make_golden_kmedoids.py) and loaded by file path over stub modules for what it imports but these cases
never reach (mdtraj.utils.ensure_type, msmbuilder.utils, hmm.discrete_approx); msmbuilder.msm._markovstatemodel's
_transmat_mle_prinz is make_golden_msm.mle_numpy, as for the MSM goldens.  Nothing of the reference, neither text nor
anything compiled from it, is copied into this repository.  Only outputs are stored; the inputs are regenerated from
seeds (tests/hmm_ref.py) by this script and by the tests alike.

The start of every fit is fixed through a Python subclass whose ``_init`` calls ``__setstate__`` (the extension's
attributes cannot be set any other way).  The extension keeps its raw statistics private, so what is stored per case of
hmm_ref.GOLDEN is public: fit_logprob_, means_, vars_, transmat_, populations_, timescales_, score and predict on other
data, summarize() with the time masked -- and ``dist_*``: the distance of each from the longdouble restatement of the
same fit, which the tests add to their bound, and ``amp_*``: the measured amplification of an error in the E-step's sums
into each quantity (hmm_ref.golden_amplification), which carries that bound from the sums to the quantity.

Usage:  python tests/golden/make_golden_hmm.py
"""
import contextlib
import importlib.util
import os
import re
import subprocess
import sys
import sysconfig
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_msm  # noqa: E402
import hmm_ref as R  # noqa: E402

REF = make_golden_msm.REF


def stubs():
    for alias, typ in (("int", int), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)
    md = types.ModuleType("mdtraj")
    mdu = types.ModuleType("mdtraj.utils")
    mdu.ensure_type = lambda val, dtype=None, ndim=None, name=None, **kw: np.asarray(val, dtype=dtype)
    md.utils = mdu
    sys.modules["mdtraj"] = md
    sys.modules["mdtraj.utils"] = mdu
    pkg = types.ModuleType("msmbuilder")
    pkg.__path__ = [REF]
    sys.modules["msmbuilder"] = pkg
    utils = types.ModuleType("msmbuilder.utils")

    def check_iter_of_sequences(sequences, **kw):
        if not all(getattr(s, "ndim", 0) == 2 for s in sequences):
            raise ValueError("sequences must be a list of sequences")

    @contextlib.contextmanager
    def printoptions(*args, **kwargs):
        original = np.get_printoptions()
        np.set_printoptions(*args, **kwargs)
        try:
            yield
        finally:
            np.set_printoptions(**original)
    utils.check_iter_of_sequences = check_iter_of_sequences
    utils.printoptions = printoptions
    sys.modules["msmbuilder.utils"] = utils
    hmm = types.ModuleType("msmbuilder.hmm")
    hmm.__path__ = [os.path.join(REF, "hmm")]
    sys.modules["msmbuilder.hmm"] = hmm
    da = types.ModuleType("msmbuilder.hmm.discrete_approx")
    da.discrete_approx_mvn = None
    da.NotSatisfiableError = type("NotSatisfiableError", (Exception,), {})
    sys.modules["msmbuilder.hmm.discrete_approx"] = da
    msm = types.ModuleType("msmbuilder.msm")
    msm.__path__ = [os.path.join(REF, "msm")]
    sys.modules["msmbuilder.msm"] = msm
    stub = types.ModuleType("msmbuilder.msm._markovstatemodel")

    def _transmat_mle_prinz(C, tol=1e-10):
        T, pi, _ = make_golden_msm.mle_numpy(np.asarray(C))
        return T, pi
    stub._transmat_mle_prinz = _transmat_mle_prinz
    sys.modules["msmbuilder.msm._markovstatemodel"] = stub


def build_extension(tmp):
    """The reference's hmm.gaussian extension, built in tmp; returns the loaded module."""
    hmm = os.path.join(REF, "hmm")
    cpp = os.path.join(tmp, "gaussian.cpp")
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", os.path.join(hmm, "gaussian.pyx"), "-o", cpp])
    so = os.path.join(tmp, "gaussian" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-w", "-DNPY_NO_DEPRECATED_API=0",
                           "-I", sysconfig.get_paths()["include"], "-I", np.get_include(),
                           "-I", os.path.join(hmm, "src", "include"), "-I", os.path.join(hmm, "src"), "-I", tmp, cpp,
                           os.path.join(hmm, "src", "GaussianHMMFitter.cpp"), "-o", so])
    spec = importlib.util.spec_from_file_location("msmbuilder.hmm.gaussian", so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["msmbuilder.hmm.gaussian"] = mod
    spec.loader.exec_module(mod)
    return mod


def mask_time(text):
    return re.sub(r"fit_time: [0-9.]+s", "fit_time: #s", text)


def main():
    warnings.simplefilter("ignore")
    stubs()
    mle = R.mle_solver()
    with tempfile.TemporaryDirectory() as tmp:
        ext = build_extension(tmp)

        class Fixed(ext.GaussianHMM):
            def _init(self, sequences):
                starts = R.golden_starts(2)
                k = getattr(self, "_run", 0)
                self._run = k + 1
                means, vars, transmat, pops = starts[k % len(starts)]
                self.__setstate__((means.copy(), vars.copy(), transmat.copy(), pops.copy(), None, 0.0, means.shape[1]))

        g = {}
        for name, dn, kw, ragged, merged in R.GOLDEN:
            fit, other = R.golden_data(R.DT[dn], ragged=ragged, merged=merged)
            est = Fixed(n_states=3, **dict(dict(n_init=1), **kw)).fit(fit)
            lp, paths = est.predict(other)
            out = {"fit_logprob": np.asarray(est.fit_logprob_), "means": np.asarray(est.means_), "vars": np.asarray(est.vars_),
                   "transmat": np.asarray(est.transmat_), "populations": np.asarray(est.populations_),
                   "timescales": np.asarray(est.timescales_), "score": np.float64(est.score(other)),
                   "predict_logprob": np.float64(lp), "predict_states": np.concatenate(paths).astype(np.int32),
                   "fit_states": np.concatenate(est.predict(fit)[1]).astype(np.int32)}
            (m, v, T, p), logs = R.golden_fit(fit, kw, mle, dt=np.longdouble, form='centred')
            lsp = np.tile(1.0 / 3, 3)
            yard = {"fit_logprob": logs, "means": m, "vars": v, "transmat": T, "populations": p,
                    # (with the RESTATED fit's parameters: the distance is that of the whole fit-then-score pipeline, as for
                    #  the parameters themselves -- an estimator scores with what it fitted)
                    "score": R.estep(other, m, v, T, lsp)["logprob"],
                    "predict_logprob": sum(R.viterbi_optimum(X, m, v, T, lsp) for X in other)}
            for key, val in out.items():
                g[name + "_" + key] = val
            for key, val in yard.items():
                a = np.asarray(out[key], dtype=np.float64)
                b = np.asarray(val, dtype=np.float64)
                assert a.shape == b.shape, (name, key, a.shape, b.shape)
                g[name + "_dist_" + key] = np.float64(np.abs(a - b).max()) if a.size else np.float64(0.0)
            for key, val in R.golden_amplification(fit, other, kw, mle).items():
                g[name + "_amp_" + key] = np.float64(val)
            g[name + "_summarize"] = np.array(mask_time(est.summarize()))
            print(name, "iterations recorded", len(out["fit_logprob"]), "logprob", out["fit_logprob"][-1],
                  "dist", {k: float(g[name + "_dist_" + k]) for k in yard}, "amp", {k: float(g[name + "_amp_" + k]) for k in R.AMP_KEYS})
    np.savez_compressed(os.path.join(HERE, "hmm_golden.npz"), **g)
    print("hmm_golden.npz:", len(g), "arrays")


if __name__ == "__main__":
    main()
