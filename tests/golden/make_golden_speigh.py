#!/usr/bin/env python
"""tests/golden/make_golden_speigh.py -- speigh_golden.npz: the reference's sparse eigenpair solver and SparseTICA.

Runs only where the reference tree is present.  The reference's compiled solver (decomposition/_speigh.pyx) is built in a
temporary directory OUTSIDE this repository (cython at language level 2 -- its cy_blas.pyx divides integers with `/` --,
then gcc -O2 -shared), its python files are imported by file path, and only OUTPUTS are stored: the inputs are
regenerated from seeds by tests/speigh_ref.py.

A case enters the goldens only if the reference, the float64 restatement, the longdouble restatement and two runs of the
float64 restatement with permuted features (a reordered summation) all give the SAME mask and the SAME outer-step count;
the script refuses to write when more than one case in ten of a family fails that.

Usage:  python tests/golden/make_golden_speigh.py [output.npz]
"""
import contextlib
import importlib.util
import io
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types
import warnings

import numpy as np
import scipy.linalg

REF = "/root/reference/msmbuilder"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import speigh_ref as R  # noqa: E402

EPS, TOL, MAXITER = 1e-6, 1e-6, 10000            # SparseTICA's defaults
SIZES = (1, 2, 3, 12, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 513)
RHOS = (1e-4, 1e-3, 1e-2, 1e-1)
STORED_EIGH = (12, 33, 65, 129, 200)             # sizes whose (w, V) are stored for the project / solve_admm cases
ADMM_CASES = ((1e-2, 1.0), (1e-1, 1.0), (1e-2, 10.0))   # (rho, scale of b): the scaled case doubles the penalty at F = 12


def _load(name, path, package=None):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def build_extension(tmp):
    src = os.path.join(REF, "decomposition", "_speigh.pyx")
    c = os.path.join(tmp, "_speigh.c")
    inc = os.path.join(REF, "src")
    subprocess.check_call([sys.executable, "-m", "cython", "-2", "-I", inc, "-o", c, src])
    so = os.path.join(tmp, "_speigh" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-I", sysconfig.get_paths()["include"], "-I", np.get_include(),
                           "-I", inc, c, "-o", so])
    spec = importlib.util.spec_from_file_location("msmbuilder.decomposition._speigh", so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["msmbuilder.decomposition._speigh"] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(tmp):
    md = types.ModuleType("mdtraj")
    md.Trajectory = type("Trajectory", (object,), {})
    sys.modules["mdtraj"] = md
    _eigh = scipy.linalg.eigh

    def eigh_compat(a, b=None, eigvals=None, **kw):
        if eigvals is not None:
            kw["subset_by_index"] = list(eigvals)
        return _eigh(a, b=b, **kw)
    scipy.linalg.eigh = eigh_compat

    pkg = types.ModuleType("msmbuilder")
    pkg.__path__ = [REF]
    sys.modules["msmbuilder"] = pkg
    _load("msmbuilder.base", os.path.join(REF, "base.py"), "msmbuilder")
    utils = types.ModuleType("msmbuilder.utils")
    utils.__path__ = [os.path.join(REF, "utils")]
    sys.modules["msmbuilder.utils"] = utils
    val = _load("msmbuilder.utils.validation", os.path.join(REF, "utils", "validation.py"), "msmbuilder.utils")
    utils.check_iter_of_sequences = val.check_iter_of_sequences
    utils.array2d = val.array2d
    utils.experimental = lambda *a, **k: (lambda f: f)
    dec = types.ModuleType("msmbuilder.decomposition")
    dec.__path__ = [os.path.join(REF, "decomposition")]
    sys.modules["msmbuilder.decomposition"] = dec
    _load("msmbuilder.decomposition.tica", os.path.join(REF, "decomposition", "tica.py"), "msmbuilder.decomposition")
    ext = build_extension(tmp)
    sp = _load("msmbuilder.decomposition.sparsetica", os.path.join(REF, "decomposition", "sparsetica.py"), "msmbuilder.decomposition")
    return ext, sp.SparseTICA


def reference_speigh(ext, A, B, rho):
    """(u, v, outer steps): the solver prints one objective line per pass of its outer loop when verbose."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        u, v = ext.speigh(np.ascontiguousarray(A), np.ascontiguousarray(B), rho, eps=EPS, tol=TOL, maxiter=MAXITER, verbose=1)
    passes = sum(1 for line in buf.getvalue().splitlines() if line.startswith("QCQP objective"))
    return float(u), np.asarray(v), passes - 1       # the last pass is the one that met the stop rule


def qualifies(ext, A, B, rho, F, seed):
    u_ref, v_ref, outer_ref = reference_speigh(ext, A, B, rho)
    mask_ref = np.abs(v_ref) > 0
    u64, v64, i64 = R.speigh(A, B, rho, EPS, TOL, MAXITER)
    runs = [("float64", i64['mask'], i64['outer'])]
    _, _, ild = R.speigh(A, B, rho, EPS, TOL, MAXITER, dtype=np.longdouble)
    runs.append(("longdouble", ild['mask'], ild['outer']))
    for p in range(2):
        perm = np.random.RandomState(7919 * seed + p).permutation(F)
        _, _, ip = R.speigh(A[np.ix_(perm, perm)], B[np.ix_(perm, perm)], rho, EPS, TOL, MAXITER)
        back = np.empty(F, bool)
        back[perm] = ip['mask']
        runs.append(("permuted %d" % p, back, ip['outer']))
    ok = all(np.array_equal(m, mask_ref) and o == outer_ref for _, m, o in runs) and i64['status'] == 'converged'
    if not ok:
        print("  F=%d rho=%g does not qualify: reference (%d nonzeros, %d steps) vs %s" % (
            F, rho, mask_ref.sum(), outer_ref, [(n, int(m.sum()), o) for n, m, o in runs]))
    return ok, u_ref, v_ref, mask_ref, outer_ref, i64


def main():
    warnings.simplefilter("ignore")
    tmp = tempfile.mkdtemp(prefix="speigh_ref_")
    assert not os.path.abspath(tmp).startswith(os.path.dirname(os.path.dirname(HERE)) + os.sep)
    try:
        ext, SparseTICA = load_reference(tmp)
        out = {"sizes": np.array(SIZES), "rhos": np.array(RHOS), "eps_tol_maxiter": np.array([EPS, TOL, MAXITER])}
        qualified = []
        dropped = 0
        for F in SIZES:
            seed = F
            A, B = R.matrices(F, seed)
            for ri, rho in enumerate(RHOS):
                ok, u, v, mask, outer, i64 = qualifies(ext, A, B, rho, F, seed)
                if not ok:
                    dropped += 1
                    continue
                key = "pair_F%d_r%d_" % (F, ri)
                qualified.append((F, ri))
                out[key + "u"] = np.float64(u)
                out[key + "v"] = v
                out[key + "mask"] = mask
                out[key + "outer"] = np.int64(outer)
                out[key + "admm"] = np.int64(i64['admm'])
                print("F=%-4d rho=%-7g nnz=%-4d outer=%-4d admm=%-6d doubled=%d halved=%d u=%.6f" % (
                    F, rho, mask.sum(), outer, i64['admm'], i64['doubled'], i64['halved'], u))
        total = len(SIZES) * len(RHOS)
        assert dropped * 10 <= total, "%d of %d cases failed the qualifying condition" % (dropped, total)
        out["qualified"] = np.array(qualified, dtype=np.int64)

        # project / solve_admm on stored (w, V): the first outer step of the pair
        doubled = halved = 0
        for F in STORED_EIGH:
            A, B = R.matrices(F, F)
            w, V = scipy.linalg.eigh(B)
            key = "eig_F%d_" % F
            out[key + "w"], out[key + "V"] = w, V
            rs = np.random.RandomState(1000 + F)
            a = rs.randn(F) * 4.0 / np.sqrt(np.sort(w)[F // 2])      # far outside the ellipsoid
            got = np.empty(F)
            ext.project(a, np.ascontiguousarray(w), np.ascontiguousarray(V), got)
            want = R.project(a, w, V, np.longdouble)
            out[key + "proj_a"], out[key + "proj_ref"] = a, got
            out[key + "dist_project"] = np.float64(np.max(np.abs(got - want)))
            for ci, (rho, scale) in enumerate(ADMM_CASES):
                x0 = R.top_pair(A, B)[1]
                rho_e = rho / np.log1p(1 / EPS)
                tau = 0.1 + max(0.0, -scipy.linalg.eigvalsh(A).min())
                b = scale * (A.dot(x0) / tau + x0)
                ww = rho_e / (2 * tau * (np.abs(x0) + EPS))
                x = x0.copy()
                ext.solve_admm(b, ww, np.ascontiguousarray(w), np.ascontiguousarray(V), x, tol=TOL, maxiter=MAXITER)
                x64, inf64 = R.solve_admm(b, ww, w, V, x0, TOL, MAXITER)
                xld, _ = R.solve_admm(b, ww, w, V, x0, TOL / 1000, MAXITER, np.longdouble)
                assert np.array_equal(x != 0, x64 != 0) and np.array_equal(x != 0, xld != 0), "ADMM zero patterns differ at F=%d" % F
                k2 = key + "admm%d_" % ci
                out[k2 + "b"], out[k2 + "w"], out[k2 + "x0"], out[k2 + "x_ref"] = b, ww, x0, x
                out[k2 + "dist_admm"] = np.float64(np.max(np.abs(x - np.asarray(xld, np.float64))))
                out[k2 + "iterations"] = np.int64(inf64['iterations'])
                out[k2 + "doubled"], out[k2 + "halved"] = np.int64(inf64['doubled']), np.int64(inf64['halved'])
                doubled += inf64['doubled']
                halved += inf64['halved']
                print("admm F=%d rho=%g scale=%g: %d iterations, doubled %d, halved %d, dist %.2e" % (
                    F, rho, scale, inf64['iterations'], inf64['doubled'], inf64['halved'], out[k2 + "dist_admm"]))
        assert doubled > 0 and halved > 0, "the ADMM cases must adapt the penalty in both directions (%d, %d)" % (doubled, halved)

        # SparseTICA on float64 rows
        cases = []
        for F in (12, 33):
            X = R.rows(F, F)
            seqs = [X[:len(X) // 2], X[len(X) // 2:]]
            held = R.rows(F, F + 1000)[:200]
            for k in (1, 3):
                for ri, rho in enumerate((1e-3, 1e-2)):
                    for shrink in (0, None):
                        kinetic = (F == 12 and k == 3 and ri == 0 and shrink is None)
                        m = SparseTICA(n_components=k, lag_time=R.LAG, rho=rho, shrinkage=shrink, kinetic_mapping=kinetic)
                        m.fit(seqs)
                        key = "stica_F%d_k%d_r%d_s%s_" % (F, k, ri, "none" if shrink is None else "0")
                        out[key + "eigenvalues"] = np.array(m.eigenvalues_)
                        out[key + "components"] = np.array(m.components_)
                        out[key + "timescales"] = np.array(m.timescales_)
                        out[key + "transform"] = np.array(m.transform([held])[0])
                        out[key + "summary"] = np.array(m.summarize())
                        out[key + "kinetic"] = np.bool_(kinetic)
                        cases.append(key)
        out["stica_cases"] = np.array(cases)
        np.savez_compressed(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "speigh_golden.npz"), **out)
        print("wrote speigh_golden.npz: %d pair cases (%d dropped), %d SparseTICA cases" % (len(qualified), dropped, len(cases)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
