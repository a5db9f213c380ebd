"""The tICA solve on DESIGNED moments (tests/tica_solve_ref.py): the reduction (csrc/eigsolve.hip, the U^-T tiles of
csrc/toppairs.hip), the top-k subspace iteration (csrc/subspace.hip) and the back-solve behind ``msm_tica_reduce``,
``msm_tica_solve_topk`` and ``msm_tica_backsolve``, held to spectra whose answer is known by construction and to what
float64 LAPACK makes of the same stored matrices (the "yardstick").  All solves run with
``MSMBUILDER_AMD_DEVICE_SOLVE=hybrid``; the host route (``=0``) of the same imported state is the second reference.

Bounds (none of them taken from what the device returns):

    eigenvalues    |lambda_dev - lambda_designed| <= 2e-11 + 4 * yardstick      (2e-11: tests/test_gpu_toppairs.py and the
                   solver's own acceptance threshold; yardstick: LAPACK's error on the same pencil)
                   |lambda_dev - lambda_host| <= 2e-11 + 5 * yardstick            (triangle inequality: the host is within one
                   yardstick of the designed values)
    residual       max |OC v - lambda S v| <= (2e-11 + 4 * yardstick) * max |S v|,  evaluated in extended precision
    S-orthonormal  |V^T S V - I| <= 1e-9
    per vector     1e-8 * max |v| / min(gap, 1) up to sign, where both neighbouring gaps of the designed spectrum exceed 1e-4;
                   the number of vectors NOT compared this way is a property of the named spectrum and is asserted
    subspaces      S-projector defect <= 1e-6 for every group of tied vectors and for the whole wanted set
    reduction      |Cs - Cr| <= 8 * max |Cs_host - Cr| + 1e-14 * max |Cr|          (8: the explicit inverse and two GEMMs against
                   LAPACK's two triangular solves -- same order in kappa, larger constant)
    back-solve     |V - V_designed| <= 8 * max |V_host - V_designed| + 1e-14 * max |V_designed|

Measured on an MI355X: max |Cs_dev - Cr| / max |Cs_host - Cr| of ``test_reduce_and_backsolve_directly``
(host = scipy ``cholesky`` + two ``solve_triangular``):

          F  cond(S)   reduce   back-solve, k = 1 / 64 / 65 (capped at F)
          1     1e2     both 0   both 0
          2     1e2     0.65     0.33 / 0.33
         31     1e2     1.19     0.56 / 1.59
         32     1e2     1.05     1.45 / 0.70
         33     1e2     1.36     0.80 / 2.00
         64     1e2     1.29     1.20 / 1.00
         65     1e2     1.55     1.88 / 1.27 / 1.09
        255     1e2     1.40     1.32 / 1.07 / 1.20
        257     1e2     1.18     1.21 / 1.30 / 1.35
      1,023     1e2     1.69     1.21 / 1.39 / 1.21
      1,024     1e2     1.26     1.07 / 1.80 / 1.27
      1,025     1e2     1.31     1.34 / 1.46 / 1.46      (rocSOLVER dpotrf and dtrsm)
        257     1e5     0.85     1.29 / 1.23 / 1.23
        257     1e8     0.77     0.73 / 0.96 / 0.96

The explicit inverse costs no accuracy against two triangular solves, at cond(S) = 1e8 either: every ratio is at most 2 where
the bound allows 8.  Eigenvalues of the same run: within 3e-15 of the designed ones at cond(S) = 1e2 (LAPACK: 3e-15), 4.8e-14
at 1e5 (6.8e-14), 5.2e-11 at 1e8 (4.3e-11).  Routes: every spectrum converged in the iteration (2 rounds; 3 for ``negative``)
except ``wide_cluster`` and ``outside``, which it handed to LAPACK with status 1 at all three sizes.
"""
import re
import warnings

import numpy as np
import pytest

import tica_solve_ref as R

pytestmark = pytest.mark.gpu

SIZES_GAP = [(128, 16), (129, 16), (255, 16), (257, 16), (513, 16), (1023, 16), (1024, 16),      # subspace iteration
             (129, 1), (1024, 1), (513, 10),
             (127, 10), (513, 17), (1025, 10)]                                                   # LAPACK on the reduced matrix
LAPACK_CASES = {(127, 10), (513, 17), (1025, 10)}
OTHER_SPECTRA = [name for name in R.SPECTRA if name != "gap"]
SOLVE_CASES = ([(F, "gap", k, 1e2) for F, k in SIZES_GAP]
               + [(F, name, k, 1e2) for F, k in ((257, 16), (513, 10), (1024, 16)) for name in OTHER_SPECTRA]
               + [(513, "gap", 10, 1e5), (513, "gap", 10, 1e8)])


def _model(monkeypatch, state, route, **over):
    from msmbuilder_amd import tICA
    monkeypatch.setenv("MSMBUILDER_AMD_TICA_MODE", "f64")
    monkeypatch.setenv("MSMBUILDER_AMD_DEVICE_SOLVE", route)
    return tICA.from_reference_state(dict(state, **over) if over else state)


def _solved(m):
    """(eigenvalues, eigenvectors as columns, route) of a model; the environment must still name the route."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vals, vecs = m.eigenvalues_.copy(), m.eigenvectors_.copy()
    return vals, vecs, getattr(m, "_solve_route", None)


def _tied_groups(lam, k):
    """Maximal runs of indices < k whose consecutive designed eigenvalues are at most GAP_MIN apart."""
    groups, run = [], [0]
    for j in range(1, k):
        if lam[j - 1] - lam[j] <= R.GAP_MIN:
            run.append(j)
        else:
            groups.append(run)
            run = [j]
    groups.append(run)
    return [g for g in groups if len(g) > 1]


def _check_designed(d, yard, k, exempt, name, vals, V, what):
    """Every assertion of the module docstring against the designed truth."""
    lam, S, OC, Vd = d["lam"], d["S"], d["OC"], d["V"]
    top = d["order"][:k]
    assert np.array_equal(top, np.arange(k))                       # spectra come in descending order
    bound = 2e-11 + 4 * yard["eig"]
    err = np.abs(vals - lam[:k])
    print("%s: max eigenvalue error %.3e (yardstick %.3e, bound %.3e)" % (what, err.max(), yard["eig"], bound))
    assert (err <= bound).all(), (what, err, bound)
    worst = 0.0
    for j in range(k):
        res, sv = R.pencil_residual(OC, S, V[:, j], vals[j])
        worst = max(worst, res / sv)
        assert res <= bound * sv, (what, j, res, sv, bound)
    gram = np.abs(V.T.dot(S).dot(V) - np.eye(k)).max()
    print("%s: max residual / max|Sv| %.3e, S-orthonormality defect %.3e" % (what, worst, gram))
    assert gram <= 1e-9, (what, gram)
    # per-vector agreement where the designed vector is determined; how many are not is the spectrum's property
    loose = [j for j in range(k) if R.neighbour_gap(lam, j) <= R.GAP_MIN]
    assert len(loose) == exempt, (what, loose, exempt)
    for j in range(k):
        if j in loose:
            continue
        g = min(R.neighbour_gap(lam, j), 1.0)
        sg = np.sign(V[:, j].dot(S).dot(Vd[:, j]))
        np.testing.assert_allclose(V[:, j] * sg, Vd[:, j], rtol=0, atol=1e-8 * np.abs(Vd[:, j]).max() / g, err_msg="%s vector %d" % (what, j))
    # tied vectors as subspaces; a tie across the cut leaves the k-th vector anywhere in the tied plane
    cut_tie = lam[k - 1] - lam[k] <= R.GAP_MIN if k < len(lam) else False
    for grp in _tied_groups(lam, k):
        if cut_tie and grp[-1] == k - 1:
            continue
        assert R.s_projector_defect(V[:, grp], S, Vd[:, grp]) <= 1e-6, (what, grp)
    if cut_tie:
        assert name == "edge_tie"
        assert R.s_projector_defect(V[:, :k - 1], S, Vd[:, :k - 1]) <= 1e-6, what
        plane = [j for j in range(len(lam)) if abs(lam[j] - lam[k - 1]) <= R.GAP_MIN]
        c = Vd[:, plane].T.dot(S).dot(V[:, k - 1])
        assert abs(c.dot(c) - 1.0) <= 1e-6, (what, c)
    else:
        assert R.s_projector_defect(V, S, Vd[:, :k]) <= 1e-6, what


def _check_against_host(vals, V, hvals, hV, S, k, yard_eig, what):
    """Device pairs against the host route's; ``hvals`` / ``hV`` carry k + 1 pairs so that the k-th gap is known."""
    bound = 2e-11 + 5 * yard_eig
    err = np.abs(vals - hvals[:k])
    print("%s: max |lambda_dev - lambda_host| %.3e (bound %.3e)" % (what, err.max(), bound))
    assert (err <= bound).all(), (what, err, bound)
    assert np.abs(V.T.dot(S).dot(V) - np.eye(k)).max() <= 1e-9, what
    for j in range(k):
        g = R.neighbour_gap(hvals, j)
        if g > R.GAP_MIN:
            sg = np.sign(V[:, j].dot(S).dot(hV[:, j]))
            np.testing.assert_allclose(V[:, j] * sg, hV[:, j], rtol=0, atol=1e-8 * np.abs(hV[:, j]).max() / min(g, 1.0),
                                       err_msg="%s vector %d" % (what, j))


def _check_route(F, name, k, route, what):
    print("%s: route %r" % (what, route))
    if (F, k) in LAPACK_CASES:
        assert route[0] == "lapack" and route[2] != 2, route
    elif name == "gap" and F >= 256:
        assert route[0] == "subspace" and route[2] == 0, route
    else:   # the iteration may hand over (status 1); a failed verification (status 2) is not accepted
        assert (route[0] == "subspace" and route[2] == 0) or (route[0] == "lapack" and route[2] == 1), route


@pytest.mark.parametrize("F,name,k,kappa", SOLVE_CASES, ids=lambda v: str(v))
def test_solve_on_designed_spectrum(gpu, monkeypatch, F, name, k, kappa):
    d, yard, k, exempt = R.case(F, name, k, kappa)
    what = "F=%d %s k=%d kappa=%g" % (F, name, k, kappa)
    m = _model(monkeypatch, d["state"], "hybrid")
    vals, V, route = _solved(m)
    assert vals.shape == (k,) and V.shape == (F, k)
    _check_route(F, name, k, route, what)
    _check_designed(d, yard, k, exempt, name, vals, V, what)
    assert np.array_equal(m.means_, np.zeros(F))
    # the host route on the same imported state
    h = _model(monkeypatch, d["state"], "0", n_components=min(k + 1, F))
    hvals, hV, _ = _solved(h)
    if name in ("double", "edge_tie"):      # ties: eigenvalues only, the subspaces were held to the designed ones above
        assert (np.abs(vals - hvals[:k]) <= 2e-11 + 5 * yard["eig"]).all(), what
    else:
        _check_against_host(vals, V, hvals, hV, d["S"], k, yard["eig"], what)


REDUCE_CASES = [(F, 1e2) for F in (1, 2, 31, 32, 33, 64, 65, 255, 257, 1023, 1024, 1025)] + [(257, 1e5), (257, 1e8)]


@pytest.mark.parametrize("F,kappa", REDUCE_CASES, ids=lambda v: str(v))
def test_reduce_and_backsolve_directly(gpu, monkeypatch, F, kappa):
    """``msm_tica_reduce`` returns the designed reduced matrix and a zero mean; ``msm_tica_backsolve`` maps designed rows of
    W^T to the matching rows of V^T on both sides of its k <= 64 split (and, at F = 1,025, of its F <= 1,024 split)."""
    d, yard, _, _ = R.case(F, "gap", min(10, F), kappa)
    m = _model(monkeypatch, d["state"], "hybrid")
    L = gpu.lib()
    Cs, mu, info = np.empty((F, F)), np.full(F, np.nan), np.zeros(12)
    gpu.check(L.msm_tica_reduce(m._handle, 0.0, int(m.n_observations_), None, Cs.ctypes.data, mu.ctypes.data, info.ctypes.data))
    assert info[0] == 0.0 and info[2] == 0 and info[4] == 0 and info[5] == 0
    assert np.array_equal(mu, np.zeros(F))
    Cr = d["Cr"]
    err, bound = np.abs(Cs - Cr).max(), 8 * yard["Cr"] + 1e-14 * np.abs(Cr).max()
    print("reduce F=%d kappa=%g: device %.3e host %.3e ratio %.2f bound %.3e" % (F, kappa, err, yard["Cr"], err / yard["Cr"] if yard["Cr"] else np.inf, bound))
    np.testing.assert_allclose(Cs, Cs.T, rtol=0, atol=2 * bound)      # symmetric up to rounding
    failed = [] if err <= bound else ["reduce: %.3e > %.3e" % (err, bound)]
    for k in sorted({min(kk, F) for kk in (1, 64, 65)}):
        rows = d["order"][:k]
        Y = np.ascontiguousarray(d["W"][:, rows].T)
        V = np.full((k, F), np.nan)
        gpu.check(L.msm_tica_backsolve(m._handle, Y.ctypes.data, k, V.ctypes.data))
        want = d["V"][:, rows].T
        yb = R.back_error(d, yard["U"], rows)
        err, bound = np.abs(V - want).max(), 8 * yb + 1e-14 * np.abs(want).max()
        print("backsolve F=%d kappa=%g k=%d: device %.3e host %.3e ratio %.2f bound %.3e" % (F, kappa, k, err, yb, err / yb if yb else np.inf, bound))
        if not err <= bound:
            failed.append("backsolve k=%d: %.3e > %.3e" % (k, err, bound))
    assert not failed, failed


def _host_pairs(monkeypatch, state, k, scale=None):
    h = _model(monkeypatch, state, "0", n_components=k + 1)
    if scale is not None:
        h.set_input_scaling(scale=scale)
    hvals, hV, _ = _solved(h)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return hvals, hV, h.covariance_.copy(), h.shrinkage_


def test_estimated_shrinkage_on_the_device_route(gpu, monkeypatch):
    """shrinkage=None: the Rao-Blackwell Ledoit-Wolf intensity of the designed S, then the host route's eigenpairs."""
    from msmbuilder_amd.decomposition import _moments
    d, yard, k, _ = R.case(513, "gap", 10)
    m = _model(monkeypatch, d["state"], "hybrid", shrinkage=None)
    vals, V, route = _solved(m)
    assert route[0] == "subspace" and route[2] == 0, route
    want = _moments.rblw_shrinkage(d["S"], n=R.N_OBSERVATIONS)
    assert 0.0 < want < 1.0
    np.testing.assert_allclose(m.shrinkage_, want, rtol=1e-12)
    hvals, hV, cov, hrho = _host_pairs(monkeypatch, dict(d["state"], shrinkage=None), k)
    np.testing.assert_allclose(hrho, want, rtol=1e-12)
    _check_against_host(vals, V, hvals, hV, cov, k, yard["eig"], "shrinkage=None")


def test_designed_mean_of_order_one(gpu, monkeypatch):
    d, yard, k, exempt = R.case(513, "gap", 10, 1e2, None, 1.0)
    assert 1.0 < np.abs(d["mean"]).max() < 10.0
    m = _model(monkeypatch, d["state"], "hybrid")
    vals, V, route = _solved(m)
    assert route[0] == "subspace" and route[2] == 0, route
    assert np.array_equal(m.means_, d["mean"])
    _check_designed(d, yard, k, exempt, "gap", vals, V, "mean of order 1")
    hvals, hV, cov, _ = _host_pairs(monkeypatch, d["state"], k)
    _check_against_host(vals, V, hvals, hV, cov, k, yard["eig"], "mean of order 1")
    # the reduction entry returns the same mean
    monkeypatch.setenv("MSMBUILDER_AMD_DEVICE_SOLVE", "hybrid")
    Cs, mu = np.empty((513, 513)), np.empty(513)
    gpu.check(gpu.lib().msm_tica_reduce(m._handle, 0.0, int(m.n_observations_), None, Cs.ctypes.data, mu.ctypes.data, None))
    assert np.array_equal(mu, d["mean"])
    assert np.abs(Cs - d["Cr"]).max() <= 8 * yard["Cr"] + 1e-14 * np.abs(d["Cr"]).max()


def test_input_scaling_on_the_device_route(gpu, monkeypatch):
    d, yard, k, _ = R.case(513, "gap", 10)
    scale = np.random.RandomState(5).uniform(0.5, 2.0, 513)
    m = _model(monkeypatch, d["state"], "hybrid")
    m.set_input_scaling(scale=scale)
    vals, V, route = _solved(m)
    assert route[0] == "subspace" and route[2] == 0, route
    hvals, hV, cov, _ = _host_pairs(monkeypatch, d["state"], k, scale=scale)
    _check_against_host(vals, V, hvals, hV, cov, k, yard["eig"], "input scaling")
    # the scaled pencil is D OC D, D S D: its eigenvalues are the designed ones, its vectors D^-1 V
    assert (np.abs(vals - d["lam"][:k]) <= 2e-11 + 4 * yard["eig"]).all()
    assert R.s_projector_defect(V / scale[:, None], d["S"], d["V"][:, :k]) <= 1e-6


@pytest.mark.parametrize("k", [10, 17])
@pytest.mark.parametrize("F,p", [(130, 0), (130, 31), (130, 32), (130, 70), (130, 129), (1025, 600)])
def test_not_positive_definite_is_reported_with_its_minor(gpu, monkeypatch, F, p, k):
    """S[p, p] < 0 through the path tICA takes (U^-T tiles present): LAPACK's report, from the top-k entry (k = 10) and the
    reduction entry (k = 17; F = 1,025 takes it for either k, with rocSOLVER's factorisation)."""
    d = R.case(F, "gap", 10)[0]
    m = _model(monkeypatch, R.not_positive_definite(d, p), "hybrid", n_components=k)
    with pytest.raises(np.linalg.LinAlgError) as e:
        _solved(m)
    assert re.search(r"(?i)leading minor of order %d of" % (p + 1), str(e.value)), str(e.value)
    # the handle is usable afterwards: the intact state solves
    vals, _, _ = _solved(_model(monkeypatch, d["state"], "hybrid", n_components=k))
    assert (np.abs(vals[:10] - d["lam"][:10]) <= 2e-11 + 4 * R.case(F, "gap", 10)[1]["eig"]).all()
