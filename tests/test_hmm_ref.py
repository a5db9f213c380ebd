"""CPU tier of the Gaussian HMM: the numpy restatement (tests/hmm_ref.py) against the reference's goldens
(tests/golden/hmm_golden.npz, made by tests/golden/make_golden_hmm.py from the reference's own extension), and the
rounding bound the GPU tier holds the device to against what the reference's arithmetic itself achieves.

* the float64 restatement in the reference's arithmetic reproduces every golden quantity to a few ulps of its scale;
* the longdouble restatement agrees with the goldens under the bound plus the recorded distance;
* Viterbi paths are the goldens' state for state;
* on every case of the GPU tier the float64 restatement of the reference's arithmetic lies within the bound of the
  longdouble one (the bound is no tighter than what the reference achieves), and the bound stays below sqrt(2^-53)
  relative to each quantity's scale (one float32 intermediate anywhere fails it).
"""
import os

import numpy as np
import pytest

import hmm_ref as R
from msmbuilder_amd.hmm import gaussian   # (msm_hmm_plan; the estimator itself runs on the GPU tier)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmm_golden.npz")
EPS = np.finfo(np.float64).eps
try:
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hmm_bounds.txt")) as _fh:
        BOUNDS_PROFILE = _fh.read()
except FileNotFoundError:   # (scripts/hmm_probe.py --bounds writes it from this module's cases)
    BOUNDS_PROFILE = ""


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mle():
    return R.mle_solver()


@pytest.mark.parametrize("name,dn,kw,ragged,merged", R.GOLDEN, ids=[c[0] for c in R.GOLDEN])
def test_float64_restatement_is_the_reference(golden, mle, name, dn, kw, ragged, merged):
    g = golden
    fit, other = R.golden_data(R.DT[dn], ragged=ragged, merged=merged)
    (means, vars, T, pops), logs = R.golden_fit(fit, kw, mle)
    assert len(logs) == len(g[name + "_fit_logprob"])
    N = sum(len(X) for X in fit)
    # the same arithmetic in the same order up to the sums over trajectories and frames: a few ulps of each quantity's
    # scale per frame summed
    ulps = 8 * N * EPS
    for key, val in (('fit_logprob', logs), ('means', means), ('vars', vars), ('transmat', T), ('populations', pops)):
        ref = g[name + "_" + key]
        assert np.abs(val - ref).max() <= ulps * max(np.abs(ref).max(), 1.0) * len(logs), key
    lsp = np.tile(1 / 3.0, 3)
    p = (g[name + "_means"], g[name + "_vars"], g[name + "_transmat"], lsp)
    sc = float(R.estep(other, *p, dt=np.float64, form='expanded')['logprob'])
    assert abs(sc - float(g[name + "_score"])) <= 8 * EPS * abs(sc) * 10
    lp, paths = 0.0, []
    for X in other:
        a, b = R.viterbi(X, *p)
        lp += float(a)
        paths.append(b)
    assert np.array_equal(np.concatenate(paths), g[name + "_predict_states"])
    assert abs(lp - float(g[name + "_predict_logprob"])) <= 8 * EPS * abs(lp) * 10
    assert np.array_equal(np.concatenate([R.viterbi(X, *p)[1] for X in fit]), g[name + "_fit_states"])


@pytest.mark.parametrize("name,dn,kw,ragged,merged", R.GOLDEN, ids=[c[0] for c in R.GOLDEN])
def test_longdouble_restatement_under_the_bound(golden, name, dn, kw, ragged, merged):
    g = golden
    fit, other = R.golden_data(R.DT[dn], ragged=ragged, merged=merged)
    lsp = np.tile(1 / 3.0, 3)
    p = (g[name + "_means"], g[name + "_vars"], g[name + "_transmat"], lsp)
    for data in (fit, other):
        b = R.bound(data, *p)
        assert b['rel'] < R.SQRT_U
        yard = R.estep(data, *p)
        ref = R.estep(data, *p, dt=np.float64, form='expanded')
        R.check_stats(ref, yard, b, who=name)
    bo = R.bound(other, *p)
    sc = R.estep(other, *p)['logprob']
    assert abs(float(sc) - float(g[name + "_score"])) <= bo['logprob'].sum() + float(g[name + "_dist_score"])
    best = sum(R.viterbi_optimum(X, *p) for X in other)
    assert abs(float(best) - float(g[name + "_predict_logprob"])) <= bo['logprob'].sum() + float(g[name + "_dist_predict_logprob"])
    # the goldens' paths are optimal: re-evaluated in longdouble they reach the optimum
    o = 0
    for X in other:
        path = g[name + "_predict_states"][o:o + len(X)]
        o += len(X)
        i = [len(Y) for Y in other].index(len(X))
        assert abs(R.path_logprob(X, path, *p) - R.viterbi_optimum(X, *p)) <= bo['logprob'][i]


def gpu_tier_cases():
    """Every generated case of tests/test_gpu_hmm.py, from the same generators over the same plan (msm_hmm_plan needs no
    device), and the hard inputs."""
    out = []
    for shape in R.generated_shapes(gaussian.plan):
        for dn in ('f32', 'f64'):
            out.append((R.shape_name(*shape, dn),) + R.generated_case(*shape, dn))
    for name, (seqs, means, vars, A, lsp) in R.hard_cases().items():
        out.append((name, seqs, (means, vars, A, lsp)))
    return out


CASES = gpu_tier_cases()


@pytest.mark.parametrize("name,seqs,mdl", CASES, ids=[c[0] for c in CASES])
def test_bound_is_what_the_reference_achieves_and_below_sqrt_u(name, seqs, mdl):
    b = R.bound(seqs, *mdl)
    # below sqrt(u) relative to each quantity's scale
    assert b['rel'] < R.SQRT_U, (b['rel'], R.SQRT_U)
    yard = R.estep(seqs, *mdl)
    assert np.all(b['logprob'] < R.SQRT_U * np.maximum(np.abs(np.asarray(yard['traj_logprob'], dtype=np.float64)), 1.0))
    # no tighter than what the reference's own arithmetic achieves
    ref = R.estep(seqs, *mdl, dt=np.float64, form='expanded')
    R.check_stats(ref, yard, b, who=name)
    # the profile lists this very bound
    assert R.bounds_line(name, b) in BOUNDS_PROFILE.split("\n"), name


def test_bound_is_linear_in_length_and_states():
    T, K, F, E = 385, 17, 5, 80.0
    base = R.rho_of(T, K, F, E)
    assert abs(R.rho_of(2 * T, K, F, E) / base - 2.0) < 1e-12
    assert abs(R.rho_of(3 * T, K, F, E) / base - 3.0) < 1e-12
    step = R.rho_of(T, K + 1, F, E) - base
    assert step > 0
    for more in (2, 10, 47):   # equal steps in K: affine-linear
        assert abs((R.rho_of(T, K + more, F, E) - base) / (more * step) - 1.0) < 1e-9
    mdl = R.model(3, 3, 0)
    seqs = R.sequences(mdl[0], mdl[1], mdl[2], [1, 2, 7, 8, 9, 25], 1)
    b = R.bound(seqs, *mdl)
    assert b['rho'] == R.rho_of(b['T'], b['K'], b['F'], b['E'])
    twice = R.bound([np.concatenate([X, X]) for X in seqs], *mdl)
    assert abs(twice['rho'] / b['rho'] - 2.0) < 1e-12


def test_bound_catches_a_float32_intermediate():
    mdl = R.model(3, 3, 0)
    seqs = R.sequences(mdl[0], mdl[1], mdl[2], [1, 2, 7, 8, 9, 25], 1)
    b = R.bound(seqs, *mdl)
    yard = R.estep(seqs, *mdl)
    spoiled = dict(yard)
    spoiled['post'] = np.asarray(yard['post'], dtype=np.float64).astype(np.float32).astype(np.float64)
    with pytest.raises(AssertionError):
        R.check_stats(spoiled, yard, b)


def test_first_maximum_rules():
    means = np.array([[0.0], [0.0], [5.0]])
    vars = np.ones((3, 1))
    A = np.array([[0.45, 0.45, 0.1], [0.45, 0.45, 0.1], [0.1, 0.1, 0.8]])
    X = np.array([[0.1], [5.2], [0.0], [-0.3]])
    lp, s = R.viterbi(X, means, vars, A, np.tile(1 / 3.0, 3))
    assert s.tolist() == [0, 2, 0, 0]


def test_bounds_profile_has_no_other_lines():
    """profiles/hmm_bounds.txt is the bound at the test shapes and nothing else (every case checks its own line)."""
    names = {c[0] for c in CASES}
    listed = [line.split()[0] for line in BOUNDS_PROFILE.split("\n")[3:] if line.strip()]
    assert sorted(listed) == sorted(names)
