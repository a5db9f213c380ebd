"""CPU tier of the von Mises HMM: the numpy restatement (tests/vmhmm_ref.py) against the reference's goldens
(tests/golden/vmhmm_golden.npz, made by tests/golden/make_golden_vmhmm.py from the reference's own extension), the
M-step of the estimator, and the rounding bound the GPU tier holds the device to.

* the longdouble restatement of every golden fit lies within the recorded ``dist`` of the golden, and the float64
  restatement in the reference's arithmetic (the split form) reproduces the float64 goldens to a few ulps per frame;
* the estimator's ``A^-1`` (spline) inverts ``A`` within the spline's own error, clips at both ends, and survives states
  without posterior weight; its M-step is the restatement's;
* ``overlap_`` against the golden;
* the split form lies within the bound of the direct form on every case of the GPU tier;
* the Viterbi cases of the GPU tier have decision margins above the bound.
"""
import os

import numpy as np
import pytest

import vmhmm_ref as V
from msmbuilder_amd.hmm import gaussian, vonmises   # (msm_hmm_plan and the host M-step; the device runs on the GPU tier)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vmhmm_golden.npz")
EPS = np.finfo(np.float64).eps
IDS = [c[0] for c in V.GOLDEN]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mle():
    return V.H.mle_solver()


def finite_close(got, ref, tol):
    """|got - ref| <= tol where the reference is finite (its overlap_ overflows where a concentration is above ~355)."""
    ok = np.isfinite(ref)
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64)[ok] - ref[ok]) <= tol))


@pytest.mark.parametrize("name,dn,kw,ragged,tight", V.GOLDEN, ids=IDS)
def test_longdouble_restatement_within_dist(golden, mle, name, dn, kw, ragged, tight):
    g = golden
    fit, other = V.golden_data(V.DT[dn], ragged=ragged, tight=tight)
    (m, k, T, p), logs = V.golden_fit(fit, kw, mle, dt=np.longdouble, form='direct')
    assert len(logs) == len(g[name + "_fit_logprob"])
    lsp = np.tile(1 / 3.0, 3)
    yard = {"fit_logprob": logs, "means": m, "kappas": k, "transmat": T, "populations": p,
            "overlap": V.overlap(m, k, in_place=True),
            "score": V.estep(other, m, k, T, lsp)["logprob"],
            "predict_logprob": sum(V.viterbi(X, m, k, T, lsp)[0] for X in other)}
    for key, val in yard.items():
        ref = np.asarray(g[name + "_" + key], dtype=np.float64)
        dist = float(g[name + "_dist_" + key])
        # (the distance was recorded from this very computation: a few ulps of the quantity for a different libm)
        assert finite_close(np.asarray(val, dtype=np.float64), ref, dist + 64 * EPS * max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))), key
    paths = np.concatenate([V.viterbi(X, g[name + "_means"], g[name + "_kappas"], g[name + "_transmat"], lsp)[1] for X in other])
    assert np.array_equal(paths, g[name + "_predict_states"])


@pytest.mark.parametrize("name,dn,kw,ragged,tight", [c for c in V.GOLDEN if c[1] == 'f64'], ids=[i for i in IDS if i.endswith('f64')])
def test_float64_split_restatement_is_the_reference(golden, mle, name, dn, kw, ragged, tight):
    g = golden
    fit, other = V.golden_data(V.DT[dn], ragged=ragged, tight=tight)
    (m, k, T, p), logs = V.golden_fit(fit, kw, mle)
    assert len(logs) == len(g[name + "_fit_logprob"])
    N = sum(len(X) for X in fit)
    # the same arithmetic up to the order of the sums over frames and the Bessel routine: a few ulps of each quantity's
    # scale per frame summed, carried through the recorded amplification of the sums into the quantity
    for key, val in (('fit_logprob', logs), ('means', m), ('kappas', k), ('transmat', T), ('populations', p)):
        ref = g[name + "_" + key]
        assert np.abs(val - ref).max() <= 8 * N * EPS * max(float(g[name + "_amp_" + key]), np.abs(ref).max(), 1.0) * len(logs), key


# ---- M-step ------------------------------------------------------------------------------------------------------
def test_inverse_bessel_ratio_inverts_within_the_splines_error():
    inv = vonmises.inverse_bessel_ratio
    ref = V.spline_inverse()
    nodes = ref.x
    mid = np.sqrt(nodes[:-1] * nodes[1:])
    for x in (nodes, mid):
        y = V.bessel_ratio(x)
        got = inv(y)
        # the spline's own error: the restated spline against A^-1 by bisection, doubled, plus the rounding of y (A^-1 is
        # ill-conditioned where A saturates: dx / x = dy / (x A'(x)), and y carries an ulp)
        exact = V.bessel_ratio_inverse_exact(y)
        own = np.abs(ref(y) - exact) / exact
        slope = np.maximum(x * (1 - y * y - y / x), 1e-300)   # x A'(x), A' = 1 - A^2 - A / x
        tol = 2 * own + 8 * EPS * np.maximum(1.0, y / slope) + 64 * EPS
        assert np.all(np.abs(got - exact) / exact <= tol), float((np.abs(got - exact) / exact / tol).max())
        # and against the exact argument where the function is well conditioned
        well = y / slope < 1e3
        assert np.all(np.abs(got[well] - x[well]) / x[well] <= tol[well] + 1e-6)
    assert np.abs(inv(V.bessel_ratio(mid)) / mid - 1).max() < 1e-6   # the reference's own figure is 1e-9 typical


def test_inverse_bessel_ratio_clips_at_both_ends():
    inv = vonmises.inverse_bessel_ratio
    assert inv(0.0) == pytest.approx(1e-5, rel=1e-12) and inv(-0.3) == inv(0.0)
    assert inv(1.0) == pytest.approx(700.0, rel=1e-12) and inv(1.5) == inv(1.0)
    assert inv(np.array([[0.0, 1.0]])).shape == (1, 2)
    assert np.isnan(inv(np.nan))


def test_mstep_is_the_restatement_and_survives_empty_states(mle):
    rs = np.random.RandomState(0)
    K, F = 4, 3
    post = np.array([30.0, 0.0, 12.5, 1e-12])
    mu = rs.uniform(-np.pi, np.pi, (K, F))
    r = rs.uniform(0.05, 0.95, (K, F))
    stats = {'post': post, 'cosobs': post[:, None] * r * np.cos(mu), 'sinobs': post[:, None] * r * np.sin(mu),
             'trans': rs.rand(K, K) * 10}
    for rt in ('transpose',):
        est = vonmises.VonMisesHMM(n_states=K, reversible_type=rt)
        est.stats = dict(stats)
        est._do_mstep()
        m, k, T, p = V.mstep(stats, mle, rt)
        assert np.array_equal(est.means_, m) and np.array_equal(est.transmat_, T) and np.array_equal(est.populations_, p)
        np.testing.assert_allclose(est.kappas_, k, rtol=1e-12)
        assert np.all(np.isfinite(est.kappas_)) and np.all(np.isfinite(est.means_))
        # a state without weight: atan2(0, 0) = 0 and the smallest concentration the table holds
        assert np.all(est.means_[1] == 0.0) and np.allclose(est.kappas_[1], 1e-5, rtol=1e-9)
        # the weighted states recover what the sums were made from
        np.testing.assert_allclose(est.means_[[0, 2]], mu[[0, 2]], atol=1e-12)
        np.testing.assert_allclose(V.bessel_ratio(est.kappas_[[0, 2]]), r[[0, 2]], rtol=1e-6)


@pytest.mark.parametrize("name,dn,kw,ragged,tight", V.GOLDEN, ids=IDS)
def test_overlap_against_the_golden(golden, name, dn, kw, ragged, tight):
    g = golden
    est = vonmises.VonMisesHMM(n_states=3)
    est.__setstate__((g[name + "_means"], g[name + "_kappas"], g[name + "_transmat"], g[name + "_populations"], None, 0.0, 2))
    got = est.overlap_
    assert got.shape == (3, 3) and np.all(np.isfinite(got))
    assert np.all(np.diag(got) == 0.0) and np.allclose(got, got.T, atol=1e-12) and np.all(got <= 1e-12)
    # the reference normalises in place (vmhmm_ref.overlap): put back what its loop leaves out, then compare; log I0 of
    # concentrations near 20 is near 20 and rounds at its own magnitude in both
    want = V.overlap_from_reference(g[name + "_overlap"], g[name + "_means"], g[name + "_kappas"])
    scale = float(np.abs(np.asarray(V.log_i0(2 * g[name + "_kappas"]), dtype=np.float64)).sum(1).max())
    assert finite_close(got, want, 64 * EPS * max(scale, 1.0))
    assert finite_close(got, V.overlap(g[name + "_means"], g[name + "_kappas"]), 64 * EPS * max(scale, 1.0))


# ---- the bound ---------------------------------------------------------------------------------------------------
CASES = V.estep_cases(gaussian.plan)


@pytest.mark.parametrize("name,seqs,mdl,segment", CASES, ids=[c[0] for c in CASES])
def test_split_form_within_the_bound_of_the_direct_form(name, seqs, mdl, segment):
    b = V.bound(seqs, *mdl)
    assert b['rel'] < 1e-6   # (one float32 intermediate anywhere fails it; the sharpest models and the longest
    #                           trajectory are what take it above sqrt(u))
    yard = V.estep(seqs, *mdl)
    ref = V.estep(seqs, *mdl, dt=np.float64, form='split')
    V.check_stats(ref, yard, b, who=name)


def test_viterbi_cases_have_margins_above_the_bound():
    for name, seqs, mdl, res in V.viterbi_cases(gaussian.plan):
        b = V.bound(seqs, *mdl)
        for (lp, states, margin), need in zip(res, b['logprob']):
            assert margin > 2 * need, name
        # and the float64 split form decides as the longdouble direct form does
        for X, (lp, states, margin) in zip(seqs, res):
            assert np.array_equal(V.viterbi(X, *mdl, dt=np.float64, form='split')[1], states), name


def test_bounds_profile_lists_every_case():
    with open(V.BOUNDS_FILE) as fh:
        text = fh.read()
    assert V.read_tau() is not None, "profiles/vmhmm_bounds.txt says not measured"
    for name, seqs, mdl, segment in CASES:
        assert V.bounds_line(name, V.bound(seqs, *mdl)) in text, name
