"""GPU tier of the von Mises HMM: msm_hmm_trig_{f32,f64}, msm_hmm_lin_{estep,score,loglik,viterbi} and VonMisesHMM against
the longdouble restatement under its rounding bound (tests/vmhmm_ref.py; held to the reference's goldens by
tests/test_vmhmm_ref.py) and against the goldens themselves.

Shapes are the smallest that reach each seam of the device code: the image at row counts either side of a workgroup
and past one grid round of it, widths 1, odd, even and past a workgroup; the E-step at the seam lengths of every segment
length, the K seams of msm_hmm_plan, and widths at which D = 2 F crosses the 256 threads of a workgroup and K D one
round of them.  One longdouble reference per case, shared by the tests that need it."""
import ctypes as C
import functools
import os
import pickle
import re

import numpy as np
import pytest

import vmhmm_ref as V
from msmbuilder_amd import _lib
from msmbuilder_amd.hmm import VonMisesHMM, gaussian, vonmises

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vmhmm_golden.npz")
STAT_KEYS = ('post', 'obs', 'trans', 'traj_logprob')


class Fixed(VonMisesHMM):
    """The goldens' starts, one per run of n_init."""

    def _init(self, sequences):
        starts = V.golden_starts(2)
        k = getattr(self, "_run", 0)
        self._run = k + 1
        means, kappas, transmat, pops = starts[k % len(starts)]
        self.__setstate__((means.copy(), kappas.copy(), transmat.copy(), pops.copy(), None, 0.0, means.shape[1]))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def rows_of(seqs, how="device"):
    """The trajectories back to back on the device, on the host, or pitched (a column slice of a wider array)."""
    X = np.concatenate(seqs)
    lengths = [len(s) for s in seqs]
    if how == "device":
        X = dev(X)
    elif how != "host":
        wide = np.zeros((X.shape[0], X.shape[1] + 3), dtype=X.dtype)
        wide[:, :X.shape[1]] = X
        wide[:, X.shape[1]:] = np.nan   # never read
        X = dev(wide)[:, :X.shape[1]] if how == "device_pitched" else wide[:, :X.shape[1]]
    return gaussian._Rows(X, lengths)


def image_of(seqs, how="device", pad=0):
    return vonmises.trig(rows_of(seqs, how), pad=pad)


def form(mdl):
    means, kappas, A, lsp = mdl
    return vonmises.linear_form(means, kappas) + (A, lsp)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- the image ---------------------------------------------------------------------------------------------------
def test_image_and_tau(gpu):
    """Every shape and dtype of the image from device rows, the largest error against longdouble cos / sin of the exactly
    widened element in units of u printed and held to the tau of the bound (twice the recorded measurement, because
    the arguments are sampled, not exhausted)."""
    worst = 0.0
    for dn in ('f32', 'f64'):
        for n in V.IMAGE_N:
            for F in V.IMAGE_F:
                X = V.image_arguments(n, F, dn)
                Z = image_of([X]).X.cpu().numpy()
                assert Z.shape == (n, 2 * F) and Z.dtype == np.float64
                err = V.image_error(Z, X)
                worst = max(worst, err)
                assert np.all(np.abs(Z) <= 1.0)
    print("tau_measured %.4f" % worst)
    recorded = V.read_tau()
    assert recorded is not None, "profiles/vmhmm_bounds.txt holds no measurement; this run measured %.4f" % worst
    assert worst <= 2.0 * recorded, (worst, recorded)


@pytest.mark.parametrize("dn", ['f32', 'f64'])
@pytest.mark.parametrize("how", ["host", "device_pitched", "host_pitched"])
def test_image_placement(gpu, dn, how):
    for n, F in ((257, 3), (255, 129), (1, 1)):
        X = V.image_arguments(n, F, dn)
        want = image_of([X]).X.cpu().numpy()
        got = image_of([X], how).X.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (n, F)   # the same arithmetic wherever the rows lie
        padded = image_of([X], how, pad=5)
        assert padded.ld == 2 * F + 5
        assert np.array_equal(bits(padded.X.cpu().numpy()), bits(want))
        whole = padded.X.as_strided((n, 2 * F + 5), (2 * F + 5, 1)).cpu().numpy()
        assert np.all(np.isnan(whole[:, 2 * F:]))   # the pitch is never written


def test_image_special_angles(gpu):
    for dn in ('f32', 'f64'):
        dt = V.DT[dn]
        x = np.array([[0.0, np.pi, -np.pi, 50.0, -50.0, 1e5, -1e5, 5e-324 if dn == 'f64' else 1e-45]], dtype=dt)
        Z = image_of([x]).X.cpu().numpy()
        assert V.image_error(Z, x) <= V.tau()
        assert Z[0, 0] == 1.0 and Z[0, 8] == 0.0          # cos 0, sin 0
        assert Z[0, 7] == 1.0                              # a denormal: cos = 1
        if dn == 'f64':
            assert Z[0, 1] == -1.0 and Z[0, 2] == -1.0     # (the float32 pi is 8.7e-8 off: its cosine is not -1 in float64)
        # sin of the rounded pi is the rounding error of pi in the rows' type, not zero
        assert abs(Z[0, 9] - float(np.sin(np.longdouble(x[0, 1])))) <= V.tau() * V.U
    bad = np.array([[0.5, np.nan], [np.inf, 1.0]])
    Zb = image_of([bad]).X.cpu().numpy()
    assert np.isnan(Zb[0, 1]) and np.isnan(Zb[0, 3]) and np.isnan(Zb[1, 0]) and np.isnan(Zb[1, 2])
    assert Zb[0, 0] == float(np.cos(0.5)) or abs(Zb[0, 0] - np.cos(0.5)) <= V.tau() * V.U


# ---- emissions ---------------------------------------------------------------------------------------------------
def test_lin_loglik(gpu):
    rs = np.random.RandomState(3)
    for K, F in ((1, 1), (4, 5), (17, 9), (64, 3)):
        means = rs.uniform(-np.pi, np.pi, (K, F))
        kappas = rs.choice(V.KAPPAS, size=(K, F))
        X = V.wrap(rs.uniform(-np.pi, np.pi, (35, F)))
        got = vonmises.lin_loglik(image_of([X]), *vonmises.linear_form(means, kappas))
        want = V.loglik(X, means, kappas)
        assert got.shape == want.shape == (35, K)
        tol = V.emission_error(means, kappas, V.tau())
        assert float(np.abs(got.astype(np.longdouble) - want).max()) <= tol, (K, F)


# ---- E-step ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def estep_cases():
    return {name: (seqs, mdl, segment) for name, seqs, mdl, segment in V.estep_cases(gaussian.plan)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per-trajectory longdouble references of one case (the sums of a list are the sums of its trajectories)."""
    seqs, mdl, _ = estep_cases()[name]
    return [V.estep([X], *mdl) for X in seqs]


def add_refs(refs):
    out = {k: sum(r[k] for r in refs) for k in ('post', 'obs', 'trans')}
    out['traj_logprob'] = np.concatenate([r['traj_logprob'] for r in refs])
    return out


def check(seqs, mdl, refs, segment, who=''):
    got = vonmises.lin_estep(image_of(seqs), *form(mdl), segment=segment)
    b = V.bound(seqs, *mdl)
    V.check_stats(got, add_refs(refs), b, who=who)
    N, K = sum(len(s) for s in seqs), mdl[0].shape[0]
    assert abs(got['post'].sum() - N) <= b['rel'] * N * K
    assert abs(got['trans'].sum() - (N - len(seqs))) <= b['rel'] * max(N - len(seqs), 1) * K ** 2
    assert got['logprob'] == np.cumsum(got['traj_logprob'])[-1]
    return got


ESTEP_NAMES = [c[0] for c in V.estep_cases(gaussian.plan)]


@pytest.mark.parametrize("name", ESTEP_NAMES)
def test_estep(gpu, name):
    seqs, mdl, segment = estep_cases()[name]
    refs = reference(name)
    check(seqs, mdl, refs, segment, who=name)
    if name.startswith('segment') and len(seqs) > 1:
        for i in range(len(seqs)):   # every seam length on its own
            check(seqs[i:i + 1], mdl, refs[i:i + 1], segment, who='%s T=%d' % (name, len(seqs[i])))


def test_estep_longest_segment(gpu):
    for K in V.H.k_seams(gaussian.plan)[-2:]:
        seqs, mdl, _ = estep_cases()['K%d' % K]
        check(seqs, mdl, reference('K%d' % K), gaussian.plan(K)['segment_max'], who='K=%d longest' % K)


def test_estep_drops_states_and_clamps(gpu):
    seqs, mdl, _ = estep_cases()['mixed_kappa']
    got = check(seqs, mdl, reference('mixed_kappa'), 4)
    # exp(-1400) per feature between the sharp states: their emission ratios underflow, and yet every frame keeps a state
    ll = np.asarray(V.loglik(np.concatenate(seqs), mdl[0], mdl[1]), dtype=np.float64)
    assert (ll.max(1) - ll.min(1)).max() > 708.0
    assert np.all(np.isfinite(got['traj_logprob']))
    seqs, mdl, _ = estep_cases()['zero_transition']
    assert (mdl[2] == 0.0).sum() == 3
    check(seqs, mdl, reference('zero_transition'), 0)


# ---- bit-stability -----------------------------------------------------------------------------------------------
def test_bit_stability_and_score(gpu):
    for name in ('segment31', 'F129', 'K64'):
        seqs, mdl, segment = estep_cases()[name]
        img = image_of(seqs)
        a = vonmises.lin_estep(img, *form(mdl), segment=segment)
        b = vonmises.lin_estep(image_of(seqs, "host"), *form(mdl), segment=segment)
        for k in STAT_KEYS:
            assert np.array_equal(bits(a[k]), bits(b[k])), (name, k)
        assert a['logprob'] == b['logprob']
        tl, lp = vonmises.lin_score(img, *form(mdl), segment=segment)
        assert np.array_equal(bits(tl), bits(a['traj_logprob'])) and lp == a['logprob']
        # a pitched image gives the same bits
        c = vonmises.lin_estep(image_of(seqs, pad=3), *form(mdl), segment=segment)
        for k in STAT_KEYS:
            assert np.array_equal(bits(a[k]), bits(c[k])), (name, k, 'pitched')
        # the halves of obs are the reference's cosobs and sinobs
        refs = add_refs(reference(name))
        F = mdl[0].shape[1]
        bd = V.bound(seqs, *mdl)
        want = np.hstack([sum(r['cosobs'] for r in reference(name)), sum(r['sinobs'] for r in reference(name))])
        assert np.array_equal(np.asarray(want, dtype=np.float64), np.asarray(refs['obs'], dtype=np.float64))
        tol = bd['rel'] * bd['scale']['obs'] + bd['obs_abs']
        assert np.all(np.abs(a['obs'][:, :F].astype(np.longdouble) - want[:, :F]) <= tol[:, :F])
        assert np.all(np.abs(a['obs'][:, F:].astype(np.longdouble) - want[:, F:]) <= tol[:, F:])
    # a segment longer than every trajectory (refused by the E-step): the forward recursion serial in time
    seqs, mdl, _ = estep_cases()['segment31']
    tl, lp = vonmises.lin_score(image_of(seqs), *form(mdl), segment=10 ** 6)
    want = np.concatenate([r['traj_logprob'] for r in reference('segment31')])
    assert np.all(np.abs(tl.astype(np.longdouble) - want) <= V.bound(seqs, *mdl)['logprob'])


# ---- Viterbi -----------------------------------------------------------------------------------------------------
def test_viterbi_paths_are_the_restatements(gpu):
    for name, seqs, mdl, res in V.viterbi_cases(gaussian.plan):
        img = image_of(seqs)
        states, tl, lp = vonmises.lin_viterbi(img, *form(mdl))
        assert states.dtype == np.int32 and lp == np.cumsum(tl)[-1]
        b = V.bound(seqs, *mdl)
        for i, (best, path, margin) in enumerate(res):
            assert margin > 2 * b['logprob'][i]   # the generator's promise: no case is left out
            assert np.array_equal(states[img.offsets[i]:img.offsets[i + 1]], path), (name, i)
            assert abs(np.longdouble(tl[i]) - best) <= b['logprob'][i], (name, i)


def test_viterbi_first_maximum_on_ties(gpu):
    means = np.array([[0.0, 1.0], [0.0, 1.0], [2.5, -2.0], [2.5, -2.0]])
    kappas = np.full((4, 2), 4.0)
    A = np.array([[0.4, 0.4, 0.1, 0.1]] * 2 + [[0.1, 0.1, 0.4, 0.4]] * 2)
    lsp = np.tile(0.25, 4)
    seqs = V.sequences(means[[0, 2]], kappas[[0, 2]], np.array([[0.8, 0.2], [0.3, 0.7]]), [90, 1, 2, 17], 5)
    states, tl, lp = vonmises.lin_viterbi(image_of(seqs), *vonmises.linear_form(means, kappas), A, lsp)
    want = np.concatenate([V.viterbi(X, means, kappas, A, lsp)[1] for X in seqs])
    assert set(np.unique(want)) == {0, 2}
    assert np.array_equal(states, want)


# ---- estimator ---------------------------------------------------------------------------------------------------
def golden_tolerances(g, name, fit):
    """Per quantity: the bound of the E-step's sums carried to the quantity by the amplification the goldens record for
    this very case (measured on the restated fit, doubled because random directions sample a sensitivity and do not
    maximise it), plus the recorded distance of the reference's fitter from the longdouble restatement; log
    probabilities also carry their own bound."""
    b = V.bound(fit, g[name + "_means"], g[name + "_kappas"], g[name + "_transmat"], np.tile(1 / 3.0, 3))
    assert b['rel'] < V.SQRT_U
    tol = {key: 2.0 * float(g[name + "_amp_" + key]) * b['rel'] + float(g[name + "_dist_" + key]) for key in V.AMP_KEYS}
    tol['fit_logprob'] += float(b['logprob'].sum())
    return tol, b


@pytest.mark.parametrize("name,dn,kw,ragged,tight", V.GOLDEN, ids=[c[0] for c in V.GOLDEN])
@pytest.mark.parametrize("where", ["host", "device"])
def test_estimator_golden(gpu, golden, name, dn, kw, ragged, tight, where):
    g = golden
    fit, other = V.golden_data(V.DT[dn], ragged=ragged, tight=tight)
    fit_in, other_in = ([dev(X) for X in fit], [dev(X) for X in other]) if where == "device" else (fit, other)
    est = Fixed(n_states=3, **dict(dict(n_init=1), **kw))
    assert est.fit(fit_in) is est
    tol, b = golden_tolerances(g, name, fit)
    assert len(est.fit_logprob_) == len(g[name + "_fit_logprob"])   # the EM stopping iteration (and the n_init choice)
    for key in ('fit_logprob', 'means', 'kappas', 'transmat', 'populations'):
        got = np.asarray(getattr(est, key + "_"))
        assert got.shape == g[name + "_" + key].shape
        err = float(np.abs(got - g[name + "_" + key]).max())
        assert err <= tol[key], (key, err, tol[key])
    if tight:
        assert est.kappas_.max() > 100.0
    ts = est.timescales_
    assert ts.shape == g[name + "_timescales"].shape
    np.testing.assert_allclose(ts, g[name + "_timescales"], rtol=1e-6)
    want = V.overlap_from_reference(g[name + "_overlap"], g[name + "_means"], g[name + "_kappas"])
    ok = np.isfinite(want)   # (the reference's own overflows where a concentration is above ~355)
    assert np.all(np.isfinite(est.overlap_)) and np.all(np.abs(est.overlap_ - want)[ok] <= tol['overlap'] + 1e-12)
    bo = V.bound(other, g[name + "_means"], g[name + "_kappas"], g[name + "_transmat"], np.tile(1 / 3.0, 3))
    assert abs(est.score(other_in) - float(g[name + "_score"])) <= bo['logprob'].sum() + tol['score']
    lp, paths = est.predict(other_in)
    assert abs(lp - float(g[name + "_predict_logprob"])) <= bo['logprob'].sum() + tol['predict_logprob']
    assert all(p.dtype == np.int32 for p in paths) and [len(p) for p in paths] == [len(X) for X in other]
    assert np.array_equal(np.concatenate(paths), g[name + "_predict_states"])
    assert np.array_equal(np.concatenate(est.predict(fit_in)[1]), g[name + "_fit_states"])


def test_estimator_surface(gpu, golden):
    name, dn, kw, ragged, tight = [c for c in V.GOLDEN if c[0] == 'run_f64'][0]
    fit, other = V.golden_data(V.DT[dn], ragged=ragged, tight=tight)
    est = Fixed(n_states=3, n_init=1, **kw)
    lp, paths = est.fit_predict(fit)
    twin = Fixed(n_states=3, n_init=1, **kw).fit(fit)
    lp2, paths2 = twin.predict(fit)
    assert lp == lp2 and all(np.array_equal(a, b) for a, b in zip(paths, paths2))   # fit_predict is fit().predict
    assert np.array_equal(np.concatenate(paths), golden[name + "_fit_states"])
    number = r"logprob: (\S+)"
    text = re.sub(r"fit_time: [0-9.]+s", "fit_time: #s", est.summarize())
    want = str(golden[name + "_summarize"])
    assert text.startswith("VonMises HMM\n")
    assert re.sub(number, "logprob: #", text) == re.sub(number, "logprob: #", want)
    tol = golden_tolerances(golden, name, fit)[0]['fit_logprob']
    assert abs(float(re.search(number, text).group(1)) - float(re.search(number, want).group(1))) <= tol
    assert float(re.search(number, text).group(1)) == est.fit_logprob_[-1]
    # pickling: the dict layout, and the reference's 7-tuple
    twin = pickle.loads(pickle.dumps(est))
    for key in ('means_', 'kappas_', 'transmat_', 'populations_', 'fit_logprob_'):
        assert np.array_equal(getattr(twin, key), getattr(est, key))
    assert twin.score(other) == est.score(other)
    assert twin.get_params() == est.get_params()
    assert est.get_params() == dict(n_states=3, n_init=1, n_iter=10, thresh=1e-2, reversible_type='mle', random_state=None)
    third = VonMisesHMM(n_states=3)
    third.__setstate__((est.means_, est.kappas_, est.transmat_, est.populations_, est.fit_logprob_, 0.5, 2))
    assert third.score(other) == est.score(other) and third.n_features == 2
    assert third.score([X.astype(np.float32) for X in other]) == pytest.approx(est.score(other), abs=1e-2)


def circle(seed, n_traj=4, T=600):
    means = np.array([[-2.0, 0.5, 2.5], [0.3, 2.4, -1.0], [2.2, -1.5, 0.2]])
    kappas = np.full((3, 3), 12.0)
    A = np.array([[0.95, 0.03, 0.02], [0.02, 0.95, 0.03], [0.03, 0.02, 0.95]])
    out = [V.sample(means, kappas, A, T, seed * 17 + i, np.float32) for i in range(n_traj)]
    return means, [o[0] for o in out], [o[1] for o in out]


def test_default_fit_recovers_the_means(gpu):
    means, seqs, hidden = circle(5)
    a = VonMisesHMM(n_states=3, random_state=7)
    a._init(seqs)
    b = VonMisesHMM(n_states=3, random_state=7)
    b._init([dev(X) for X in seqs])
    assert np.array_equal(a.means_, b.means_) and np.all(a.kappas_ == 1.0) and a.means_.shape == (3, 3)
    assert np.allclose(a.transmat_, 1 / 3.0) and np.allclose(a.populations_, 1 / 3.0)
    est = VonMisesHMM(n_states=3, n_init=2, n_iter=10, random_state=11).fit(seqs)
    gap = np.abs(V.wrap(est.means_[:, None, :] - means[None, :, :])).max(2)   # [fitted, true]
    order = gap.argmin(0)
    assert sorted(order) == [0, 1, 2]
    assert np.all(gap[order, np.arange(3)] <= 0.1), gap
    lp, paths = est.predict(seqs)
    relabel = np.empty(3, dtype=np.int64)
    relabel[order] = np.arange(3)
    assert np.mean(relabel[np.concatenate(paths)] == np.concatenate(hidden)) > 0.99


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    means, seqs, hidden = circle(1, n_traj=2, T=30)
    kappas = np.full((3, 3), 2.0)
    A, lsp = np.full((3, 3), 1 / 3.0), np.tile(1 / 3.0, 3)
    est = VonMisesHMM(n_states=3)
    est.__setstate__((means, kappas, A, np.full(3, 1 / 3.0), None, 0.0, 3))
    limit = gaussian.plan(1)['n_states_max']
    with pytest.raises(ValueError, match=str(limit)):
        VonMisesHMM(n_states=limit + 1).fit(seqs)
    big = V.model(limit + 1, 3, 0)
    with pytest.raises(ValueError, match="n_states = %d is outside 1 .. %d" % (limit + 1, limit)):
        vonmises.lin_estep(image_of(seqs), *form(big))
    with pytest.raises(ValueError, match="All sequences must have the same data type"):
        est.score([seqs[0], seqs[1].astype(np.float64)])
    with pytest.raises(ValueError, match="Unsupported data type"):
        est.score([(s * 10).astype(np.int64) for s in seqs])
    with pytest.raises(ValueError, match="sequences is empty"):
        est.fit([])
    with pytest.raises(ValueError, match="sequences is empty"):
        est.score([seqs[0], seqs[1][:0]])
    with pytest.raises(ValueError, match="All sequences must have 3 features"):
        est.score([seqs[0][:, :2]])
    with pytest.raises(ValueError, match="Invalid value for reversible_type"):
        VonMisesHMM(n_states=3, reversible_type='sideways').fit(seqs)
    for poison in (np.nan, np.inf, -np.inf):
        bad = [seqs[0].copy(), seqs[1].copy()]
        bad[1][7, 1] = poison
        with pytest.raises(ValueError, match="Input contains NaN, infinity"):
            est.score(bad)
        with pytest.raises(ValueError, match="Input contains NaN, infinity"):
            est.predict([dev(X) for X in bad])
        with pytest.raises(ValueError, match="Input contains NaN, infinity"):
            vonmises.lin_estep(image_of(bad), *form((means, kappas, A, lsp)))
    # through the C ABI
    img = image_of(seqs)
    w, cst = vonmises.linear_form(means, kappas)
    with pytest.raises(ValueError, match="segment"):
        vonmises.lin_estep(img, w, cst, A, lsp, segment=gaussian.plan(3)['segment_max'] + 1)
    with pytest.raises(ValueError, match="a weight is not finite"):
        vonmises.lin_estep(img, w * np.inf, cst, A, lsp)
    lib = _lib.lib()
    tl, post, obs, trans, lp = np.zeros(2), np.zeros(3), np.zeros((3, 6)), np.zeros((3, 3)), C.c_double(0.0)
    args = [img.ptr, img.n, 6, img.ld, img.offsets.ctypes.data, 2, 3, w.ctypes.data, cst.ctypes.data, A.ctypes.data, lsp.ctypes.data, 0,
            tl.ctypes.data, post.ctypes.data, obs.ctypes.data, trans.ctypes.data, C.byref(lp)]

    def refused(pos, value, match):
        a = list(args)
        a[pos] = value
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.msm_hmm_lin_estep(*a))
    refused(0, None, "null pointer")
    refused(7, None, "null pointer")
    refused(8, None, "null pointer")
    refused(9, None, "null pointer")
    refused(13, None, "null output")
    refused(3, 5, "bad shape")      # ldz < D
    x = rows_of(seqs)
    with pytest.raises(ValueError, match="bad shape"):   # ldz < 2 n_features
        _lib.check(lib.msm_hmm_trig_f32(x.ptr, x.n, 3, x.ld, img.ptr, 5, 1))
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(lib.msm_hmm_trig_f32(x.ptr, x.n, 3, x.ld, None, 6, 1))
    _lib.check(lib.msm_hmm_lin_estep(*args))   # and the unaltered call is served
    assert abs(post.sum() - img.n) < 1e-9
