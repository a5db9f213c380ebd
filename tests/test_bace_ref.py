"""CPU tests of the BACE restatement (tests/bace_ref.py) against the reference's stored runs (tests/golden/bace_golden.npz,
written by tests/golden/make_golden_bace.py), of the four deliberate differences on hand cases, and of the host side of
``msmbuilder_amd.lumping.BACE`` -- maps and Bayes factors from a merge record -- with the device call replaced by the
restatement's record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bace_ref as R  # noqa: E402

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bace_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN_PATH) as z:
        return {k: z[k] for k in z.files}


_WIDE = {}


def wide_run(name):
    """The longdouble restatement of a golden case, computed once per session."""
    if name not in _WIDE:
        _WIDE[name] = R.golden_run(name, wide=True)
    return _WIDE[name]


def within_ulps(got, want, ulps):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    with np.errstate(all='ignore'):
        return np.all((got == want) | (np.abs(got.astype(np.float64) - want) <= ulps * np.spacing(np.maximum(np.abs(got), np.abs(want)))))


@pytest.mark.parametrize("name", list(R.GOLDEN))
def test_restatement_against_reference(golden, name):
    spec = R.GOLDEN[name]
    narrow = R.golden_run(name, wide=False)
    r = wide_run(name)
    assert [tuple(m) for m in golden[name + "_merges"]] == r['merges'] == narrow['merges']
    assert all(np.array_equal(narrow['maps'][k], r['maps'][k]) for k in r['maps']) and sorted(narrow['maps']) == sorted(r['maps'])
    assert within_ulps([narrow['bayes'][k] for k in sorted(narrow['bayes'])], [r['bayes'][k] for k in sorted(r['bayes'])], 2), name
    assert min(narrow['gaps']) >= 64 * R.F32_ULP
    left = sorted(r['maps'], reverse=True)
    assert len(left) == len(golden[name + "_maps"])
    for k, want in zip(left, golden[name + "_maps"]):
        assert np.array_equal(r['maps'][k], want), (name, k)
    assert np.array_equal(r['filter_map'], golden[name + "_filter_map"])
    keys = golden[name + "_bayes_keys"].tolist()
    assert keys == sorted(r['bayes'], reverse=True)
    assert all(isinstance(r['bayes'][k], np.float32) for k in keys)
    assert within_ulps([r['bayes'][k] for k in keys], golden[name + "_bayes"], 2), name
    assert min(r['gaps']) >= 64 * R.F32_ULP and golden[name + "_min_gap"] >= 64 * R.F32_ULP
    # (a): always set, and the entry of the maps at n_macrostates
    assert np.array_equal(r['mapping'], r['maps'][spec['n_macrostates']])
    if golden[name + "_mapping"].min() >= 0:
        assert np.array_equal(r['mapping'], golden[name + "_mapping"])


def test_bounds_file_is_current():
    """The derived bound stays below half the admission gap for every golden case (asserted inside), and
    profiles/bace_bounds.txt holds exactly the table these goldens and this bound give."""
    report = R.bounds_report({name: wide_run(name) for name in R.GOLDEN})
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bace_bounds.txt")
    with open(path) as f:
        assert f.read().startswith(report + "\n")


def test_golden_cases_cover_the_issue(golden):
    assert {R.GOLDEN[k]['n'] for k in R.GOLDEN} >= {8, 31, 32, 33, 65, 130, 257, 48}
    pruned = 48 - len(np.unique(golden["weak48_filter_map"]))
    assert 1 <= pruned <= 5 and golden["weak48_maps"].min() >= 0
    assert (R.golden_counts(R.GOLDEN['sparse40']) == 0).mean() > 0.65
    # the reference leaves microstate_mapping_ unset where one merge is needed
    assert golden["one_merge_mapping"].min() == -1 and len(golden["one_merge_merges"]) == 1
    assert len(golden["two_merges_merges"]) == 2 and len(golden["to_one_merges"]) == 11
    assert np.isinf(golden["to_one_bayes"][-1])   # the look-ahead at one state: nothing left to compare


def test_difference_a_mapping_without_a_merge():
    C = R.block_counts(12, 2, 0)
    for nm in (12, 40):
        r = R.bace(C, nm, filt=0)
        assert r['merges'] == [] and r['maps'] == {} and np.array_equal(r['mapping'], np.arange(12))
        assert sorted(r['bayes']) == [11]
    weak = R.golden_counts(R.GOLDEN['weak48'])
    r = R.bace(weak, 48, filt=1.1)
    assert r['merges'] == [] and np.array_equal(r['mapping'], r['filter_map']) and r['mapping'].max() == len(r['keep']) - 1


def test_difference_c_no_candidate_pair():
    C = R.disconnected_counts()
    r = R.bace(C, 2, filt=0)
    assert r['mapping'].tolist() == [0, 0, 1, 1]
    assert np.isinf(r['bayes'][1]) and r['values'][-1] == 0     # the look-ahead finds no pair: inf, and no error
    with pytest.raises(ValueError, match="at 2 states"):
        R.bace(C, 1, filt=0)


def test_difference_d_self_heavy_pruned_state(golden):
    C = R.self_heavy_counts()
    assert C[0].argmax() == 0
    r = R.bace(C, 2, filt=1.1)
    assert 0 not in r['keep'] and r['filter_map'][0] == r['filter_map'][2] and r['filter_map'].min() == 0
    assert golden["self_heavy_reference_map"].min() == -1        # what the reference makes of it
    assert all(m.min() >= 0 and m[0] == m[2] for m in r['maps'].values())
    lone = C.copy()
    lone[0, 1:] = 0
    with pytest.raises(ValueError, match="no counts to any other state"):
        R.bace(lone, 2, filt=1.1)


def test_first_maximum_rule():
    d = np.zeros((4, 4), dtype=np.float32)
    assert R.first_maximum(d)[:3] == (-1, -1, 0)
    d[2, 1] = d[1, 3] = 5.0
    d[3, 0] = -7.0
    assert R.first_maximum(d)[:2] == (1, 3) and R.first_maximum(d)[3] == 0.0
    d[3, 2] = np.inf
    assert R.first_maximum(d)[:2] == (3, 2)
    d[0, 1] = np.inf
    assert R.first_maximum(d)[:2] == (0, 1)
    r = R.bace(R.tied_counts(), 2, filt=0)
    assert r['merges'][0] == (1, 7) and r['gaps'][0] == 0.0 and np.isfinite(r['values'][0])
    r = R.bace(R.duplicated_counts(20, 2, 0), 2, filt=0)
    assert r['merges'][0] == (1, 4) and np.isinf(r['values'][0]) and r['bayes'][19] == 0.0


# ---- the estimator's host side ------------------------------------------------------------------------------------------
class _Msm(object):
    def __init__(self, counts, **params):
        from msmbuilder_amd import MarkovStateModel
        self._model = MarkovStateModel(verbose=False, **params)
        n = len(counts)
        self.transmat_, self.populations_, self.countsmat_ = None, np.full(n, 1.0 / n), counts
        self.mapping_, self.n_states_ = dict(zip(range(n), range(n))), n

    def get_params(self):
        return self._model.get_params()


def _record_from_restatement(monkeypatch, calls):
    """``bace_merges`` answered by the restatement's merge loop on the arguments the estimator hands over."""
    from msmbuilder_amd.lumping import bace as B

    def fake(counts, w, keep, n_macrostates, timings=False):
        c, w, keep = np.array(counts), np.array(w), np.flatnonzero(keep)
        calls.append((c.copy(), w.copy(), keep.copy()))
        unm = np.zeros(len(c), dtype=np.int8)
        unm[keep] = 1
        dmat = R.initial_matrix(c, w, unm, keep)[0]
        merges, values = [], []
        total = max(len(keep) - n_macrostates, 0)
        for step in range(total + 1):
            x, y, v, _gap = R.first_maximum(dmat)
            merges.append((x, y))
            values.append(v)
            if x < 0:
                merges += [(-1, -1)] * (total - step)
                values += [np.float32(0)] * (total - step)
                break
            if step < total:
                keep = R.merge_counts(c, w, unm, keep, x, y)
                dmat[[x, y], :] = 0
                dmat[:, [x, y]] = 0
                dmat[x, :] = R.initial_matrix(c, w, unm, keep, row=x)[0][x, :]
        return np.array(merges, dtype=np.int32).reshape(-1, 2), np.array(values, dtype=np.float32)
    monkeypatch.setattr(B, "bace_merges", fake)


@pytest.mark.parametrize("name", ["n33", "weak48", "lag3", "to_one", "one_merge"])
def test_estimator_host_side(golden, monkeypatch, name):
    from msmbuilder_amd import BACE
    from msmbuilder_amd.lumping import BACE as BACE2
    assert BACE is BACE2
    spec, calls = R.GOLDEN[name], []
    _record_from_restatement(monkeypatch, calls)
    msm = _Msm(R.golden_counts(spec), lag_time=spec.get('lag_time', 1), sliding_window=spec.get('sliding_window', True))
    before = msm.countsmat_.copy()
    m = BACE.from_msm(msm, spec['n_macrostates'], filter=spec['filter'])
    assert np.array_equal(msm.countsmat_, before) and m.countsmat_ is msm.countsmat_
    left = sorted(m.map_dict, reverse=True)
    assert left == list(range(len(calls[0][2]) - 1, spec['n_macrostates'] - 1, -1))
    for k, want in zip(left, golden[name + "_maps"]):
        assert np.array_equal(m.map_dict[k], want) and m.map_dict[k].dtype == np.int32
    assert m.microstate_mapping_.dtype == np.int32 and np.array_equal(m.microstate_mapping_, m.map_dict[spec['n_macrostates']])
    assert sorted(m.bayesFactors, reverse=True) == golden[name + "_bayes_keys"].tolist()
    assert all(isinstance(v, np.float32) for v in m.bayesFactors.values())
    assert within_ulps([m.bayesFactors[k] for k in sorted(m.bayesFactors, reverse=True)], golden[name + "_bayes"], 2)
    # (b): a second lumping of the same object starts afresh
    m.n_macrostates = spec['n_macrostates'] + 1
    m._do_lumping()
    assert set(m.map_dict) == set(range(spec['n_macrostates'] + 1, len(calls[0][2]))) and min(m.bayesFactors) == spec['n_macrostates']
    none = BACE.from_msm(msm, spec['n_macrostates'], filter=spec['filter'], save_all_maps=False)
    assert not hasattr(none, 'map_dict') and np.array_equal(none.microstate_mapping_, golden[name + "_maps"][-1])


def test_estimator_parameters_and_refusals(monkeypatch):
    from msmbuilder_amd import BACE
    from sklearn.base import clone
    m = BACE(3, filter=0, n_proc=4, chunk_size=7, lag_time=2, verbose=False)
    p = m.get_params()
    assert (p['n_macrostates'], p['filter'], p['save_all_maps'], p['n_proc'], p['chunk_size'], p['lag_time']) == (3, 0, True, 4, 7, 2)
    q = clone(m).get_params()
    assert q['n_proc'] == 4 and q['chunk_size'] == 7 and q['lag_time'] == 2
    d = BACE(3)
    assert (d.filter, d.save_all_maps, d.n_proc, d.chunk_size, d.map_dict) == (1.1, True, 1, 100, {})
    with pytest.raises(RuntimeError, match="n_macrostates must not be None to transform"):
        BACE(None).partial_transform([0, 1])
    C = R.block_counts(12, 2, 0)
    assert not hasattr(BACE.from_msm(_Msm(C), None), 'microstate_mapping_')
    with pytest.raises(ValueError, match="n_macrostates"):
        BACE.from_msm(_Msm(C), 0, filter=0)
    for bad in (-1.0, np.nan, np.inf):
        X = C.copy()
        X[3, 4] = bad
        with pytest.raises(ValueError, match="non-negative and finite"):
            BACE.from_msm(_Msm(X), 2, filter=0)
    with pytest.raises(ValueError, match="at most 16384 states"):
        BACE.from_msm(_Msm(np.broadcast_to(np.ones(1), (16385, 16385))), 2, filter=0)
    with pytest.raises(ValueError, match="at least 2 states"):
        BACE.from_msm(_Msm(np.ones((1, 1))), 1, filter=0)
    # (c) and (d) through the estimator
    calls = []
    _record_from_restatement(monkeypatch, calls)
    two = R.disconnected_counts()
    ok = BACE.from_msm(_Msm(two), 2, filter=0)
    assert np.isinf(ok.bayesFactors[1]) and ok.microstate_mapping_.tolist() == [0, 0, 1, 1]
    with pytest.raises(ValueError, match="at 2 states"):
        BACE.from_msm(_Msm(two), 1, filter=0)
    heavy = BACE.from_msm(_Msm(R.self_heavy_counts()), 2, filter=1.1)
    assert heavy.microstate_mapping_.min() == 0 and heavy.microstate_mapping_[0] == heavy.microstate_mapping_[2]
    lone = R.self_heavy_counts()
    lone[0, 1:] = 0
    with pytest.raises(ValueError, match="no counts to any other state"):
        BACE.from_msm(_Msm(lone), 2, filter=1.1)
    mapped = ok.partial_transform(np.array([0, 3, 2]), mode='fill')
    assert np.array_equal(mapped, ok.microstate_mapping_[[0, 3, 2]])
    with pytest.raises(ValueError, match="mode must be one of"):
        ok.partial_transform([0, 1], mode='other')
