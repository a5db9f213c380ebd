"""CPU tests of the PCCA / PCCA+ restatement (tests/pcca_ref.py) against the reference's stored runs
(tests/golden/pcca_golden.npz, written by tests/golden/make_golden_pcca.py), of the host module functions of
``msmbuilder_amd.lumping.pcca_plus`` against the restatement, of the identity that replaces T by the m x m moments, of the
lattice systems' exactness, of the bounds table, and of what the estimators refuse before any device work."""
import os
import sys

import numpy as np
import pytest

import pcca_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_pcca import GOLDEN, OPTIMISED  # noqa: E402

LD = np.longdouble


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "pcca_golden.npz")))


def system(golden, name):
    n, m, seed = GOLDEN[name]
    T, pi, labels = R.planted(n, m, seed)
    return dict(T=T, pi=pi, V=golden[name + '_V'], labels=labels, n=n, m=m)


def close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rtol * np.abs(b).max())


@pytest.mark.parametrize("name", list(GOLDEN))
def test_restatement_and_host_functions_against_the_reference(golden, name):
    """Integers equal, reals to 1e-12 relative: index_search, fill_A, chi and the mapping, the three objectives at the listed
    alphas (-inf where the reference says -inf), PCCA's splitting -- by the restatement and by the package's host functions."""
    from msmbuilder_amd.lumping import pcca_plus as PP
    from msmbuilder_amd.lumping.pcca import split_by_sign
    s = system(golden, name)
    T, pi, V, m = s['T'], s['pi'], s['V'], s['m']
    assert len(golden[name + '_V']) == s['n'] and 8 <= s['n'] <= 257 and 2 <= m <= 9
    assert close(V, R.eigenvectors(T, pi, m), 1e-8)            # (the stored eigenvectors are this system's)
    A0, index = R.initial_A(V)
    assert np.array_equal(index, golden[name + '_index']) and np.array_equal(PP.index_search(V), index)
    assert close(A0, golden[name + '_A0']) and close(PP.fill_A(np.linalg.inv(V[index]), V), golden[name + '_A0'])
    chi, mapping = R.chi_of(A0, V)
    assert close(chi, golden[name + '_chi0']) and np.array_equal(mapping, golden[name + '_map0'])
    assert R.same_partition(mapping, s['labels'])
    flat_map, square_map = PP.get_maps(np.zeros((m, m)))
    assert np.array_equal(PP.to_square(PP.to_flat(np.asarray(A0, dtype=float), flat_map), square_map)[1:, 1:], np.asarray(A0, dtype=float)[1:, 1:])
    assert not PP.has_constraint_violation(np.asarray(A0, dtype=float), V)
    for alpha, values in zip(golden[name + '_alphas'], golden[name + '_values']):
        A, chi_f, map_f = PP.calculate_fuzzy_chi(alpha, square_map, V)
        for kind, fn in enumerate(R.KINDS):
            want = values[kind]
            got_r = float(R.objective(kind, alpha, T, pi, V)[0])
            got_h = getattr(PP, fn)(alpha, T, V, square_map, pi)
            if np.isinf(want):
                assert np.isneginf(want) and np.isneginf(got_r) and np.isneginf(got_h)
            else:
                assert abs(got_r - want) <= 1e-12 * abs(want) and abs(got_h - want) <= 1e-12 * abs(want)
                assert np.array_equal(map_f, R.objective(kind, alpha, T, pi, V)[1]['mapping'])
    assert np.isneginf(golden[name + '_values'][-1]).all() and not golden[name + '_alphas'][-1].any()   # the all-zero alpha
    assert np.array_equal(R.pcca_split(V[:, 1:], m), golden[name + '_pcca'])
    assert np.array_equal(split_by_sign(V[:, 1:], m, 1e-5), golden[name + '_pcca'])
    if name in OPTIMISED:
        for k in range(3):
            assert R.same_partition(golden[name + '_opt_map'][k], s['labels'])
            assert golden[name + '_opt_value'][k] >= golden[name + '_values'][0, k]


@pytest.mark.parametrize("n,m", [(8, 2), (33, 3), (33, 6), (129, 3), (257, 6)])
def test_moments_replace_the_transition_matrix(n, m):
    """chi_i^T diag(pi) T chi_i = (A^T G A)_ii and chi_i^T pi = (A^T w)_i: algebra, for any V and any A -- on the planted
    models and on a V of noise."""
    s = R.planted_system(n, m, 1)
    noise = np.random.RandomState(n + m).standard_normal((n, m))
    for V in (s['V'], noise):
        G, w = R.moments(s['T'], s['pi'], V)
        for alpha in R.alphas_around(s['V'], 3, 2):
            A = R.fill_A(R.to_square(alpha, m), V)
            chi = np.asarray(V, dtype=LD) @ A
            direct = (((np.asarray(s['pi'], dtype=LD)[:, None] * chi) * (np.asarray(s['T'], dtype=LD) @ chi)).sum(axis=0) / (chi.T @ np.asarray(s['pi'], dtype=LD))).sum()
            assert abs(R.metastability_from_moments(A, G, w) - direct) <= 1e-15 * abs(direct)


def test_lattice_systems_are_exact_in_any_order():
    """Every product and sum on a lattice system is a small dyadic rational: float64 and longdouble give the same numbers, and
    so does a permuted order of summation.  The memberships put every state in its home macrostate; the tie is exact."""
    for n, m in ((2, 2), (9, 2), (65, 8), (129, 17), (257, 64)):
        s = R.lattice(n, m, 0, zero_population=n > 3 * m)
        assert not np.any(np.mod(s['T'] * 4, 1)) and not np.any(np.mod(s['pi'] * 16, 1)) and not np.any(np.mod(s['V'] * 4, 1))
        A = R.fill_A(R.to_square(s['alpha'], m), s['V'])
        assert np.array_equal(A, A.astype(np.float64)) and A[0].sum() == 1 and np.log2(s['P']) % 1 == 0
        chi64 = s['V'] @ A.astype(np.float64)
        perm = np.random.RandomState(n).permutation(m)
        assert np.array_equal(chi64, R.chi_of(A, s['V'])[0]) and np.array_equal(chi64, s['V'][:, perm] @ A.astype(np.float64)[perm])
        assert np.array_equal(np.argmax(chi64, axis=1), np.arange(n) % m)
        order = np.random.RandomState(n + 1).permutation(n)
        G, w = R.moments(s['T'], s['pi'], s['V'])
        G2, w2 = R.moments(s['T'][np.ix_(order, order)], s['pi'][order], s['V'][order])
        assert np.array_equal(G, G2) and np.array_equal(w, w2) and np.array_equal(G, G.astype(np.float64))
        value = [R.replay(kind, s)[0] for kind in range(3)]
        assert np.all(np.isfinite(value))
        assert abs(value[2] - float(R.objective(2, s['alpha'], s['T'], s['pi'], s['V'])[0])) <= 1e-13 * abs(value[2])
    tie = R.lattice(9, 2, 1, tie=True)
    chi, mapping = R.chi_of(R.fill_A(R.to_square(tie['alpha'], 2), tie['V']), tie['V'])
    assert chi[8].tolist() == [0.5, 0.5] and mapping[8] == 0


def bounds_table():
    lines = ["# |device - exact| <= bound for the three PCCA+ objectives and chi: pcca_ref.device_bounds at the first perturbed alpha",
             "# of pcca_ref.alphas_around(V, 20, 100 + n + m) on pcca_ref.planted_system(n, m, 0) (what tests/test_gpu_pcca.py runs)",
             "#    n   m   crispness  metastability  crisp_metastability  chi (largest)"]
    for n, m in ((33, 3), (33, 6), (257, 3), (257, 6), (1025, 3), (1025, 6)):
        s = R.planted_system(n, m, 0)
        b = R.device_bounds(s, R.alphas_around(s['V'], 20, 100 + n + m)[1])
        lines.append("%6d %3d   %.2e   %.2e       %.2e             %.2e" % ((n, m) + tuple(b['value']) + (b['chi'].max(),)))
    return lines


def test_bounds_table_is_the_committed_one():
    """profiles/pcca_bounds.txt holds the table the bound gives (to the 3 digits printed, and 1 % for another BLAS)."""
    path = os.path.join(os.path.dirname(HERE), "profiles", "pcca_bounds.txt")
    kept = [ln.rstrip("\n") for ln in open(path) if ln.strip() and not ln.startswith("observed")]
    table = bounds_table()
    assert len(kept) == len(table) and kept[:3] == table[:3]
    for a, b in zip(kept[3:], table[3:]):
        fa, fb = np.array(a.split(), dtype=float), np.array(b.split(), dtype=float)
        assert np.array_equal(fa[:2], fb[:2]) and np.allclose(fa[2:], fb[2:], rtol=1e-2)
        assert np.all(fb[2:] < 1e-10)      # far below what tells two lumpings apart


def test_estimators_refuse_before_any_device_work():
    from msmbuilder_amd import PCCA, PCCAPlus
    from msmbuilder_amd.lumping import PCCA as P2, PCCAPlus as PP2
    from sklearn.base import clone
    assert PCCA is P2 and PCCAPlus is PP2
    with pytest.raises(AttributeError, match="does not use an objective function"):
        PCCA(3, objective_function='crispness')
    with pytest.raises(AttributeError, match="must be one of"):
        PCCAPlus(3, objective_function='nonsense')
    assert PCCAPlus(3, objective_function=None).objective_function == 'crisp_metastability'
    model = PCCAPlus(4, do_minimization=False, objective_function='metastability', random_state=7, lag_time=3, pcca_tolerance=1e-3, verbose=False)
    params = clone(model).get_params()
    assert (params['n_macrostates'], params['do_minimization'], params['objective_function'], params['random_state'],
            params['lag_time'], params['pcca_tolerance']) == (4, False, 'metastability', 7, 3, 1e-3)
    assert clone(PCCA(2, lag_time=5, pcca_tolerance=0.5)).get_params()['lag_time'] == 5
    # too few eigenvectors: n_timescales = 1 yields two, three are asked for (no device is needed: the eigensystem is set)
    s = R.planted_system(12, 3, 0)
    msm = R.fitted_msm(s['T'], s['pi'], n_timescales=1)
    msm._eigenvalues, msm._left_eigenvectors, msm._right_eigenvectors, msm._is_dirty = np.ones(2), s['V'][:, :2], s['V'][:, :2], False
    for cls in (PCCA, PCCAPlus):
        lumper = cls(3, n_timescales=1, verbose=False)
        lumper.transmat_, lumper.populations_, lumper.n_states_ = s['T'], s['pi'], 12
        lumper._right_eigenvectors, lumper._eigenvalues, lumper._left_eigenvectors, lumper._is_dirty = s['V'][:, :2], np.ones(2), s['V'][:, :2], False
        with pytest.raises(ValueError, match="n_macrostates=3 needs 3 eigenvectors, but n_timescales=1 on 12 states yields 2"):
            lumper._do_lumping()
    # PCCA itself needs no device once the eigenvectors are there: pcca_tolerance moves the cut, fill / clip map labels
    lumper = PCCA(3, verbose=False)
    lumper.transmat_, lumper.populations_, lumper.n_states_ = s['T'], s['pi'], 12
    lumper._right_eigenvectors, lumper._eigenvalues, lumper._left_eigenvectors, lumper._is_dirty = s['V'], np.ones(3), s['V'], False
    lumper.mapping_ = {10 * i: i for i in range(12)}
    lumper._do_lumping()
    assert np.array_equal(lumper.microstate_mapping_, R.pcca_split(s['V'][:, 1:], 3)) and lumper.microstate_mapping_.dtype == int
    assert R.same_partition(lumper.microstate_mapping_, s['labels'])
    high = PCCA(3, pcca_tolerance=10.0, verbose=False)
    high.__dict__.update({k: v for k, v in lumper.__dict__.items() if k != 'pcca_tolerance'})
    with pytest.raises(ValueError, match="is empty"):     # nothing reaches a tolerance of 10: the split leaves a macrostate empty
        high._do_lumping()
    mp = lumper.microstate_mapping_
    clipped = lumper.partial_transform([0, 10, 5, 110, 20], mode='clip')
    assert [c.tolist() for c in clipped] == [mp[[0, 1]].tolist(), mp[[11, 2]].tolist()]
    filled = lumper.partial_transform([0, 10, 5, 110], mode='fill')
    assert np.isnan(filled[2]) and filled[[0, 1, 3]].tolist() == mp[[0, 1, 11]].astype(float).tolist()
    assert lumper.partial_transform([0, 10], mode='fill').tolist() == mp[[0, 1]].tolist()
    with pytest.raises(ValueError, match="mode must be one of"):
        lumper.partial_transform([0], mode='other')
    assert [x.tolist() for x in lumper.transform([[0, 10], [5, 20]])] == [mp[[0, 1]].tolist(), mp[[2]].tolist()]
