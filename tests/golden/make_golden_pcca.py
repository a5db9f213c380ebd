#!/usr/bin/env python
"""tests/golden/make_golden_pcca.py -- generate pcca_golden.npz.

Runs ONLY where the reference tree is present.  The reference's own ``lumping/pcca.py`` and ``lumping/pcca_plus.py`` are
imported *by file path* over the stub modules of make_golden_msm.py (nothing of the reference is copied into this
repository) and their outputs are stored next to this script.  The systems are the planted block models of
tests/pcca_ref.py (``GOLDEN`` below: n from 8 to 257, m from 2 to 9); T and pi are regenerated from seeds by this script and
by the tests alike, the eigenvectors V are stored (they are what every result is sensitive to), and the reference's classes
run on exactly these V: their cached eigensystem is set, so that no second eigensolver comes into play.

Stored per system <name>:
  _V, _index, _A0, _chi0, _map0     index_search; fill_A(inv(V[index])); calculate_fuzzy_chi at it = what
                                    PCCAPlus(do_minimization=False) sets as A_, chi_, microstate_mapping_ (asserted equal)
  _pcca                             PCCA's mapping
  _alphas, _values                  the listed alphas -- the initial one, two perturbed ones, a degenerate one (two equal
                                    columns of A: one macrostate stays empty; m = 2: a NaN), the all-zero one
                                    (a NaN A) -- and the three objectives at each, [alpha, kind]
  _opt_map, _opt_value              (OPTIMISED systems) per objective, under np.random.seed(0): the mapping and the
                                    objective after the reference's minimisation

A case is admitted only where the longdouble restatement and the reference agree on every integer result and every argmax
of a feasible case has a margin of at least 1,000 x the rounding bound of its row of chi; this script asserts that every
listed case is admitted.

Usage:  python tests/golden/make_golden_pcca.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_msm as M  # noqa: E402  (the loader recipe)
import pcca_ref as R  # noqa: E402

GOLDEN = {'p8_2': (8, 2, 0), 'p33_3': (33, 3, 0), 'p65_4': (65, 4, 0), 'p100_9': (100, 9, 0), 'p129_3': (129, 3, 0),
          'p257_6': (257, 6, 0)}
OPTIMISED = ('p33_3', 'p129_3')


def load():
    MSM = M.load_reference_msm()
    sys.modules["msmbuilder.msm"].MarkovStateModel = MSM
    lump = types.ModuleType("msmbuilder.lumping")
    lump.__path__ = [os.path.join(M.REF, "lumping")]
    sys.modules["msmbuilder.lumping"] = lump
    pcca = M._load("msmbuilder.lumping.pcca", os.path.join(M.REF, "lumping", "pcca.py"), "msmbuilder.lumping")
    plus = M._load("msmbuilder.lumping.pcca_plus", os.path.join(M.REF, "lumping", "pcca_plus.py"), "msmbuilder.lumping")
    return pcca.PCCA, plus.PCCAPlus, plus


def listed_alphas(V):
    m = V.shape[1]
    a0, p1, p2 = R.alphas_around(V, 3, 5)
    if m > 2:
        sq = a0.reshape(m - 1, m - 1).copy()
        sq[:, 1] = sq[:, 0]
        degenerate = sq.ravel()
    else:
        degenerate = np.full_like(a0, np.nan)   # (m = 2: every nonzero alpha gives the same A)
    return np.array([a0, p1, p2, degenerate, np.zeros_like(a0)])


def lumper_on(cls, sysm, **kw):
    """The reference's lumper carrying T, pi and the stored V as its cached eigensystem."""
    n, m = sysm['n'], sysm['m']
    lumper = cls(n_macrostates=m, verbose=False, **kw)
    lumper.transmat_, lumper.populations_, lumper.n_states_ = sysm['T'], sysm['pi'], n
    lumper.mapping_, lumper.countsmat_ = dict(zip(range(n), range(n))), None
    lumper._right_eigenvectors, lumper._is_dirty = sysm['V'], False
    lumper._do_lumping()
    return lumper


def main():
    warnings.simplefilter("ignore")
    PCCA, PCCAPlus, plus = load()
    kinds = [getattr(plus, k) for k in R.KINDS]
    g = {}
    for name, (n, m, seed) in GOLDEN.items():
        s = R.planted_system(n, m, seed)
        T, pi, V = s['T'], s['pi'], s['V']
        index = plus.index_search(V)
        assert np.array_equal(index, R.index_search(V)), name
        A0 = plus.fill_A(np.linalg.inv(V[index, :]), V)
        flat_map, square_map = plus.get_maps(A0)
        a0 = plus.to_flat(1.0 * A0, flat_map)
        Af, chi0, map0 = plus.calculate_fuzzy_chi(a0, square_map, V)
        fixed = lumper_on(PCCAPlus, s, do_minimization=False)
        assert np.array_equal(fixed.A_, Af) and np.array_equal(fixed.chi_, chi0) and np.array_equal(fixed.microstate_mapping_, map0)
        assert R.same_partition(map0, s['labels']), name
        alphas = listed_alphas(V)
        assert np.allclose(alphas[0], a0, rtol=1e-10, atol=0), name
        alphas[0] = a0                               # (the reference's own bits)
        values = np.zeros((len(alphas), 3))
        with np.errstate(all='ignore'):
            for i, alpha in enumerate(alphas):
                for k in range(3):
                    values[i, k] = kinds[k](alpha, T, V, square_map, pi)
                    want, info = R.objective(k, alpha, T, pi, V)
                    assert np.isinf(values[i, k]) == np.isinf(want), (name, i, k)
                    if np.isfinite(want):
                        margin, bound = R.argmax_margin(info['chi']), R.device_bounds(s, alpha)['chi'].max(axis=1)
                        assert np.all(margin >= 1000 * bound), (name, i, k)
                        assert np.array_equal(info['mapping'], plus.calculate_fuzzy_chi(alpha, square_map, V)[2]), (name, i)
                        assert abs(values[i, k] - float(want)) <= 1e-12 * abs(float(want)), (name, i, k)
        assert np.all(np.isfinite(values[:3])) and np.all(np.isneginf(values[3:])), (name, values)
        coarse = lumper_on(PCCA, s)
        assert np.array_equal(coarse.microstate_mapping_, R.pcca_split(V[:, 1:], m)), name
        g[name + '_V'], g[name + '_index'] = V, np.asarray(index, dtype=np.int32)
        g[name + '_A0'], g[name + '_chi0'], g[name + '_map0'] = Af, chi0, np.asarray(map0, dtype=np.int16)
        g[name + '_pcca'] = np.asarray(coarse.microstate_mapping_, dtype=np.int16)
        g[name + '_alphas'], g[name + '_values'] = alphas, values
        print(name, 'index', index.tolist(), 'values', values[0], 'pcca', np.bincount(g[name + '_pcca']).tolist())
        if name in OPTIMISED:
            maps, finals = [], []
            for k, kind in enumerate(R.KINDS):
                np.random.seed(0)
                best = lumper_on(PCCAPlus, s, objective_function=kind)
                assert R.same_partition(best.microstate_mapping_, s['labels']), (name, kind)
                final = plus.to_flat(best.A_, flat_map)
                maps.append(best.microstate_mapping_)
                finals.append(kinds[k](final, T, V, square_map, pi))
                assert finals[-1] >= values[0, k], (name, kind)
                print('  optimised', kind, values[0, k], '->', finals[-1])
            g[name + '_opt_map'], g[name + '_opt_value'] = np.asarray(maps, dtype=np.int16), np.asarray(finals)
    path = os.path.join(HERE, "pcca_golden.npz")
    np.savez_compressed(path, **g)
    print("pcca_golden.npz:", len(g), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
