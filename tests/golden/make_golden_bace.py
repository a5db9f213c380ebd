#!/usr/bin/env python
"""tests/golden/make_golden_bace.py -- generate bace_golden.npz.

Runs ONLY where the reference tree is present.  The reference's own ``lumping/bace.py`` is imported *by file path* over the
stub modules of make_golden_msm.py (nothing of the reference is copied into this repository) and run through ``from_msm`` on
the seeded count matrices of tests/bace_ref.py (``GOLDEN`` there: inputs are stored as seeds only).  The pair that each
merge picks is recorded by a subclass that wraps ``_mergeTwoClosestStates``; the maps come from ``map_dict``.

Admission.  A case is stored only if the reference, the float64 restatement and the longdouble restatement of bace_ref.py
give the same merge sequence and the same maps, the reference's map holds no negative label, no Bayes factor is NaN, and
the relative gap between the best two stored values is at least 64 float32 ulps (taken as 2^-23: 7.6e-6) at EVERY evaluation, in both
restatements.  ``--search NAME`` prints the first seeds that are admitted for a case.

Also stored: self_heavy_reference_map, the reference's map on ``bace_ref.self_heavy_counts()`` (it holds the label -1).

Stored per case:  _merges (M x 2), _maps (M x n, the map after each merge, n - 1 states downwards), _bayes_keys, _bayes
(float32), _mapping (``microstate_mapping_``; all -1 where the reference leaves it unset), _filter_map, _min_gap.

Usage:  python tests/golden/make_golden_bace.py
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
import bace_ref as R  # noqa: E402

MIN_GAP = 64 * R.F32_ULP


def load():
    MSM = M.load_reference_msm()
    sys.modules["msmbuilder.msm"].MarkovStateModel = MSM
    lump = types.ModuleType("msmbuilder.lumping")
    lump.__path__ = [os.path.join(M.REF, "lumping")]
    sys.modules["msmbuilder.lumping"] = lump
    ref = M._load("msmbuilder.lumping.bace", os.path.join(M.REF, "lumping", "bace.py"), "msmbuilder.lumping")

    class Recording(ref.BACE):
        def _mergeTwoClosestStates(self, c, w, indRecalc, dMat, macro_map, statesKeep, minX, minY, unmerged):
            self.__dict__.setdefault('picked', []).append((int(minX), int(minY)))
            return super(Recording, self)._mergeTwoClosestStates(c, w, indRecalc, dMat, macro_map, statesKeep, minX, minY, unmerged)

    return MSM, Recording


def run_reference(MSM, BACE, spec):
    n = spec['n']
    msm = MSM(verbose=False, lag_time=spec.get('lag_time', 1), sliding_window=spec.get('sliding_window', True))
    msm.transmat_, msm.populations_ = None, np.full(n, 1.0 / n)
    msm.mapping_, msm.countsmat_, msm.n_states_ = dict(zip(range(n), range(n))), R.golden_counts(spec), n
    with np.errstate(all='ignore'):
        return BACE.from_msm(msm, spec['n_macrostates'], filter=spec['filter'])


def admit(MSM, BACE, spec, verbose=False):
    """The arrays of one case, or a string saying why it is not admitted."""
    n, nm = spec['n'], spec['n_macrostates']
    lumped = run_reference(MSM, BACE, spec)
    picked = getattr(lumped, 'picked', [])
    counts = R.golden_counts(spec)
    kw = dict(filt=spec['filter'], lag_time=spec.get('lag_time', 1), sliding_window=spec.get('sliding_window', True))
    try:
        narrow, wide = R.bace(counts, nm, **kw), R.bace(counts, nm, wide=True, **kw)
    except ValueError as e:
        return 'restatement: %s' % e
    if not (picked == narrow['merges'] == wide['merges']):
        return 'merge sequences differ'
    left = sorted(lumped.map_dict, reverse=True)
    if left != sorted(narrow['maps'], reverse=True):
        return 'map_dict keys differ'
    maps = np.array([lumped.map_dict[k] for k in left], dtype=np.int64).reshape(len(left), n)
    if maps.size and maps.min() < 0:
        return 'the reference produced a negative label'
    for r in (narrow, wide):
        if any(not np.array_equal(lumped.map_dict[k], r['maps'][k]) for k in left):
            return 'maps differ'
    keys = sorted(lumped.bayesFactors, reverse=True)
    bayes = np.array([lumped.bayesFactors[k] for k in keys], dtype=np.float32)
    if np.isnan(bayes).any():
        return 'NaN Bayes factor'
    if keys != sorted(narrow['bayes'], reverse=True):
        return 'bayesFactors keys differ'
    gap = min(min(narrow['gaps']), min(wide['gaps']))
    if not gap >= MIN_GAP:
        return 'gap %.3g' % gap
    ours = np.array([narrow['bayes'][k] for k in keys], dtype=np.float32)
    with np.errstate(all='ignore'):
        off = np.abs(ours.astype(np.float64) - bayes) / np.abs(bayes)
    if not np.all((off <= 2 * R.F32_ULP) | (ours == bayes)):
        return 'Bayes factors differ by %.3g' % np.nanmax(off)
    mapping = np.asarray(lumped.microstate_mapping_) if hasattr(lumped, 'microstate_mapping_') else np.full(n, -1)
    if verbose:
        print('   kept', len(narrow['keep']), 'merges', len(picked), 'min gap %.3g' % gap, 'final', np.bincount(narrow['mapping']).tolist())
    return dict(merges=np.array(picked, dtype=np.int32).reshape(len(picked), 2), maps=maps.astype(np.int16), bayes_keys=np.array(keys, dtype=np.int32),
                bayes=bayes, mapping=mapping.astype(np.int16), filter_map=narrow['filter_map'].astype(np.int16), min_gap=np.float64(gap))


def main():
    warnings.simplefilter("ignore")
    MSM, BACE = load()
    if len(sys.argv) > 2 and sys.argv[1] == '--search':
        spec = dict(R.GOLDEN[sys.argv[2]])
        found = []
        for seed in range(200):
            spec['seed'] = seed
            got = admit(MSM, BACE, spec)
            print(seed, got if isinstance(got, str) else 'admitted, min gap %.3g, kept %d' % (got['min_gap'], len(np.unique(got['filter_map']))))
            found += [] if isinstance(got, str) else [seed]
            if len(found) >= 3:
                break
        return
    g = {}
    for name, spec in R.GOLDEN.items():
        print(name, spec)
        got = admit(MSM, BACE, spec, verbose=True)
        if isinstance(got, str):
            raise SystemExit('%s is not admitted: %s' % (name, got))
        for key, value in got.items():
            g['%s_%s' % (name, key)] = value
    # difference (d): what the reference makes of a pruned state whose largest count is its own self-transition
    n = len(R.self_heavy_counts())
    msm = MSM(verbose=False)
    msm.transmat_, msm.populations_ = None, np.full(n, 1.0 / n)
    msm.mapping_, msm.countsmat_, msm.n_states_ = dict(zip(range(n), range(n))), R.self_heavy_counts(), n
    heavy = BACE.from_msm(msm, n - 2, filter=1.1)
    g["self_heavy_reference_map"] = np.asarray(heavy.map_dict[max(heavy.map_dict)]).astype(np.int16)
    print("self_heavy: the reference's map", g["self_heavy_reference_map"].tolist())
    assert g["self_heavy_reference_map"].min() == -1
    path = os.path.join(HERE, "bace_golden.npz")
    np.savez_compressed(path, **g)
    print("bace_golden.npz:", len(g), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
