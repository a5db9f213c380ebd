"""CPU tier of MarkovStateModel: the golden script's numpy MLE, the host-side trimming / mapping helpers against
the goldens, and the C ABI symbols."""
import os
import sys

import numpy as np

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_msm as G  # noqa: E402


def test_numpy_mle_certificates():
    for C in (G.well_counts(200, 1), G.well_counts(60, 2) + 0.5):
        T, pi, it = G.mle_numpy(C)
        assert it < 100000
        assert G.kkt_residual(C, pi) <= 1e-13
        flux = pi[:, None] * T
        assert np.abs(flux - flux.T).max() <= 1e-14 * flux.max()
        np.testing.assert_allclose(T.sum(1), 1.0, atol=1e-14)
        # the MLE beats a perturbed reversible matrix in likelihood
        nz = C > 0
        ll = (C[nz] * np.log(T[nz])).sum()
        X = pi[:, None] * T * (1 + 1e-3 * np.sin(np.add.outer(np.arange(len(pi)), np.arange(len(pi)))))
        T2 = X / X.sum(1)[:, None]
        assert ll >= (C[nz] * np.log(T2[nz])).sum()


def _raw_counts(seqs, lag):
    classes = np.unique(np.concatenate(seqs))
    idx = {c: i for i, c in enumerate(classes)}
    C = np.zeros((len(classes), len(classes)))
    for y in seqs:
        s = np.array([idx[v] for v in y])
        np.add.at(C, (s[:-lag], s[lag:]), 1.0)
    return C / lag, dict(zip(classes, range(len(classes))))


def test_trimming_matches_golden():
    from msmbuilder_amd.msm.msm import _strongly_connected_subgraph, _dict_compose, MarkovStateModel
    g = np.load(os.path.join(GOLDEN, "msm_golden.npz"))
    cases = G.cases()
    for name in ("cut_on", "cut_num", "cut_num4", "disconnected"):
        seqs, params, _ = cases[name]
        m = MarkovStateModel(**params)
        raw, mapping = _raw_counts(seqs, params['lag_time'])
        counts, mapping2, pct = _strongly_connected_subgraph(raw, m._parse_ergodic_cutoff(), verbose=False)
        full = _dict_compose(mapping, mapping2)
        assert np.array_equal(counts, g[name + "_countsmat"])
        assert np.array_equal(np.array(list(full.keys())), g[name + "_keys"])
        assert np.array_equal(np.array(list(full.values())), g[name + "_vals"])
        assert pct == float(g[name + "_percent"])


def test_trimming_verbose_line(capsys):
    from msmbuilder_amd.msm.msm import _strongly_connected_subgraph
    C = np.array([[2.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 0.0, 0.0]])
    _strongly_connected_subgraph(C, 1.0, verbose=True)
    assert capsys.readouterr().out == ("MSM contains 2 strongly connected components above weight=1.00. "
                                       "Component 1 selected, with population 87.500000%\n")


def test_cabi_symbols():
    from msmbuilder_amd import _lib
    L = _lib.lib()
    for name in ("msm_transmat_mle", "msm_mle_last_stats", "msm_syev_top"):
        assert hasattr(L, name)


def test_numpy_mle_error_messages():
    import pytest
    for C, msg in (([[1.0, -0.5], [1.0, 1.0]], "Domain error. C must be positive. Error code=-2"),
                   ([[0.0, 0.0], [1.0, 1.0]], "Row-sums of C must be positive. Error code=-1"),
                   ([[1.0, -1.0], [1.0, 1.0]], "Row-sums of C must be positive.Domain error. C must be positive. Error code=-1")):
        with pytest.raises(ValueError) as e:
            G.mle_numpy(np.array(C))
        assert str(e.value) == msg
