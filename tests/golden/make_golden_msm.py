#!/usr/bin/env python
"""tests/golden/make_golden_msm.py -- golden vectors of MarkovStateModel -> msm_golden.npz.

Runs only where the reference package is available.  Like make_golden.py it imports the reference's own
``msm/msm.py`` and ``msm/core.py`` by file path (nothing of the reference is copied here), with stub modules
for ``mdtraj`` and the compiled ``_ratematrix``.  The compiled ``_markovstatemodel._transmat_mle_prinz`` is
replaced by ``mle_numpy`` below: the same reversible maximum-likelihood estimator, solved as an
Anderson-accelerated fixed point on the populations until max|g(x) - x| / max g(x) < 1e-14 (KKT residual
<= 1e-13 asserted), so the fixtures pin the reference's Python semantics -- trimming, mapping_,
percent_retained_, the 'transpose' and None estimators, eigenvector normalisation, timescales, GMRQ score,
summarize() -- on an MLE converged far beyond the reference's own 1e-10 log-likelihood stopping rule.

``mle_numpy``, ``kkt_residual`` and the case generators import without the reference (tests/test_msm_host.py).

Usage:  python tests/golden/make_golden_msm.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/msmbuilder"


def g_map(Cs, c, x):
    """g_i(x) = sum_j Cs_ij / (d_i + d_j), d = c / x."""
    d = c / x
    return (Cs / (d[:, None] + d[None, :])).sum(1)


def kkt_residual(C, pi):
    """Stationarity residual of the reversible likelihood at populations pi: max|g(pi) - pi| / max pi (scale-free)."""
    C = np.asarray(C, dtype=float)
    return np.abs(g_map(C + C.T, C.sum(1), pi) - pi).max() / pi.max()


def mle_numpy(C, tol=1e-14, m=6, max_iter=100000, stats=None):
    """Reversible MLE of the counts C: (T, pi, iterations).  Fixed point x = g(x) on the simplex, Anderson mixing
    over m iterates (normal equations, no ridge), plain step whenever a mixed one is not positive.  ``stats`` (a dict)
    receives the counts of mixed steps accepted, rejected as non-positive, and solves rejected as singular."""
    if stats is not None:
        stats.update(accepted=0, nonpositive=0, singular=0)
    C = np.asarray(C, dtype=float)
    if C.shape[0] == 0:
        return np.zeros((0, 0)), np.zeros(0), 0
    Cs = C + C.T
    c = C.sum(1)
    rows_bad = np.any(c <= 0) or np.any(Cs.sum(1) <= 0)
    msg = ' Error code=-1' if rows_bad else ' Error code=-2'
    if rows_bad or np.any(C < 0):
        if np.any(C < 0):
            msg = 'Domain error. C must be positive.' + msg
        if np.any(c == 0):
            msg = 'Row-sums of C must be positive.' + msg
        raise ValueError(msg)
    x = Cs.sum(1)
    x = x / x.sum()
    dF, dG, Fp, Gp = [], [], None, None
    for it in range(max_iter + 1):
        g = g_map(Cs, c, x)
        if np.abs(g - x).max() / g.max() < tol:
            break
        if it == max_iter:
            raise ValueError('Likelihood not converged. Error code=-3')
        G = g / g.sum()
        F = G - x
        if Fp is not None:
            dF.append(F - Fp)
            dG.append(G - Gp)
            if len(dF) > m:
                dF.pop(0)
                dG.pop(0)
        Fp, Gp = F, G
        x = G
        if dF:
            A = np.array(dF).T
            M = A.T @ A
            try:
                gam = np.linalg.solve(M, A.T @ F)
            except np.linalg.LinAlgError:
                if stats is not None:
                    stats['singular'] += 1
                continue
            xn = G - np.array(dG).T @ gam
            if np.all(xn > 0) and np.all(np.isfinite(xn)):
                x = xn / xn.sum()
                if stats is not None:
                    stats['accepted'] += 1
            elif stats is not None:
                stats['singular' if not np.all(np.isfinite(gam)) else 'nonpositive'] += 1
    d = c / x
    X = Cs / (d[:, None] + d[None, :])
    rs = X.sum(1)
    return X / rs[:, None], rs / rs.sum(), it


# ---- inputs --------------------------------------------------------------------------------------------------------
def metastable_labels(rs, n, k, stay=0.97):
    y = np.empty(n, dtype=np.int64)
    y[0] = rs.randint(k)
    for t in range(1, n):
        y[t] = y[t - 1] if rs.rand() < stay else rs.randint(k)
    return y


def well_chain(n_states, n_steps, seed, wells=4, amp=1.5):
    """Metropolis walk (jumps of up to 4 states) on a 1-D landscape of `wells` wells: a metastable chain."""
    rs = np.random.RandomState(seed)
    E = 2 * amp * np.cos(2 * np.pi * wells * np.linspace(0, 1, n_states))
    y = np.empty(n_steps, np.int64)
    s = n_states // 2
    steps = rs.randint(-4, 5, n_steps)
    u = rs.rand(n_steps)
    for t in range(n_steps):
        j = min(max(s + steps[t], 0), n_states - 1)
        if u[t] < np.exp(-(E[j] - E[s])):
            s = j
        y[t] = s
    return y


def well_counts(n_states, seed, stay=0.98, width=3, wells=4):
    """Banded metastable count matrix of n_states states (no trajectory): transitions within `width` states, rare
    hops between `wells` blocks; every row positive, symmetric pattern."""
    rs = np.random.RandomState(seed)
    C = np.zeros((n_states, n_states))
    block = n_states // wells
    for i in range(n_states):
        for j in range(max(0, i - width), min(n_states, i + width + 1)):
            same = (i // block) == (j // block)
            C[i, j] = rs.poisson(200 if same else 1) + (1 if i == j else 0)
    return C


def ring_links(K, deg, seed):
    """Well-mixed asymmetric counts: a ring (self and +-1, poisson(20) + 1 each) plus `deg` random links per row
    (poisson(3) each)."""
    rs = np.random.RandomState(seed)
    C = np.zeros((K, K))
    idx = np.arange(K)
    for off in (-1, 0, 1):
        np.add.at(C, (idx, (idx + off) % K), rs.poisson(20, K) + 1.0)
    for _ in range(deg):
        np.add.at(C, (idx, rs.randint(0, K, K)), rs.poisson(3, K).astype(float))
    return C


def hub(K, seed):
    """ring_links plus one state linked to every other in both directions: its row of the pattern has K entries
    (its 64-row slice is padded to that width) while the others keep about 5."""
    rs = np.random.RandomState(seed + 1000)
    C = ring_links(K, 3, seed)
    h = int(rs.randint(K))
    C[h, :] += rs.poisson(2, K) + 1.0
    C[:, h] += rs.poisson(2, K) + 1.0
    return C


def ragged(K, seed):
    """Row lengths between 2 and 200 that differ widely between and inside 64-row slices: runs of 1..96 rows (not
    aligned to the slices) draw a ceiling from {2, .., 200}, each row of a run a length up to that ceiling, and the
    symmetric pattern with about those row lengths is a random pairing of that many stubs per row (duplicate pairs
    merge); a thin ring keeps the chain irreducible."""
    rs = np.random.RandomState(seed)
    top = min(200, K - 1)
    L = np.empty(K, np.int64)
    i = 0
    while i < K:
        run = int(rs.randint(1, 97))
        ceil_ = int(rs.randint(2, top + 1))
        L[i:i + run] = rs.randint(2, ceil_ + 1, len(L[i:i + run]))
        i += run
    stubs = rs.permutation(np.repeat(np.arange(K), L))
    a, b = stubs[0:len(stubs) // 2 * 2:2], stubs[1:len(stubs) // 2 * 2:2]
    C = np.zeros((K, K))
    np.add.at(C, (a, b), rs.poisson(5, len(a)) + 1.0)
    np.add.at(C, (b, a), rs.poisson(5, len(a)) + 1.0)
    idx = np.arange(K)
    np.add.at(C, (idx, (idx + 1) % K), rs.poisson(2, K) + 1.0)
    np.add.at(C, ((idx + 1) % K, idx), rs.poisson(2, K) + 1.0)
    return C


def wide_range(K, seed, decades=10.0):
    """Fractional asymmetric counts of a Metropolis-like walk (jumps of up to 2 states) on a 1-D slope whose
    equilibrium populations span `decades` decades: C_ij = N pi_i min(1, pi_j / pi_i) (1 + noise)."""
    rs = np.random.RandomState(seed)
    logp = -np.log(10.0) * decades * np.arange(K) / max(K - 1, 1)
    C = np.zeros((K, K))
    for i in range(K):
        for j in range(max(0, i - 2), min(K, i + 3)):
            C[i, j] = 1e6 * np.exp(logp[i] + min(0.0, logp[j] - logp[i])) * (1.0 + 0.3 * rs.rand())
    return C


def star(K, seed):
    """One centre with few counts out to and many counts in from every other state, and self counts over six decades:
    the start (row sums of C + C^T) is far from the solution, and mle_numpy rejects mixed steps as non-positive."""
    rs = np.random.RandomState(seed)
    C = np.zeros((K, K))
    C[0, 1:] = rs.poisson(5, K - 1) + 1
    C[1:, 0] = rs.poisson(500, K - 1) + 1
    C[np.arange(K), np.arange(K)] = rs.poisson(1000, K) * rs.rand(K) ** 4 + 1e-3
    return C


def blocks(sizes, seed):
    """Block-diagonal (reducible) counts: one ring_links block per size; a block of size 1 is a self-looping state."""
    K = int(np.sum(sizes))
    C = np.zeros((K, K))
    o = 0
    for b, n in enumerate(sizes):
        C[o:o + n, o:o + n] = ring_links(n, 2, seed + b)
        o += n
    return C


def cases():
    """name -> (sequences, params, score_sequences)."""
    rs = np.random.RandomState(42)
    ala = [metastable_labels(rs, 9999, 5, 0.99) for _ in range(10)]
    out = {
        'ala': (ala, dict(lag_time=1), [metastable_labels(rs, 3000, 5, 0.99)]),
        'ala_lag5_prior': (ala, dict(lag_time=5, prior_counts=0.5, n_timescales=2), None),
        'ala_transpose': (ala, dict(lag_time=2, reversible_type='transpose'), None),
        'ala_none': (ala, dict(lag_time=2, reversible_type=None), None),
        'nosw': (ala, dict(lag_time=3, sliding_window=False), None),
    }
    ys = np.array(['s%02d' % v for v in metastable_labels(rs, 4000, 6, 0.95)])
    out['strings'] = ([ys], dict(lag_time=1), None)
    yf = metastable_labels(rs, 5000, 7, 0.95).astype(float)
    yf[rs.randint(0, 5000, 80)] = np.nan
    out['nan'] = ([yf, yf[:300]], dict(lag_time=2), None)
    # a trimmed tail: states 20..22 visited once on the way in, never left in both directions
    y = metastable_labels(rs, 6000, 8, 0.95)
    y2 = np.concatenate([y, [20, 21, 22]])
    out['cut_on'] = ([y2], dict(lag_time=1), None)
    out['cut_off'] = ([y2], dict(lag_time=1, ergodic_cutoff='off', prior_counts=0.5), None)
    out['cut_num'] = ([y], dict(lag_time=1, ergodic_cutoff=40.0), None)
    out['cut_num4'] = ([y], dict(lag_time=1, ergodic_cutoff=4.0), None)
    # two disconnected halves: the more populated is kept
    a = metastable_labels(rs, 3000, 4, 0.9)
    b = metastable_labels(rs, 2000, 3, 0.9) + 10
    out['disconnected'] = ([a, b], dict(lag_time=1, n_timescales=2), None)
    out['meta299'] = ([well_chain(299, 400000, 1)], dict(lag_time=1, n_timescales=10, verbose=False), None)
    # a state without counts (its only sequence is shorter than the lag) kept by ergodic_cutoff='off': the 'transpose'
    # estimator divides by its zero row sum, and the reference's eigensolver refuses the non-finite matrix
    rs2 = np.random.RandomState(77)
    out['transpose_zero'] = ([metastable_labels(rs2, 3000, 5, 0.9), np.array([9])],
                             dict(lag_time=2, reversible_type='transpose', ergodic_cutoff='off'), None)
    return out


# ---- reference loading -----------------------------------------------------------------------------------------
def _load(name, path, package=None):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference_msm():
    for alias, typ in (("int", int), ("float", float)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)
    md = types.ModuleType("mdtraj")
    md.Trajectory = type("Trajectory", (object,), {})
    sys.modules["mdtraj"] = md
    pkg = types.ModuleType("msmbuilder")
    pkg.__path__ = [REF]
    sys.modules["msmbuilder"] = pkg
    _load("msmbuilder.base", os.path.join(REF, "base.py"), "msmbuilder")
    utils = types.ModuleType("msmbuilder.utils")
    utils.__path__ = [os.path.join(REF, "utils")]
    sys.modules["msmbuilder.utils"] = utils
    val = _load("msmbuilder.utils.validation", os.path.join(REF, "utils", "validation.py"), "msmbuilder.utils")
    utils.list_of_1d = val.list_of_1d
    msm = types.ModuleType("msmbuilder.msm")
    msm.__path__ = [os.path.join(REF, "msm")]
    sys.modules["msmbuilder.msm"] = msm
    sys.modules["msmbuilder.msm._ratematrix"] = types.ModuleType("msmbuilder.msm._ratematrix")
    stub = types.ModuleType("msmbuilder.msm._markovstatemodel")

    def _transmat_mle_prinz(C, tol=1e-10):
        T, pi, _ = mle_numpy(np.asarray(C))
        if T.shape[0]:
            assert kkt_residual(np.asarray(C), pi) <= 1e-13
        return T, pi
    stub._transmat_mle_prinz = _transmat_mle_prinz
    sys.modules["msmbuilder.msm._markovstatemodel"] = stub
    _load("msmbuilder.msm.core", os.path.join(REF, "msm", "core.py"), "msmbuilder.msm")
    return _load("msmbuilder.msm.msm", os.path.join(REF, "msm", "msm.py"), "msmbuilder.msm").MarkovStateModel


def main():
    import warnings
    MSM = load_reference_msm()
    g = {}
    for name, (seqs, params, score_seqs) in cases().items():
        p = dict(params)
        p.setdefault('verbose', False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = MSM(**p).fit(seqs)
            try:
                m.eigenvalues_
            except ValueError as e:   # the fit stands, the eigensystem is refused: the message is the fixture
                eig_error = str(e)
            else:
                eig_error = None
        g[name + '_countsmat'] = m.countsmat_
        keys = list(m.mapping_.keys())
        g[name + '_keys'] = np.array(keys)
        g[name + '_vals'] = np.array([m.mapping_[k] for k in keys], dtype=np.int64)
        g[name + '_n_states'] = np.int64(m.n_states_)
        g[name + '_percent'] = np.float64(m.percent_retained_)
        g[name + '_transmat'] = m.transmat_
        g[name + '_populations'] = m.populations_
        if eig_error is not None:
            g[name + '_eig_error'] = np.array(eig_error)
            print(name, m.n_states_, m.percent_retained_, 'eigensystem:', eig_error)
            continue
        g[name + '_eigenvalues'] = np.real(m.eigenvalues_)
        g[name + '_lv'] = np.real(m.left_eigenvectors_)
        g[name + '_rv'] = np.real(m.right_eigenvectors_)
        g[name + '_timescales'] = np.real(m.timescales_)
        g[name + '_score_'] = np.float64(np.real(m.score_))
        g[name + '_summary'] = np.array(m.summarize())
        if score_seqs is not None:
            g[name + '_score'] = np.float64(np.real(m.score(score_seqs)))
        print(name, m.n_states_, m.percent_retained_, m.timescales_[:3])
    np.savez_compressed(os.path.join(HERE, "msm_golden.npz"), **g)
    print("msm_golden.npz:", len(g), "arrays,", os.path.getsize(os.path.join(HERE, "msm_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
