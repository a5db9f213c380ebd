"""tests/hmm_ref.py -- the Gaussian HMM restated in numpy from its formulas, the case generators of the HMM tests and the
rounding bound they hold the device to.

Every function takes ``dt``: ``np.longdouble`` is the yardstick, ``np.float64`` with ``form='expanded'`` is the
reference's own arithmetic (log-space recursions with a max-shifted log-sum-exp, the emission term as
``a0 + x (a1 + x a2)``).  float32 rows are widened exactly in both; ``form='reference'`` is 'expanded' with the one
place where the reference does not widen first: the product x * x of obs**2 is formed in the rows' type.

The model: K states, diagonal Gaussians (means, vars: K x F), transition matrix A (clamped at 1e-20 before its logarithm),
and a vector ``lsp`` that is ADDED to the first frame's log likelihoods (the reference hands 1 / K there).  ``log(2 pi)``
is the float32-rounded constant of the reference in every arithmetic, so that only rounding differs.
"""
import os
import sys

import numpy as np

LOG_2PI_F32 = np.float32(np.log(2 * np.pi))
U = 2.0 ** -53
SQRT_U = 2.0 ** -26.5
CLAMP = 1e-20


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def loglik(X, means, vars, dt=np.longdouble, form='centred'):
    """[T, K] emission log-likelihoods."""
    x = np.asarray(X).astype(dt)[:, None, :]
    m = np.asarray(means, dtype=np.float64).astype(dt)[None]
    v = np.asarray(vars, dtype=np.float64).astype(dt)[None]
    F = x.shape[2]
    c = dt(LOG_2PI_F32)
    temp = np.zeros((x.shape[0], m.shape[1]), dtype=dt)
    if form in ('expanded', 'reference'):
        a0 = m * m / v + np.log(v)
        a1 = dt(-2.0) * m / v
        a2 = dt(1.0) / v
        for f in range(F):   # the reference's order
            temp = temp + (a0[:, :, f] + x[:, :, f] * (a1[:, :, f] + x[:, :, f] * a2[:, :, f]))
    else:
        for f in range(F):
            d = x[:, :, f] - m[:, :, f]
            temp = temp + (d * d / v[:, :, f] + np.log(v[:, :, f]))
    return dt(-0.5) * (dt(F) * c + temp)


def _lse(a, axis):
    mx = a.max(axis=axis, keepdims=True)
    return (np.log(np.exp(a - mx).sum(axis=axis, keepdims=True)) + mx).squeeze(axis)


def log_transmat(transmat, dt):
    return np.log(np.maximum(np.asarray(transmat, dtype=np.float64), CLAMP).astype(dt))


def forward(ll, logA, lsp):
    T, K = ll.shape
    fwd = np.empty_like(ll)
    fwd[0] = lsp + ll[0]
    for t in range(1, T):
        fwd[t] = _lse(fwd[t - 1][:, None] + logA, 0) + ll[t]
    return fwd


def backward(ll, logA):
    T, K = ll.shape
    bwd = np.zeros_like(ll)
    for t in range(T - 2, -1, -1):
        bwd[t] = _lse(logA + (ll[t + 1] + bwd[t + 1])[None, :], 1)
    return bwd


def estep(seqs, means, vars, transmat, lsp, dt=np.longdouble, form='centred'):
    """The E-step's sums over a list of trajectories: dict of traj_logprob, post, obs, obs**2, trans, logprob."""
    K = np.asarray(means).shape[0]
    F = np.asarray(means).shape[1]
    logA = log_transmat(transmat, dt)
    lsp = np.asarray(lsp, dtype=np.float64).astype(dt)
    post = np.zeros(K, dtype=dt)
    obs = np.zeros((K, F), dtype=dt)
    obs2 = np.zeros((K, F), dtype=dt)
    trans = np.zeros((K, K), dtype=dt)
    tl = []
    for X in seqs:
        ll = loglik(X, means, vars, dt, form)
        fwd = forward(ll, logA, lsp)
        bwd = backward(ll, logA)
        lp = _lse(fwd[-1], 0)
        g = fwd + bwd
        gamma = np.exp(g - _lse(g, 1)[:, None])
        if len(X) > 1:
            w = fwd[:-1, :, None] + logA[None] + (ll[1:] + bwd[1:])[:, None, :] - lp
            trans += np.exp(_lse(w, 0))
        x = np.asarray(X).astype(dt)
        post += gamma.sum(0)
        obs += gamma.T @ x
        # (the reference multiplies x * x in the rows' own type before widening: form='reference' keeps that)
        obs2 += gamma.T @ ((np.asarray(X) * np.asarray(X)).astype(dt) if form == 'reference' else x * x)
        tl.append(lp)
    tl = np.array(tl, dtype=dt)
    return {'traj_logprob': tl, 'post': post, 'obs': obs, 'obs**2': obs2, 'trans': trans, 'logprob': tl.sum()}


def viterbi(X, means, vars, transmat, lsp, dt=np.float64, form='expanded'):
    """(log probability, int32 states): the induction and the traceback both take the FIRST maximum."""
    ll = loglik(X, means, vars, dt, form)
    logA = log_transmat(transmat, dt)
    lsp = np.asarray(lsp, dtype=np.float64).astype(dt)
    T, K = ll.shape
    lat = np.empty_like(ll)
    lat[0] = lsp + ll[0]
    for t in range(1, T):
        lat[t] = (lat[t - 1][:, None] + logA).max(0) + ll[t]
    states = np.empty(T, dtype=np.int32)
    states[-1] = int(np.argmax(lat[-1]))   # numpy's argmax is the first maximum
    lp = lat[-1][states[-1]]
    for t in range(T - 2, -1, -1):
        states[t] = int(np.argmax(lat[t] + logA[:, states[t + 1]]))
    return lp, states


def path_logprob(X, states, means, vars, transmat, lsp, dt=np.longdouble):
    """Joint log probability of the rows and one state path."""
    ll = loglik(X, means, vars, dt)
    logA = log_transmat(transmat, dt)
    s = np.asarray(states)
    t = np.arange(len(s))
    return dt(np.asarray(lsp, dtype=np.float64)[s[0]]) + ll[t, s].sum() + logA[s[:-1], s[1:]].sum()


def viterbi_optimum(X, means, vars, transmat, lsp, dt=np.longdouble):
    return viterbi(X, means, vars, transmat, lsp, dt, 'centred')[0]


# ------------------------------------------------------------------------------------------------------------------
# M-step and EM loop (float64 on K x F and K x K objects, as the estimator has them)
# ------------------------------------------------------------------------------------------------------------------
MERGE = 1e-10


def lqa_system(post, vars_f, weights):
    """The normal equations of one feature's local quadratic approximation, assembled pair by pair.  The objective
        sum_k (post_k mu_k^2 / 2 - obs_k mu_k) / var_k + sum_{k<j} w_kj (mu_k - mu_j)^2 / 2
    has the gradient (D + sum_{k<j} w_kj (e_k - e_j)(e_k - e_j)^T) mu - obs / var, D = diag(post / var)."""
    K = len(post)
    M = np.zeros((K, K))
    for k in range(K):
        for j in range(k + 1, K):
            w = weights[k, j]
            M[k, k] += w
            M[j, j] += w
            M[k, j] -= w
            M[j, k] -= w
    for k in range(K):
        M[k, k] += post[k] / vars_f[k]
    return M


def mstep(stats, vars_old, mle, reversible_type='mle', fusion_prior=1e-2, n_lqa_iter=10, vars_prior=1e-3, vars_weight=1):
    """New (means, vars, transmat, populations) from the E-step's sums, written from the model's formulas.

    Transition matrix: the reversible maximum-likelihood estimate ``mle(counts) -> (T, pi)`` of the expected counts
    floored at 1e-20, or the symmetrised counts row-normalised.  Means: the minimiser of the expected complete-data
    negative log likelihood plus the L1 fusion penalty ``fusion_prior sum_{k<j} |mu_k - mu_j|`` per feature, by up to
    ``n_lqa_iter`` steps of local quadratic approximation |d| ~ d^2 / (2 |d_now|) with the prior divided by the gap of
    the unpenalised means (gaps floored at 1e-10); a singular step ends the iteration after its sweep; pairs whose gap
    before the last step was at the floor are merged.  Variances: (vars_prior + sum gamma (x - mu)^2) /
    (max(vars_weight - 1, 0) + sum gamma), the posterior weight padded by 10 float32 epsilons."""
    xi = np.asarray(stats['trans'], dtype=np.float64)
    post = np.asarray(stats['post'], dtype=np.float64)
    obs = np.asarray(stats['obs'], dtype=np.float64)
    obs2 = np.asarray(stats['obs**2'], dtype=np.float64)
    K, F = obs.shape
    if reversible_type == 'mle':
        transmat, pops = mle(np.maximum(np.nan_to_num(xi), 1e-20))
    else:
        sym = np.maximum(xi + xi.T, 1e-20)
        pops = sym.sum(0) / sym.sum()
        transmat = sym / sym.sum(1)[:, None]
    mass = post + 10 * np.finfo(np.float32).eps
    means = obs / mass[:, None]
    if fusion_prior > 0 and n_lqa_iter > 0:
        def gap(mu_f):
            return np.maximum(np.abs(mu_f[:, None] - mu_f[None, :]), MERGE)
        lam = [fusion_prior / gap(means[:, f]) for f in range(F)]
        seen, singular = None, False
        for step in range(n_lqa_iter):
            seen = [gap(means[:, f]) for f in range(F)]
            if singular or all(np.all(g <= MERGE) for g in seen):
                break
            for f in range(F):
                if np.all(seen[f] <= MERGE):
                    continue
                M = lqa_system(post, vars_old[:, f], lam[f] / seen[f])
                try:
                    means[:, f] = np.linalg.solve(M, obs[:, f] / vars_old[:, f])
                except np.linalg.LinAlgError:
                    singular = True
        for f in range(F):
            for k in range(K):
                for j in range(k + 1, K):
                    if seen[f][k, j] <= MERGE:
                        means[k, f] = means[j, f]
    if vars_prior is None:
        vars_prior, vars_weight = 0.0, 0.0
    scatter = obs2 - 2 * means * obs + means ** 2 * mass[:, None]
    return means, (vars_prior + scatter) / (max(vars_weight - 1, 0) + mass[:, None]), transmat, pops


def em(seqs, start, mle, n_iter, thresh=1e-2, dt=np.float64, form='expanded', perturb=None, **mkw):
    """One EM run from ``start = (means, vars, transmat, populations)``: E-step, log probability, stop when it moved by
    less than ``thresh`` (kept as a float32) from the second iteration on, otherwise M-step.  Returns the parameters the
    last E-step ran with or the last M-step produced, and the log probabilities the M-steps recorded.  ``perturb(stats,
    iteration)`` may alter the sums before the M-step sees them (golden_amplification)."""
    means, vars, transmat, pops = [np.array(a, dtype=np.float64) for a in start]
    K = means.shape[0]
    lsp = np.tile(1.0 / K, K)
    thresh = float(np.float32(thresh))
    logs, recorded = [], []
    for i in range(n_iter):
        st = estep(seqs, means, vars, transmat, lsp, dt, form)
        logs.append(float(st['logprob']))
        if i > 0 and abs(logs[i] - logs[i - 1]) < thresh:
            break
        recorded = list(logs)
        if perturb is not None:
            st = perturb(st, i)
        means, vars, transmat, pops = mstep(st, vars, mle, **mkw)
    return (means, vars, transmat, pops), np.array(recorded)


def mle_solver():
    """The numpy reversible-MLE solver the MSM goldens were made with: counts -> (T, pi)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_msm
    def solve(counts):
        out = make_golden_msm.mle_numpy(np.asarray(counts, dtype=np.float64))
        return out[0], out[1]
    return solve


# ------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------
# The device runs the scaled LINEAR recursion: alpha_t = (alpha_{t-1} A) o b_t / n_t and its mirror for beta, with
# b_t(k) = exp(l_t(k) - max_k l_t(k)), also in the associated form (K x K products per segment, then a sweep over them).
# Every quantity in it is a sum of products of NON-NEGATIVE numbers, so there is no cancellation and rounding enters
# componentwise: a computed value is the exact one times a product of (1 + d_i), |d_i| <= u = 2^-53, one factor per
# floating-point operation on the longest path that leads to it.  Per frame that path has at most
#     K - 1 additions and 1 multiplication of the K-term dot product, the product with b_t, the division by n_t
#     (K + 2 operations), once in the segment's operator and once in the pass through the segment, plus one more
#     K + 1 per segment for the stitch:                                         at most 2 K + 6 operations per frame,
# and the relative error e_t of b_t itself: exp() (2 u) and the absolute error of l_t(k) - max.  The emission term is a
# sum of F three-operation terms and a constant; any evaluation that is at least as accurate as the reference's
# a0 + x (a1 + x a2) satisfies  |dl_t(k)| <= (F + 6) u E_t,
#     E_t = max_k [ sum_f ((|x| + |mu|)^2 / var + |log var|) / 2 ] + F log(2 pi) / 2
# (the magnitude of the terms the expanded form adds; the centred form the device uses adds smaller ones).  A state far
# from the frame has a large |dl| but a weight exp(-d) that outruns it (d e^-d <= 1), so E_t bounds the weighted error.
# b_t enters alpha_t' for t' >= t and beta_t' for t' < t, never both, so alpha_t(k) beta_t(k) carries every frame's
# errors once, and normalising to gamma_t doubles the bound:
#     |d gamma_t(k)| / gamma_t(k)  <=  rho(T) = 2 T ((2 K + 6) u + (F + 6) u E + 3 u),     E = max_t E_t,
# linear in the trajectory length T and in K.  xi_t(i, j) is one more product of the same factors: the same rho.
# The sums over frames add (N + 2) u for N terms of one sign.  So, relative to each quantity's scale
#     post: N        trans: N - n_traj        obs[., f]: sum_t |x_t(f)|        obs**2[., f]: sum_t x_t(f)^2
# the bound is  rel = rho(T_max) + (N + 2) u + underflow + logspace.
# Log space: the bound must be no tighter than what the reference's own arithmetic achieves, and that arithmetic keeps its
# lattices as logarithms: an entry of magnitude up to Lmax = max |fwd_t(k)| is rounded at u Lmax ABSOLUTE by every
# addition that forms it, which is a relative u Lmax of the weight it stands for; four such entries make a xi term and
# the roundings of up to T steps add:
#     logspace = 4 T u Lmax.
# (The device's linear recursion has no such term; it is there so that the comparison is fair to the reference.)
# Underflow: a state whose b_t(k) is below 2^-1022 is dropped.  Its posterior is at most 2^-1022 times the ratio of the
# predictions and of the betas of two states, each at most 1 / 1e-20 because A is clamped there:
#     underflow = K 2^-1022 1e40     per frame, relative to a posterior sum of 1.
# The log probability of a trajectory is a sum of T terms max_k l_t(k) + log(normaliser): each maximum is off by at most
# (F + 6) u E_t, each logarithm by u |log| <= u log(1e20 K) (A is clamped at 1e-20) plus the (2 K + 6) u of its argument,
# and a sequential sum of T terms by u times its largest partial sum per addition; the partial sums are the lattice's
# own scale, at most Lmax = max |fwd_t(k)|:
#     |d logprob| <= T u ((F + 6) E + 2 K + 8 + log(1e20 K)) + 2 T u Lmax.
def emission_magnitude(X, means, vars):
    x = np.abs(np.asarray(X, dtype=np.float64))[:, None, :]
    m = np.abs(np.asarray(means, dtype=np.float64))[None]
    v = np.asarray(vars, dtype=np.float64)[None]
    F = x.shape[2]
    return float((((x + m) ** 2 / v + np.abs(np.log(v))) / 2).sum(2).max() + F * np.log(2 * np.pi) / 2)


def rho_of(T, K, F, E):
    """The relative bound of one posterior: linear in the trajectory length T and in the number of states K."""
    return 2.0 * T * ((2 * K + 6) * U + (F + 6) * U * E + 3 * U)


def bounds_line(name, b):
    """One line of profiles/hmm_bounds.txt."""
    return ("%-26s %6d %6d %4d %4d %10.3e %10.3e %10.3e %10.3e %12.3e"
            % (name, b['N'], b['T'], b['K'], b['F'], b['E'], b['rho'], b['logspace'], b['rel'], b['logprob'].max()))


def bound(seqs, means, vars, transmat, lsp):
    """dict: ``rel`` (relative to the scales in ``scale``), ``scale`` (post, trans, obs, obs**2), ``logprob`` (absolute,
    per trajectory), and the pieces (``rho``, ``E``, ``underflow``, ``logspace``)."""
    means = np.asarray(means, dtype=np.float64)
    K, F = means.shape
    N = sum(len(X) for X in seqs)
    T = max(len(X) for X in seqs)
    E = max(emission_magnitude(X, means, vars) for X in seqs)
    rho = rho_of(T, K, F, E)
    underflow = K * 2.0 ** -1022 * 1e40
    logA = log_transmat(transmat, np.float64)
    lp = []
    logspace = 0.0
    for X in seqs:
        ll = np.asarray(loglik(X, means, vars, np.float64), dtype=np.float64)
        lmax = float(np.abs(forward(ll, logA, np.asarray(lsp, dtype=np.float64))).max())
        Tj = len(X)
        logspace = max(logspace, 4.0 * Tj * U * lmax)
        lp.append(Tj * U * ((F + 6) * E + 2 * K + 8 + np.log(1e20 * K)) + 2 * Tj * U * lmax)
    allx = np.abs(np.concatenate([np.asarray(X, dtype=np.float64) for X in seqs]))
    scale = {'post': float(N), 'trans': float(max(N - len(seqs), 1)),
             'obs': np.maximum(allx.sum(0), np.finfo(np.float64).tiny)[None, :],
             'obs**2': np.maximum((allx ** 2).sum(0), np.finfo(np.float64).tiny)[None, :]}
    return {'rel': rho + (N + 2) * U + underflow + logspace, 'rho': rho, 'E': E, 'underflow': underflow, 'logspace': logspace,
            'scale': scale,
            'logprob': np.array(lp), 'N': N, 'T': T, 'K': K, 'F': F}


def check_stats(got, want, b, factor=1.0, who=''):
    """Assert every sum of ``got`` within ``factor`` times the bound ``b`` of ``want`` (longdouble)."""
    for key in ('post', 'trans', 'obs', 'obs**2'):
        g = np.asarray(got[key]).astype(np.longdouble)
        w = np.asarray(want[key]).astype(np.longdouble)
        err = np.abs(g - w) / b['scale'][key]
        assert np.all(np.isfinite(np.asarray(g, dtype=np.float64))), (who, key, 'not finite')
        assert float(err.max()) <= factor * b['rel'], (who, key, float(err.max()), factor * b['rel'])
    g = np.asarray(got['traj_logprob']).astype(np.longdouble)
    w = np.asarray(want['traj_logprob']).astype(np.longdouble)
    err = np.abs(g - w)
    assert np.all(np.asarray(err, dtype=np.float64) <= factor * b['logprob']), (who, 'traj_logprob', err, factor * b['logprob'])


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
DT = {'f32': np.float32, 'f64': np.float64}


def random_transmat(rs, K, stay=0.8):
    A = rs.rand(K, K) + 0.05
    A = (1 - stay) * A / A.sum(1, keepdims=True) + stay * np.eye(K)
    return A / A.sum(1, keepdims=True)


def model(K, F, seed, spread=3.0):
    """(means, vars, transmat, lsp): states ``spread`` standard deviations apart on average."""
    rs = np.random.RandomState(1000 + seed)
    means = rs.randn(K, F) * spread
    vars = 0.5 + rs.rand(K, F)
    return means, vars, random_transmat(rs, K), np.tile(1.0 / K, K)


def sample(means, vars, transmat, T, seed, dtype=np.float64):
    """(rows [T, F] of ``dtype``, hidden states) drawn from the model."""
    rs = np.random.RandomState(seed)
    K, F = means.shape
    s = np.empty(T, dtype=np.int64)
    s[0] = rs.randint(K)
    cum = np.cumsum(transmat, axis=1)
    r = rs.rand(T)
    for t in range(1, T):
        s[t] = min(int(np.searchsorted(cum[s[t - 1]], r[t])), K - 1)
    X = means[s] + rs.randn(T, F) * np.sqrt(vars[s])
    return X.astype(dtype), s


def sequences(means, vars, transmat, lengths, seed, dtype=np.float64):
    return [sample(means, vars, transmat, T, seed * 131 + i, dtype)[0] for i, T in enumerate(lengths)]


def seam_lengths(S):
    return [1, 2, max(S - 1, 1), S, S + 1, 3 * S + 1]


def hard_cases():
    """name -> (seqs, means, vars, transmat, lsp): the numerically hard inputs, each small enough for the bound to stay
    under sqrt(u)."""
    out = {}
    rs = np.random.RandomState(7)
    # states hundreds of standard deviations apart: emission ratios underflow
    means = np.array([[0.0], [300.0], [-450.0]])
    vars = np.ones((3, 1))
    A = random_transmat(rs, 3, stay=0.6)
    out['far'] = (sequences(means, vars, A, [12, 1, 9], 3), means, vars, A, np.tile(1 / 3.0, 3))
    # exact zeros in the transition matrix: the 1e-20 clamp
    means, vars, _, lsp = model(3, 2, 11)
    A = np.array([[0.7, 0.3, 0.0], [0.0, 0.6, 0.4], [0.5, 0.0, 0.5]])
    out['zeros'] = (sequences(means, vars, np.maximum(A, 1e-3) / np.maximum(A, 1e-3).sum(1, keepdims=True), [40, 17, 2], 5),
                    means, vars, A, lsp)
    # un-centred features, |mean| / std = 100
    means = 100.0 + np.array([[0.0, 1.0], [2.5, -1.0]])
    vars = np.ones((2, 2))
    A = random_transmat(rs, 2)
    out['uncentred'] = (sequences(means, vars, A, [20, 9], 9), means, vars, A, np.tile(0.5, 2))
    # a variance of 1e-12 (rows on that scale)
    means = np.array([[0.0, 0.0], [3e-6, 1.0]])
    vars = np.array([[1e-12, 1.0], [1e-12, 2.0]])
    A = random_transmat(rs, 2)
    out['tinyvar'] = (sequences(means, vars, A, [30, 11], 13), means, vars, A, np.tile(0.5, 2))
    # a long trajectory: the log scale carried over many segments
    # (variances near 1 / (2 pi e): the log likelihood of a frame is near 0 on average, so the reference's log-space
    # lattice stays small enough over 20,000 frames for its own rounding to stay under sqrt(u); see bound())
    means = np.array([[-0.3], [0.3]])
    vars = np.array([[0.046], [0.0552]])
    A = np.array([[0.98, 0.02], [0.03, 0.97]])
    out['long'] = (sequences(means, vars, A, [20000], 17), means, vars, A, np.tile(0.5, 2))
    return out


# ---- golden cases (tests/golden/make_golden_hmm.py stores the reference's outputs for these) ----
def golden_data(dtype, seed=0, ragged=False, merged=False):
    """Well-separated three-state data in two features, and other data of the same model for score / predict.
    ``merged``: the second feature is the same in every frame, so every state's mean in it coincides and the M-step's
    merging of coincident means is what sets them."""
    means = np.array([[-4.0, 0.0], [0.0, 3.0], [4.0, -1.0]])
    vars = np.array([[0.6, 0.9], [1.1, 0.5], [0.8, 0.7]])
    A = np.array([[0.90, 0.06, 0.04], [0.05, 0.90, 0.05], [0.03, 0.07, 0.90]])
    lengths = [150, 1, 2, 97] if ragged else [120, 90, 140]
    fit = sequences(means, vars, A, lengths, 100 + seed, dtype)
    other = sequences(means, vars, A, [60, 45], 200 + seed, dtype)
    if merged:
        for X in fit + other:
            X[:, 1] = 0.0
    return fit, other


def golden_starts(n_init=1, K=3, F=2):
    """The fixed starts of the golden fits, one per run of ``n_init``: (means, vars, transmat, populations)."""
    vars = np.full((K, F), 2.0)
    transmat = np.full((K, K), 1.0 / K)
    pops = np.full(K, 1.0 / K)
    starts = [(np.array([[-3.0, 0.5], [0.5, 2.0], [3.0, -0.5]]), vars, transmat, pops),
              (np.array([[-1.0, 0.0], [0.2, 1.0], [1.0, 0.3]]), vars, transmat, pops)]
    return starts[:n_init]


def golden_fit(seqs, kw, mle, dt=np.float64, form='reference', perturb=None):
    """The restated fit of a golden case: every run of ``n_init`` from its start, the best by its last recorded log
    probability.  Returns ((means, vars, transmat, populations), fit_logprob)."""
    kw = dict(kw)
    n_init = kw.pop('n_init', 1)
    best, best_lp = None, -np.inf
    for start in golden_starts(n_init):
        params, logs = em(seqs, start, mle, dt=dt, form=form, perturb=perturb, **kw)
        if logs[-1] > best_lp:
            best, best_lp = (params, logs), logs[-1]
    return best


AMP_DELTA = 1e-7
AMP_DRAWS = 8
AMP_KEYS = ('fit_logprob', 'means', 'vars', 'transmat', 'populations', 'score', 'predict_logprob')


def golden_amplification(fit, other, kw, mle):
    """How much an error in the E-step's sums moves each quantity of a golden fit, MEASURED: the restated fit is run again
    with every sum of every E-step displaced by AMP_DELTA times its scale (the scales of bound()) in a random direction,
    AMP_DRAWS times; per quantity the largest displacement divided by AMP_DELTA.  A test multiplies it by the bound ``rel``
    of the sums.  (Random directions sample the sensitivity, they do not maximise it: the tests double it.)"""
    K = golden_starts()[0][0].shape[0]
    lsp = np.tile(1.0 / K, K)

    def quantities(res):
        (m, v, T, p), logs = res
        sc = float(estep(other, m, v, T, lsp, np.float64, 'expanded')['logprob'])
        vit = sum(float(viterbi(X, m, v, T, lsp)[0]) for X in other)
        return {'fit_logprob': logs, 'means': m, 'vars': v, 'transmat': T, 'populations': p, 'score': np.array(sc),
                'predict_logprob': np.array(vit)}

    base = golden_fit(fit, kw, mle)
    scale = bound(fit, base[0][0], base[0][1], base[0][2], lsp)['scale']
    q0 = quantities(base)
    amp = dict.fromkeys(AMP_KEYS, 0.0)
    for d in range(AMP_DRAWS):
        rs = np.random.RandomState(900 + d)

        def perturb(st, i):
            out = dict(st)
            for key in ('post', 'trans', 'obs', 'obs**2'):
                a = np.asarray(st[key], dtype=np.float64)
                out[key] = a + AMP_DELTA * np.broadcast_to(scale[key], a.shape) * rs.uniform(-1, 1, a.shape)
            return out
        q = quantities(golden_fit(fit, kw, mle, perturb=perturb))
        for key in AMP_KEYS:
            assert np.shape(q[key]) == np.shape(q0[key]), (key, 'the displaced fit stopped elsewhere')
            amp[key] = max(amp[key], float(np.abs(np.asarray(q[key]) - np.asarray(q0[key])).max()) / AMP_DELTA)
    return amp


# ---- the generated E-step cases of the GPU tier, from the plan's constants (plan: n_states -> dict of msm_hmm_plan) ----
def k_seams(plan):
    """K either side of: a second and a third matrix entry per thread, the default segment starting to shrink, the limit."""
    p1 = plan(1)
    kmax = p1['n_states_max']
    ks = {1, 2, 3, kmax - 1, kmax}
    one = int(np.floor(np.sqrt(p1['threads'])))
    two = int(np.floor(np.sqrt(2 * p1['threads'])))
    ks |= {one, one + 1, two, two + 1}
    shrink = [k for k in range(2, kmax + 1) if plan(k)['segment'] < plan(k - 1)['segment']]
    if shrink:
        ks |= {shrink[0] - 1, shrink[0]}
    return sorted(ks)


MIXED = (3, 0, 5, 1, 4, 2, 0)
STATE_LENGTHS = (1, 2, 7, 8, 9, 25)
FEATURE_LENGTHS = (1, 5, 9, 20)
SEGMENT_LENGTHS = (1, 2, 31, 130, 77)
VITERBI_SHAPES = ((1, 2, (1, 5)), (3, 3, (1, 2, 63, 64, 65, 200)), (17, 2, (40, 3)), (64, 3, (70,)))


def features(plan, K=3):
    return (1, 3, 4, 5, 17, plan(K)['threads'] // K + 1)


def default_seam_lengths(plan, K):
    S = plan(K)['segment']
    return (S - 1, S, S + 1, 2 * S + 1)


def generated_shapes(plan):
    """Every (K, F, lengths, order or None) the GPU tier generates a case for, without repeats."""
    out = []
    for segment in (4, 8, 0):
        lengths = tuple(seam_lengths(segment or plan(3)['segment']))
        out += [(3, 3, lengths, None), (3, 3, lengths, MIXED)]
    out += [(K, 3, STATE_LENGTHS, None) for K in k_seams(plan)]
    out += [(K, 2, default_seam_lengths(plan, K), None) for K in k_seams(plan)[-3:]]
    out += [(3, F, FEATURE_LENGTHS, None) for F in features(plan)]
    out += [(3, 5, STATE_LENGTHS, None), (4, 3, SEGMENT_LENGTHS, None)]
    out += [(K, F, lengths, None) for K, F, lengths in VITERBI_SHAPES]
    seen, unique = set(), []
    for shape in out:
        if shape not in seen:
            seen.add(shape)
            unique.append(shape)
    return unique


def shape_name(K, F, lengths, order, dn):
    return 'K%d_F%d_N%d_T%d%s_%s' % (K, F, sum(lengths), max(lengths), '_mixed' if order else '', dn)


def generated_case(K, F, lengths, order, dn, seed=0):
    """(trajectories, model) of one generated shape."""
    mdl = model(K, F, seed)
    seqs = sequences(mdl[0], mdl[1], mdl[2], list(lengths), seed + 1, DT[dn])
    if order:
        seqs = [seqs[i] for i in order]
    return seqs, mdl


# (name, dtype, kwargs of the estimator, ragged, merged)
GOLDEN = []
for _dn in ('f32', 'f64'):
    for _rt in ('mle', 'transpose'):
        for _fp in (0.0, 1e-2):
            GOLDEN.append(('one_%s_%s_%g' % (_dn, _rt, _fp), _dn, dict(n_iter=1, reversible_type=_rt, fusion_prior=_fp), False, False))
            GOLDEN.append(('run_%s_%s_%g' % (_dn, _rt, _fp), _dn,
                           dict(n_iter=30, thresh=1e-2, reversible_type=_rt, fusion_prior=_fp), False, False))
    GOLDEN.append(('merge_%s' % _dn, _dn, dict(n_iter=3, reversible_type='mle', fusion_prior=1e-2), False, True))
    GOLDEN.append(('ragged_%s' % _dn, _dn, dict(n_iter=4, reversible_type='transpose', fusion_prior=0.0), True, False))
    GOLDEN.append(('ninit_%s' % _dn, _dn, dict(n_iter=3, n_init=2, reversible_type='transpose', fusion_prior=1e-2), False, False))
