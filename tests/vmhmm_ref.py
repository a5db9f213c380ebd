"""tests/vmhmm_ref.py -- the von Mises HMM restated in numpy from its formulas, the case generators of its tests and the
rounding bound they hold the device to.  The chain pieces (log-space forward / backward, log-sum-exp, the clamped log
transition matrix), the seam lists and the reversible-MLE solver are hmm_ref's.

The model: K states, per feature a von Mises density with mean angle mu and concentration kappa,

    l_t(k) = sum_f kappa_kf cos(x_tf - mu_kf) - sum_f (log 2 pi + log I0(kappa_kf)),

a transition matrix A (clamped at 1e-20 before its logarithm) and a vector ``lsp`` ADDED to the first frame's log
likelihoods (the reference hands 1 / K there).  ``dt=np.longdouble`` with ``form='direct'`` (the formula above as it
stands, log I0 from its power series) is the yardstick; ``form='split'`` is the reference's own arithmetic: the angle
addition formula, cos x (kappa cos mu) + sin x (kappa sin mu) feature by feature.  A float32 angle is widened exactly
before anything is done with it.
"""
import os

import numpy as np

import hmm_ref as H

U = H.U
SQRT_U = H.SQRT_U
LOG_2PI = np.log(2 * np.pi)
PAD = 10 * np.finfo(np.float32).eps
HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS_FILE = os.path.join(os.path.dirname(HERE), "profiles", "vmhmm_bounds.txt")


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def log_i0(kappa, dt=np.longdouble):
    """log I0(kappa) from the power series I0(k) = sum_m (k^2 / 4)^m / (m!)^2: every term is positive, so the sum is as
    accurate as ``dt`` adds; longdouble holds I0(700) ~ 1e302 with room to spare."""
    kappa = np.asarray(kappa, dtype=np.float64)
    out = np.empty(kappa.shape, dtype=dt)
    for idx in np.ndindex(kappa.shape):
        q = dt(kappa[idx]) * dt(kappa[idx]) / dt(4)
        term, total, m = dt(1), dt(1), 0
        while term > total * dt(1e-24):
            m += 1
            term = term * q / (dt(m) * dt(m))
            total = total + term
        out[idx] = np.log(total)
    return out


def constants(kappas, dt=np.longdouble):
    """[K]: -sum_f (log 2 pi + log I0(kappa_kf))."""
    if dt == np.float64:   # the float64 route of an estimator: scipy's scaled Bessel function
        import scipy.special
        li0 = np.log(scipy.special.i0e(np.asarray(kappas, dtype=np.float64))) + np.asarray(kappas, dtype=np.float64)
        return -(LOG_2PI + li0).sum(1)
    return -(np.log(dt(2) * _pi(dt)) + log_i0(kappas, dt)).sum(1)


def _pi(dt):
    return dt(4) * np.arctan(dt(1))


def loglik(X, means, kappas, dt=np.longdouble, form='direct'):
    """[T, K] emission log-likelihoods."""
    x = np.asarray(X).astype(dt)[:, None, :]
    m = np.asarray(means, dtype=np.float64).astype(dt)[None]
    k = np.asarray(kappas, dtype=np.float64).astype(dt)[None]
    F = x.shape[2]
    out = np.tile(constants(kappas, dt)[None, :], (x.shape[0], 1))
    if form == 'split':
        kc, ks = k * np.cos(m), k * np.sin(m)
        for f in range(F):   # the reference's order
            out = out + (np.cos(x[:, :, f]) * kc[:, :, f] + np.sin(x[:, :, f]) * ks[:, :, f])
    else:
        for f in range(F):
            out = out + k[:, :, f] * np.cos(x[:, :, f] - m[:, :, f])
    return out


def image(X, dt=np.longdouble):
    """[T, 2F]: cos | sin of the exactly widened angles."""
    x = np.asarray(X).astype(dt)
    return np.hstack([np.cos(x), np.sin(x)])


def estep(seqs, means, kappas, transmat, lsp, dt=np.longdouble, form='direct'):
    """The E-step's sums over a list of trajectories: dict of traj_logprob, post, cosobs, sinobs, obs (= cosobs | sinobs),
    trans, logprob."""
    K, F = np.asarray(means).shape
    logA = H.log_transmat(transmat, dt)
    lsp = np.asarray(lsp, dtype=np.float64).astype(dt)
    post = np.zeros(K, dtype=dt)
    obs = np.zeros((K, 2 * F), dtype=dt)
    trans = np.zeros((K, K), dtype=dt)
    tl = []
    for X in seqs:
        ll = loglik(X, means, kappas, dt, form)
        fwd = H.forward(ll, logA, lsp)
        bwd = H.backward(ll, logA)
        lp = H._lse(fwd[-1], 0)
        g = fwd + bwd
        gamma = np.exp(g - H._lse(g, 1)[:, None])
        if len(X) > 1:
            w = fwd[:-1, :, None] + logA[None] + (ll[1:] + bwd[1:])[:, None, :] - lp
            trans += np.exp(H._lse(w, 0))
        post += gamma.sum(0)
        obs += gamma.T @ image(X, dt)
        tl.append(lp)
    tl = np.array(tl, dtype=dt)
    return {'traj_logprob': tl, 'post': post, 'obs': obs, 'cosobs': obs[:, :F], 'sinobs': obs[:, F:], 'trans': trans,
            'logprob': tl.sum()}


def viterbi_lattice(ll, logA, lsp):
    """(lattice, the smallest margin by which any maximum of the induction or the last frame beat its runner-up)."""
    T, K = ll.shape
    lat = np.empty_like(ll)
    lat[0] = lsp + ll[0]
    margin = np.inf

    def gap(cand, axis):
        if cand.shape[axis] < 2:
            return np.inf
        top = np.sort(cand, axis=axis)
        return float((np.take(top, -1, axis=axis) - np.take(top, -2, axis=axis)).min())
    for t in range(1, T):
        cand = lat[t - 1][:, None] + logA
        lat[t] = cand.max(0) + ll[t]
        margin = min(margin, gap(cand, 0))
    margin = min(margin, gap(lat[-1][None, :], 1))
    return lat, margin


def viterbi(X, means, kappas, transmat, lsp, dt=np.longdouble, form='direct'):
    """(log probability, int32 states, margin): the induction and the traceback both take the FIRST maximum."""
    ll = loglik(X, means, kappas, dt, form)
    logA = H.log_transmat(transmat, dt)
    lat, margin = viterbi_lattice(ll, logA, np.asarray(lsp, dtype=np.float64).astype(dt))
    T = len(ll)
    states = np.empty(T, dtype=np.int32)
    states[-1] = int(np.argmax(lat[-1]))
    lp = lat[-1][states[-1]]
    for t in range(T - 2, -1, -1):
        states[t] = int(np.argmax(lat[t] + logA[:, states[t + 1]]))
    return lp, states, margin


# ------------------------------------------------------------------------------------------------------------------
# M-step and EM loop (float64 on K x F and K x K objects, as the estimator has them)
# ------------------------------------------------------------------------------------------------------------------
def bessel_ratio(x):
    """A(x) = I1(x) / I0(x) from the exponentially scaled functions (no overflow at any x)."""
    import scipy.special
    x = np.asarray(x, dtype=np.float64)
    return scipy.special.i1e(x) / scipy.special.i0e(x)


def bessel_ratio_inverse_exact(y, lo=1e-5, hi=700.0):
    """A^-1(y) by bisection on log x to the last bit (A is increasing): the yardstick of the spline."""
    out = np.empty(np.shape(y))
    for idx in np.ndindex(out.shape):
        a, b, target = np.log(lo), np.log(hi), float(np.asarray(y)[idx])
        for _ in range(200):
            mid = 0.5 * (a + b)
            if bessel_ratio(np.exp(mid)) < target:
                a = mid
            else:
                b = mid
        out[idx] = np.exp(0.5 * (a + b))
    return out


class SplineInverse(object):
    """The reference's definition of A^-1: 512 nodes log-spaced on [1e-5, 700], a cubic spline of log x over y = A(x)
    (y from the unscaled Bessel functions, as the reference has it), the argument clipped to the nodes' range, exp."""

    def __init__(self, n=512, lo=1e-5, hi=700.0):
        import scipy.special
        from scipy.interpolate import interp1d
        self.x = np.logspace(np.log10(lo), np.log10(hi), n)
        self.y = scipy.special.iv(1, self.x) / scipy.special.iv(0, self.x)
        self.lo, self.hi = self.y.min(), self.y.max()
        self.spline = interp1d(self.y, np.log(self.x), kind='cubic')

    def __call__(self, y):
        return np.exp(self.spline(np.clip(np.asarray(y, dtype=np.float64), self.lo, self.hi)))


_SPLINE = []


def spline_inverse():
    if not _SPLINE:
        _SPLINE.append(SplineInverse())
    return _SPLINE[0]


def mstep(stats, mle, reversible_type='mle'):
    """New (means, kappas, transmat, populations) from the E-step's sums, written from the model's formulas.  Transition
    matrix: as hmm_ref.mstep.  With C = gamma^T cos X, S = gamma^T sin X and w the posterior weight (padded by 10 float32
    epsilons) the expected complete-data log likelihood of one (state, feature) is kappa (C cos mu + S sin mu) - w log
    I0(kappa): mu = atan2(S, C), and kappa solves A(kappa) = (C cos mu + S sin mu) / w through the spline inverse."""
    xi = np.asarray(stats['trans'], dtype=np.float64)
    post = np.asarray(stats['post'], dtype=np.float64)
    C = np.asarray(stats['cosobs'], dtype=np.float64)
    S = np.asarray(stats['sinobs'], dtype=np.float64)
    if reversible_type == 'mle':
        transmat, pops = mle(np.maximum(np.nan_to_num(xi), 1e-20))
    else:
        sym = np.maximum(xi + xi.T, 1e-20)
        pops = sym.sum(0) / sym.sum()
        transmat = sym / sym.sum(1)[:, None]
    mu = np.arctan2(S, C)
    r = (C * np.cos(mu) + S * np.sin(mu)) / (post + PAD)[:, None]
    return mu, spline_inverse()(r), transmat, pops


def em(seqs, start, mle, n_iter, thresh=1e-2, dt=np.float64, form='split', perturb=None, reversible_type='mle'):
    """One EM run from ``start = (means, kappas, transmat, populations)``: E-step, log probability, stop when it moved by
    less than ``thresh`` (kept as a float32) from the second iteration on, otherwise M-step.  Returns the parameters the
    last E-step ran with or the last M-step produced, and the log probabilities the M-steps recorded."""
    means, kappas, transmat, pops = [np.array(a, dtype=np.float64) for a in start]
    K = means.shape[0]
    lsp = np.tile(1.0 / K, K)
    thresh = float(np.float32(thresh))
    logs, recorded = [], []
    for i in range(n_iter):
        st = estep(seqs, means, kappas, transmat, lsp, dt, form)
        logs.append(float(st['logprob']))
        if i > 0 and abs(logs[i] - logs[i - 1]) < thresh:
            break
        recorded = list(logs)
        if perturb is not None:
            st = perturb(st, i)
        means, kappas, transmat, pops = mstep(st, mle, reversible_type)
    return (means, kappas, transmat, pops), np.array(recorded)


def overlap(means, kappas, in_place=False):
    """The normalised log overlap of the state densities, pair by pair and feature by feature:
    raw_ij - (raw_ii + raw_jj) / 2.  ``in_place``: what the reference's loop arrives at instead -- it normalises the matrix
    in place in row order, so a diagonal entry is already zero when later entries read it, and an off-diagonal entry ends
    up as raw_ij - raw_mm / 2 with m = max(i, j)."""
    means, kappas = np.asarray(means, dtype=np.float64), np.asarray(kappas, dtype=np.float64)
    K, F = means.shape
    li0 = np.asarray(log_i0(kappas), dtype=np.float64)
    raw = np.zeros((K, K))
    for i in range(K):
        for j in range(K):
            for f in range(F):
                kij = np.sqrt(kappas[i, f] ** 2 + kappas[j, f] ** 2 + 2 * kappas[i, f] * kappas[j, f] * np.cos(means[i, f] - means[j, f]))
                raw[i, j] += float(log_i0(np.array(kij))) - (LOG_2PI + li0[i, f] + li0[j, f])
    if in_place:
        out = raw.copy()
        for i in range(K):
            for j in range(K):
                out[i, j] -= 0.5 * (out[i, i] + out[j, j])
        return out
    return raw - 0.5 * (np.diag(raw)[:, None] + np.diag(raw)[None, :])


def overlap_from_reference(ref_overlap, means, kappas):
    """The normalised log overlap from what the reference returns for the same parameters: its in-place loop leaves out
    half the raw diagonal entry of the EARLIER state of every pair, which is put back here."""
    means, kappas = np.asarray(means, dtype=np.float64), np.asarray(kappas, dtype=np.float64)
    li0 = np.asarray(log_i0(kappas), dtype=np.float64)
    diag = (np.asarray(log_i0(2 * kappas), dtype=np.float64) - (LOG_2PI + 2 * li0)).sum(1)
    K = len(diag)
    out = np.array(ref_overlap, dtype=np.float64)
    for i in range(K):
        for j in range(K):
            if i != j:
                out[i, j] -= 0.5 * diag[min(i, j)]
    return out


# ------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------
# The chain is hmm_ref's, so its bound carries over with the emission term replaced.  The device evaluates
#     l_t(k) = cst_k + sum_{j < 2F} z_tj w_kj
# over the image z = [cos x | sin x].  |z| <= 1 and |w_kf,cos| + |w_kf,sin| <= sqrt(2) kappa_kf <= 2 kappa_kf, so with
# Ksum_k = sum_f kappa_kf the magnitude of what the sum adds is at most M_k = |cst_k| + 2 Ksum_k, and
#   * the (2F + 1)-term sum, one multiplication and one addition per term:      (2F + 2) u M_k
#   * the image: every z is off by at most tau u (tau: the measured error of the device's float64 cos / sin in units of
#     u = 2^-53, doubled because the measurement samples the argument range; profiles/vmhmm_bounds.txt):
#                                                                                tau u 2 Ksum_k
#   * w = fl(kappa fl(cos mu)): the cosine's rounding and the product's, |w| (1 + 2u):    2 u 2 Ksum_k
#   * cst_k in float64: per feature log(i0e) + kappa + log 2 pi, each operation rounded at the magnitude of its result,
#     and scipy's i0e good to a few u:                                           u sum_f 4 (1 + |log I0(kappa_kf)| + log 2 pi)
# in all   |dl_t(k)| <= e_emis = max_k [ (2F + 2) u M_k + (tau + 2) u 2 Ksum_k + 4 u sum_f (1 + |log I0| + log 2 pi) ],
# the same for every frame (the image is bounded, unlike a Gaussian's rows).  With it, exactly as in hmm_ref:
#     rho(T) = 2 T ((2 K + 6) u + e_emis + 3 u),      rel = rho(T_max) + (N + 2) u + underflow + logspace,
#     logspace = 4 T u Lmax,    underflow = K 2^-1022 1e40,
#     |d logprob| <= T (e_emis + u (2 K + 8 + log(1e20 K))) + 2 T u Lmax,
# relative to the scales   post: N    trans: N - n_traj    obs[., j]: sum_t |z_tj|.
# obs = gamma^T z carries the image's own error once more, outside the emission: every z_tj is off by at most tau u
# ABSOLUTE, and the posteriors of a state sum to at most N, so tau u N is added absolutely to the bound of obs (its
# scale sum_t |z_tj| can be arbitrarily small, e.g. the sine column of angles that are all zero).


def read_tau(path=BOUNDS_FILE):
    """The measured largest error of the device's cos / sin in units of u from profiles/vmhmm_bounds.txt (the line
    ``tau_measured <value>``); None while the file says "not measured"."""
    try:
        with open(path) as fh:
            for line in fh:
                parts = line.split()
                if len(parts) >= 2 and parts[0] == 'tau_measured':
                    try:
                        return float(parts[1])
                    except ValueError:
                        return None
    except OSError:
        pass
    return None


def tau():
    """The tau of the bound: twice the measured value."""
    t = read_tau()
    if t is None:
        raise RuntimeError("profiles/vmhmm_bounds.txt holds no measured tau: run the image test on the device first")
    return 2.0 * t


def emission_error(means, kappas, t):
    kappas = np.asarray(kappas, dtype=np.float64)
    K, F = kappas.shape
    li0 = np.abs(np.asarray(log_i0(kappas), dtype=np.float64))
    cst = (LOG_2PI + li0).sum(1)
    ksum = kappas.sum(1)
    M = cst + 2 * ksum
    return float(((2 * F + 2) * U * M + (t + 2) * U * 2 * ksum + 4 * U * (1 + li0 + LOG_2PI).sum(1)).max())


def bound(seqs, means, kappas, transmat, lsp, t=None):
    """dict: ``rel`` (relative to the scales in ``scale``), ``obs_abs`` (added absolutely to obs), ``scale`` (post,
    trans, obs), ``logprob`` (absolute, per trajectory), and the pieces."""
    t = tau() if t is None else t
    means = np.asarray(means, dtype=np.float64)
    K, F = means.shape
    N = sum(len(X) for X in seqs)
    T = max(len(X) for X in seqs)
    e = emission_error(means, kappas, t)
    rho = 2.0 * T * ((2 * K + 6) * U + e + 3 * U)
    underflow = K * 2.0 ** -1022 * 1e40
    logA = H.log_transmat(transmat, np.float64)
    lp, logspace = [], 0.0
    for X in seqs:
        ll = np.asarray(loglik(X, means, kappas, np.float64, 'split'), dtype=np.float64)
        lmax = float(np.abs(H.forward(ll, logA, np.asarray(lsp, dtype=np.float64))).max())
        Tj = len(X)
        logspace = max(logspace, 4.0 * Tj * U * lmax)
        lp.append(Tj * (e + U * (2 * K + 8 + np.log(1e20 * K))) + 2 * Tj * U * lmax)
    allz = np.abs(np.concatenate([np.asarray(image(X, np.float64), dtype=np.float64) for X in seqs]))
    scale = {'post': float(N), 'trans': float(max(N - len(seqs), 1)),
             'obs': np.maximum(allz.sum(0), np.finfo(np.float64).tiny)[None, :]}
    return {'rel': rho + (N + 2) * U + underflow + logspace, 'rho': rho, 'e_emis': e, 'underflow': underflow,
            'logspace': logspace, 'scale': scale, 'obs_abs': t * U * N, 'logprob': np.array(lp), 'N': N, 'T': T, 'K': K, 'F': F,
            'tau': t, 'kappa_max': float(np.max(kappas))}


def bounds_line(name, b):
    """One line of profiles/vmhmm_bounds.txt."""
    return ("%-30s %6d %6d %4d %4d %9.3g %10.3e %10.3e %10.3e %10.3e %12.3e"
            % (name, b['N'], b['T'], b['K'], b['F'], b['kappa_max'], b['e_emis'], b['rho'], b['logspace'], b['rel'], b['logprob'].max()))


def check_stats(got, want, b, factor=1.0, who=''):
    """Assert every sum of ``got`` within ``factor`` times the bound ``b`` of ``want`` (longdouble)."""
    for key in ('post', 'trans', 'obs'):
        g = np.asarray(got[key]).astype(np.longdouble)
        w = np.asarray(want[key]).astype(np.longdouble)
        assert np.all(np.isfinite(np.asarray(g, dtype=np.float64))), (who, key, 'not finite')
        err = np.abs(g - w)
        tol = factor * (b['rel'] * b['scale'][key] + (b['obs_abs'] if key == 'obs' else 0.0))
        assert np.all(np.asarray(err, dtype=np.float64) <= tol), (who, key, float((err / tol).max()), 'of the bound', b['rel'])
    g = np.asarray(got['traj_logprob']).astype(np.longdouble)
    w = np.asarray(want['traj_logprob']).astype(np.longdouble)
    err = np.abs(g - w)
    assert np.all(np.asarray(err, dtype=np.float64) <= factor * b['logprob']), (who, 'traj_logprob', err, factor * b['logprob'])


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
DT = H.DT


def wrap(x):
    """Angles wrapped to [-pi, pi)."""
    return (np.asarray(x) + np.pi) % (2 * np.pi) - np.pi


def model(K, F, seed, kappa=(0.5, 8.0)):
    """(means, kappas, transmat, lsp): mean angles uniform on the circle, concentrations log-uniform in ``kappa``."""
    rs = np.random.RandomState(3000 + seed)
    means = rs.uniform(-np.pi, np.pi, (K, F))
    kappas = np.exp(rs.uniform(np.log(kappa[0]), np.log(kappa[1]), (K, F)))
    return means, kappas, H.random_transmat(rs, K), np.tile(1.0 / K, K)


def sample(means, kappas, transmat, T, seed, dtype=np.float64):
    """(angles [T, F] of ``dtype`` in [-pi, pi), hidden states) drawn from the model."""
    rs = np.random.RandomState(seed)
    K, F = means.shape
    s = np.empty(T, dtype=np.int64)
    s[0] = rs.randint(K)
    cum = np.cumsum(transmat, axis=1)
    r = rs.rand(T)
    for t in range(1, T):
        s[t] = min(int(np.searchsorted(cum[s[t - 1]], r[t])), K - 1)
    X = wrap(rs.vonmises(means[s], kappas[s]))
    return X.astype(dtype), s


def sequences(means, kappas, transmat, lengths, seed, dtype=np.float64):
    return [sample(means, kappas, transmat, T, seed * 131 + i, dtype)[0] for i, T in enumerate(lengths)]


def generated_case(K, F, lengths, dn, seed=0, kappa=(0.5, 8.0)):
    mdl = model(K, F, seed, kappa)
    return sequences(mdl[0], mdl[1], mdl[2], list(lengths), seed + 1, DT[dn]), mdl


def viterbi_case(K, F, lengths, dn, margin_of, first_seed=0):
    """A generated case whose every Viterbi decision (longdouble) has a margin above ``margin_of(seqs, mdl)``: seeds are
    tried in order and the first that qualifies is taken, so no case is ever left out.  Returns (seqs, mdl, paths, seed)."""
    for seed in range(first_seed, first_seed + 50):
        seqs, mdl = generated_case(K, F, lengths, dn, seed)
        res = [viterbi(X, *mdl) for X in seqs]
        need = margin_of(seqs, mdl)
        if all(r[2] > 2 * n for r, n in zip(res, need)):
            return seqs, mdl, res, seed
    raise AssertionError('no seed with Viterbi margins above the bound')


def mixed_kappa_case(dn='f64'):
    """kappa = 700 against kappa = 1e-5 in one model: emission ratios underflow (exp(-1400) per feature) and states are
    dropped; the trajectories are drawn from the sharp states."""
    means = np.array([[0.0, 1.0], [2.5, -2.0], [-2.0, 0.5]])
    kappas = np.array([[700.0, 700.0], [700.0, 1e-5], [1e-5, 1e-5]])
    A = H.random_transmat(np.random.RandomState(5), 3, stay=0.6)
    return sequences(means, np.maximum(kappas, 50.0), A, [12, 1, 9, 40], 3, DT[dn]), (means, kappas, A, np.tile(1 / 3.0, 3))


def zero_transition_case(dn='f64'):
    means, kappas, _, lsp = model(3, 2, 11)
    A = np.array([[0.7, 0.3, 0.0], [0.0, 0.6, 0.4], [0.5, 0.0, 0.5]])
    gen = np.maximum(A, 1e-3) / np.maximum(A, 1e-3).sum(1, keepdims=True)
    return sequences(means, kappas, gen, [40, 17, 2], 5, DT[dn]), (means, kappas, A, lsp)


def long_case():
    """20,000 frames in one trajectory.  Two states of kappa near 18, where kappa A(kappa) = log(2 pi I0(kappa)): the log
    likelihood of a frame is near 0 on average, so the log-space lattice of the reference's own arithmetic stays small
    over 20,000 frames and the bound's log-space term with it (see hmm_ref.hard_cases, 'long')."""
    means = np.array([[-1.0], [1.2]])
    kappas = np.array([[18.0], [18.5]])
    A = np.array([[0.98, 0.02], [0.03, 0.97]])
    return sequences(means, kappas, A, [20000], 17), (means, kappas, A, np.tile(0.5, 2))


# ---- golden cases (tests/golden/make_golden_vmhmm.py stores the reference's outputs for these) ----
def golden_data(dtype, seed=0, ragged=False, tight=False):
    """Three states in two angular features, angles wrapped to [-pi, pi), and other data of the same model for score /
    predict.  ``tight``: the first state is a cluster of concentration 400, which drives its fitted kappa above 100."""
    means = np.array([[-2.0, 0.5], [0.3, 2.4], [2.2, -1.5]])
    kappas = np.array([[6.0, 9.0], [8.0, 5.0], [7.0, 6.0]])
    if tight:
        kappas[0] = 400.0
    A = np.array([[0.90, 0.06, 0.04], [0.05, 0.90, 0.05], [0.03, 0.07, 0.90]])
    lengths = [150, 1, 2, 97] if ragged else [120, 90, 140]
    fit = sequences(means, kappas, A, lengths, 100 + seed, dtype)
    other = sequences(means, kappas, A, [60, 45], 200 + seed, dtype)
    return fit, other


def golden_starts(n_init=1, K=3, F=2):
    """The fixed starts of the golden fits, one per run of ``n_init``: (means, kappas, transmat, populations)."""
    kappas = np.ones((K, F))
    transmat = np.full((K, K), 1.0 / K)
    pops = np.full(K, 1.0 / K)
    starts = [(np.array([[-1.5, 0.2], [0.5, 2.0], [2.0, -1.0]]), kappas, transmat, pops),
              (np.array([[-2.5, 1.0], [0.0, 1.5], [1.5, -2.0]]), kappas, transmat, pops)]
    return starts[:n_init]


def golden_fit(seqs, kw, mle, dt=np.float64, form='split', perturb=None):
    """The restated fit of a golden case: every run of ``n_init`` from its start, the best by its last recorded log
    probability.  Returns ((means, kappas, transmat, populations), fit_logprob)."""
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
AMP_KEYS = ('fit_logprob', 'means', 'kappas', 'transmat', 'populations', 'score', 'predict_logprob', 'overlap')


def golden_quantities(res, other):
    (m, k, T, p), logs = res
    lsp = np.tile(1.0 / len(p), len(p))
    sc = float(estep(other, m, k, T, lsp, np.float64, 'split')['logprob'])
    vit = sum(float(viterbi(X, m, k, T, lsp, np.float64, 'split')[0]) for X in other)
    return {'fit_logprob': logs, 'means': m, 'kappas': k, 'transmat': T, 'populations': p, 'score': np.array(sc),
            'predict_logprob': np.array(vit), 'overlap': overlap(m, k)}


def golden_amplification(fit, other, kw, mle):
    """How much an error in the E-step's sums moves each quantity of a golden fit, MEASURED as hmm_ref does: the restated
    fit is run again with every sum of every E-step displaced by AMP_DELTA times its scale in a random direction,
    AMP_DRAWS times; per quantity the largest displacement divided by AMP_DELTA.  (Random directions sample the
    sensitivity, they do not maximise it: the tests double it.)"""
    base = golden_fit(fit, kw, mle)
    N = sum(len(X) for X in fit)
    allz = np.abs(np.concatenate([np.asarray(image(X, np.float64), dtype=np.float64) for X in fit]))
    F = allz.shape[1] // 2
    scale = {'post': float(N), 'trans': float(max(N - len(fit), 1)), 'cosobs': allz.sum(0)[None, :F], 'sinobs': allz.sum(0)[None, F:]}
    q0 = golden_quantities(base, other)
    amp = dict.fromkeys(AMP_KEYS, 0.0)
    for d in range(AMP_DRAWS):
        rs = np.random.RandomState(900 + d)

        def perturb(st, i):
            out = dict(st)
            for key in ('post', 'trans', 'cosobs', 'sinobs'):
                a = np.asarray(st[key], dtype=np.float64)
                out[key] = a + AMP_DELTA * np.broadcast_to(scale[key], a.shape) * rs.uniform(-1, 1, a.shape)
            return out
        q = golden_quantities(golden_fit(fit, kw, mle, perturb=perturb), other)
        for key in AMP_KEYS:
            assert np.shape(q[key]) == np.shape(q0[key]), (key, 'the displaced fit stopped elsewhere')
            amp[key] = max(amp[key], float(np.abs(np.asarray(q[key]) - np.asarray(q0[key])).max()) / AMP_DELTA)
    return amp


# (name, dtype, kwargs of the estimator, ragged, tight)
GOLDEN = []
for _dn in ('f32', 'f64'):
    GOLDEN.append(('two_%s' % _dn, _dn, dict(n_iter=2, reversible_type='mle'), False, False))
    GOLDEN.append(('run_%s' % _dn, _dn, dict(n_iter=10, reversible_type='mle'), False, False))
    GOLDEN.append(('transpose_%s' % _dn, _dn, dict(n_iter=10, reversible_type='transpose'), False, False))
    GOLDEN.append(('ragged_%s' % _dn, _dn, dict(n_iter=4, reversible_type='transpose'), True, False))
    GOLDEN.append(('ninit_%s' % _dn, _dn, dict(n_iter=3, n_init=2, reversible_type='transpose'), False, False))
    GOLDEN.append(('tight_%s' % _dn, _dn, dict(n_iter=6, reversible_type='mle'), False, True))


# ---- the cases of the GPU tier (tests/test_gpu_vmhmm.py), from the plan's constants (plan: n_states -> msm_hmm_plan) ----
SEGMENTS = (0, 1, 2, 31, 77, 130)
FEATURES = (1, 5, 9, 20, 129)
KAPPAS = (1e-5, 1.0, 50.0, 700.0)
IMAGE_N = (1, 255, 256, 257, 1025)
IMAGE_F = (1, 3, 4, 129)


def estep_cases(plan):
    """[(name, seqs, model, segment)]: every E-step case of the GPU tier.  Lengths 1, 2, S - 1, S, S + 1, 3 S + 1 for every
    segment S (0: the plan's default) as one ragged list; K at hmm_ref.k_seams; F such that D = 2 F crosses the 256
    threads of a workgroup and K D crosses one round of them; the numerically hard inputs."""
    out = []
    for seg in SEGMENTS:
        lengths = H.seam_lengths(seg or plan(3)['segment'])
        seqs, mdl = generated_case(3, 3, lengths, 'f64', seed=seg)
        out.append(('segment%d' % seg, seqs, mdl, seg))
    seqs, mdl = generated_case(3, 3, H.seam_lengths(31), 'f32', seed=1)
    out.append(('segment31_f32_mixed', [seqs[i] for i in H.MIXED], mdl, 31))
    for K in H.k_seams(plan):
        seqs, mdl = generated_case(K, 3, H.STATE_LENGTHS, 'f64', seed=K)
        out.append(('K%d' % K, seqs, mdl, 8))
    for F in FEATURES:
        seqs, mdl = generated_case(3, F, H.FEATURE_LENGTHS, 'f64', seed=F, kappa=(0.5, 2.0))
        out.append(('F%d' % F, seqs, mdl, 8))
    seqs, mdl = generated_case(7, 20, H.FEATURE_LENGTHS, 'f32', seed=2, kappa=(0.5, 2.0))
    out.append(('K7_F20_f32', seqs, mdl, 8))
    seqs, mdl = mixed_kappa_case()
    out.append(('mixed_kappa', seqs, mdl, 4))
    out.append(('mixed_kappa_default', seqs, mdl, 0))
    seqs, mdl = zero_transition_case()
    out.append(('zero_transition', seqs, mdl, 4))
    seqs, mdl = long_case()
    out.append(('long', seqs, mdl, 0))
    return out


def viterbi_cases(plan, t=None):
    """[(name, seqs, model, longdouble results)] over hmm_ref.VITERBI_SHAPES, every decision margin above the bound."""
    out = []

    def need(seqs, mdl):
        return bound(seqs, *mdl, t=t)['logprob']
    for K, F, lengths in H.VITERBI_SHAPES:
        for dn in ('f32', 'f64'):
            seqs, mdl, res, seed = viterbi_case(K, F, lengths, dn, need)
            out.append(('viterbi_K%d_F%d_%s_seed%d' % (K, F, dn, seed), seqs, mdl, res))
    return out


def bounds_text(plan, tau_measured):
    """The text of profiles/vmhmm_bounds.txt: the measured tau (None: not measured) and the bound at every test shape."""
    head = ["# profiles/vmhmm_bounds.txt -- the rounding bound of tests/vmhmm_ref.py at every shape of the von Mises HMM tests.",
            "# tau_measured: the largest error of the device's float64 cos / sin of the exactly widened angle against longdouble,",
            "# in units of u = 2^-53, over the arguments of the image test (tests/test_gpu_vmhmm.py); the bound uses twice that.",
            "tau_measured %s" % ("not-measured" if tau_measured is None else "%.4f" % tau_measured)]
    if tau_measured is None:
        return "\n".join(head + ["# not measured: the bounds below are listed once the image test has run on the device"]) + "\n"
    t = 2.0 * tau_measured
    head.append("%-30s %6s %6s %4s %4s %9s %10s %10s %10s %10s %12s"
                % ("# case", "N", "T", "K", "F", "kappa", "e_emis", "rho", "logspace", "rel", "logprob"))
    for name, seqs, mdl, seg in estep_cases(plan):
        head.append(bounds_line(name, bound(seqs, *mdl, t=t)))
    for name, seqs, mdl, res in viterbi_cases(plan, t):
        head.append(bounds_line(name, bound(seqs, *mdl, t=t)))
    with np.load(os.path.join(HERE, "golden", "vmhmm_golden.npz")) as g:   # the fitted models of the golden cases
        for name, dn, kw, ragged, tight in GOLDEN:
            fit, other = golden_data(DT[dn], ragged=ragged, tight=tight)
            head.append(bounds_line('golden_' + name, bound(fit, g[name + "_means"], g[name + "_kappas"], g[name + "_transmat"],
                                                            np.tile(1 / 3.0, 3), t=t)))
    return "\n".join(head) + "\n"


def image_arguments(n, F, dn, seed=0):
    """[n, F] angles of the image test: random in [-pi, pi) with the special values planted at the front when they fit."""
    rs = np.random.RandomState(seed + 7 * n + F)
    X = rs.uniform(-np.pi, np.pi, (n, F))
    special = [0.0, np.pi, -np.pi, float(np.float32(np.pi)), -float(np.float32(np.pi)), 50.0, -50.0, 1e5, -1e5, 5e-324 if dn == 'f64' else 1e-45,
               0.5 * np.pi, 1.5 * np.pi]
    flat = X.reshape(-1)
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return X.astype(DT[dn])


def image_error(Z, X):
    """The largest error of the image ``Z`` of the angles ``X`` in units of u."""
    want = image(X)
    return float(np.abs(np.asarray(Z).astype(np.longdouble) - want).max() / U)
