"""``GaussianHMM`` of msmbuilder.hmm (reference: msmbuilder/hmm/gaussian.pyx, hmm/src/include/HMMFitter.h,
hmm/src/GaussianHMMFitter.cpp): the reversible Gaussian hidden Markov model with the L1 fusion prior.

What runs where:

* the rows are staged into device memory ONCE per ``fit`` and stay there for all ``n_init x n_iter`` E-steps;
* the E-step (``msm_hmm_estep``, csrc/hmm.hip): forward-backward made parallel in time -- per-segment K x K operators,
  a stitch per trajectory, one fused pass per segment that forms the posteriors, the transition sums and ``gamma^T X``,
  ``gamma^T X^2`` without the emissions, a lattice or the posteriors ever reaching device memory, and an ordered
  reduction; float64 for both row types;
* ``score`` (``msm_hmm_score``): the forward half; ``predict`` (``msm_hmm_viterbi``): the reference's log-space Viterbi
  with its first-maximum rules; ``draw_centroids`` / ``draw_samples`` (``msm_hmm_loglik``): the emission log-likelihoods;
* the hot start: ``MiniBatchKMeans`` and the column scan of ``preprocessing``, both on the device;
* the M-step: K x F and K x K objects, numpy float64 on the host as gaussian.pyx:570-647 defines it; the reversible
  transition matrix of ``reversible_type='mle'`` comes from the device solver of ``msm`` (``msm_transmat_mle``).

Kept from the reference on purpose: it hands ``HMMFitter`` the start probabilities themselves (1 / n_states each) where
that class expects their logarithms, so every trajectory's log probability carries ``+1 / n_states`` in place of
``-log(n_states)`` (``fit_logprob_``, ``score`` and the log probability of ``predict`` are comparable with the
reference's only because this is kept); ``log(2 pi)`` in the emission term is rounded to float32; ``thresh`` is held as a
float32; statistics (and with them ``fit_logprob_``) are recorded by the M-step, so a run that stops on ``thresh`` does
not list its last log probability, and its parameters are those the last E-step was run with.

Not provided: ``init_algo='GMM'`` (the reference's ``sklearn.mixture.GMM`` no longer exists) and
``draw_samples(scheme='maxent')`` (the reference's ``discrete_approx`` does not import on a current scipy): both raise
``NotImplementedError``.  Rows that do not fit in device memory raise.
"""
import ctypes as C
import time

import numpy as np
from sklearn.utils import check_random_state

from .. import _lib
from .._lib import check, is_device_array
from ..base import BaseEstimator
from ..utils.validation import check_iter_of_sequences

__all__ = ['GaussianHMM']

_MERGE_GAP = 1e-10                            # means of two states closer than this in a feature count as merged
_WEIGHT_PAD = 10 * np.finfo(np.float32).eps   # keeps a state without posterior weight from dividing by zero


def _sfx(itemsize):
    return "f64" if itemsize == 8 else "f32"


def plan(n_states, n_features=1, itemsize=8):
    """``msm_hmm_plan``: dict of the default segment, the longest segment, the largest ``n_states`` and the tile sizes."""
    out = (C.c_int64 * 8)()
    check(_lib.lib().msm_hmm_plan(int(n_states), int(n_features), int(itemsize), out))
    keys = ('segment', 'segment_max', 'n_states_max', 'threads', 'emission_chunk', 'partials_max', 'viterbi_chunk', 'lds_bytes')
    return dict(zip(keys, [int(v) for v in out]))


class _Rows(object):
    """Rows of a list of trajectories as ONE array (host numpy, or a torch CUDA tensor) with their offsets."""

    def __init__(self, X, lengths, ld=None):
        self.on_device = int(is_device_array(X))
        # rows may be pitched (any row stride), but their elements lie side by side: anything else is copied
        if self.on_device and X.stride(1) != 1 and X.shape[0] * X.shape[1] > 0:
            X = X.contiguous()
        elif not self.on_device and X.strides[1] != X.itemsize and X.size > 0:
            X = np.ascontiguousarray(X)
        self.X = X
        self.n, self.F = int(X.shape[0]), int(X.shape[1])
        if self.on_device:
            import torch
            _lib.ensure_device(X.device.index)
            _lib.set_stream(torch.cuda.current_stream(X.device).cuda_stream)
            self.ptr = X.data_ptr()
            self.itemsize = X.element_size()
            self.ld = int(X.stride(0)) if ld is None else int(ld)
        else:
            _lib.ensure_device()
            self.ptr = X.ctypes.data
            self.itemsize = X.itemsize
            self.ld = X.strides[0] // X.itemsize if ld is None else int(ld)
        self.offsets = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)
        self.n_traj = len(lengths)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def estep(rows, means, vars, transmat, log_startprob, segment=0):
    """One E-step on ``rows`` (a ``_Rows``): dict of ``traj_logprob``, ``post``, ``obs``, ``obs**2``, ``trans``, ``logprob``."""
    means, vars, transmat, lsp = _f64(means), _f64(vars), _f64(transmat), _f64(log_startprob)
    K = means.shape[0]
    F = rows.F
    if means.shape != (K, F) or vars.shape != (K, F) or transmat.shape != (K, K) or lsp.shape != (K,):
        raise ValueError('parameter shapes do not match (n_states, n_features) = (%d, %d)' % (K, F))
    tl = np.zeros(max(rows.n_traj, 1))
    post, obs, obs2, trans = np.zeros(K), np.zeros((K, F)), np.zeros((K, F)), np.zeros((K, K))
    lp = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_hmm_estep_" + _sfx(rows.itemsize))
    check(fn(rows.ptr, rows.n, F, rows.ld, rows.offsets.ctypes.data, rows.n_traj, K, means.ctypes.data, vars.ctypes.data,
             transmat.ctypes.data, lsp.ctypes.data, int(segment), tl.ctypes.data, post.ctypes.data, obs.ctypes.data,
             obs2.ctypes.data, trans.ctypes.data, C.byref(lp), rows.on_device))
    return {'traj_logprob': tl[:rows.n_traj], 'post': post, 'obs': obs, 'obs**2': obs2, 'trans': trans, 'logprob': lp.value}


def score(rows, means, vars, transmat, log_startprob, segment=0):
    """The forward half: (per-trajectory log probabilities, their sum)."""
    means, vars, transmat, lsp = _f64(means), _f64(vars), _f64(transmat), _f64(log_startprob)
    K = means.shape[0]
    tl = np.zeros(max(rows.n_traj, 1))
    lp = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_hmm_score_" + _sfx(rows.itemsize))
    check(fn(rows.ptr, rows.n, rows.F, rows.ld, rows.offsets.ctypes.data, rows.n_traj, K, means.ctypes.data, vars.ctypes.data,
             transmat.ctypes.data, lsp.ctypes.data, int(segment), tl.ctypes.data, C.byref(lp), rows.on_device))
    return tl[:rows.n_traj], lp.value


def loglik(rows, means, vars):
    """The N x K emission log-likelihoods as a host float64 array."""
    means, vars = _f64(means), _f64(vars)
    K = means.shape[0]
    if rows.on_device:
        import torch
        out = torch.empty((rows.n, K), dtype=torch.float64, device=rows.X.device)
        optr = out.data_ptr()
    else:
        out = np.zeros((rows.n, K))
        optr = out.ctypes.data
    fn = getattr(_lib.lib(), "msm_hmm_loglik_" + _sfx(rows.itemsize))
    check(fn(rows.ptr, rows.n, rows.F, rows.ld, K, means.ctypes.data, vars.ctypes.data, optr, rows.on_device))
    return out.cpu().numpy() if rows.on_device else out


def viterbi(rows, means, vars, transmat, log_startprob):
    """(states int32 [N], per-trajectory log probabilities, their sum)."""
    means, vars, transmat, lsp = _f64(means), _f64(vars), _f64(transmat), _f64(log_startprob)
    K = means.shape[0]
    states = np.zeros(max(rows.n, 1), dtype=np.int32)
    tl = np.zeros(max(rows.n_traj, 1))
    lp = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_hmm_viterbi_" + _sfx(rows.itemsize))
    check(fn(rows.ptr, rows.n, rows.F, rows.ld, rows.offsets.ctypes.data, rows.n_traj, K, means.ctypes.data, vars.ctypes.data,
             transmat.ctypes.data, lsp.ctypes.data, states.ctypes.data, tl.ctypes.data, C.byref(lp), rows.on_device))
    return states[:rows.n], tl[:rows.n_traj], lp.value


class GaussianHMM(BaseEstimator):
    """Reversible Gaussian hidden Markov model with L1 fusion regularisation: drop-in for
    ``msmbuilder.hmm.GaussianHMM`` (same arguments and defaults; see the module text for what is kept and what is not
    provided).

    Log probabilities (``fit_logprob_``, ``score``, ``predict``) carry the reference's ``+1 / n_states`` per trajectory in
    place of ``-log(n_states)``: the reference passes the start probabilities where their logarithms are expected.

    Attributes
    ----------
    means_, vars_ : [n_states, n_features]
    transmat_ : [n_states, n_states]
    populations_ : [n_states]
    fit_logprob_ : the log probabilities of the best run's E-steps, as its M-steps recorded them
    timescales_
    """

    def __init__(self, n_states, n_init=10, n_iter=10, n_lqa_iter=10, fusion_prior=1e-2, thresh=1e-2,
                 reversible_type='mle', vars_prior=1e-3, vars_weight=1, random_state=None, timing=False,
                 n_hotstart='all', init_algo='kmeans'):
        self.n_states = n_states
        self.n_init = n_init
        self.n_iter = n_iter
        self.n_lqa_iter = n_lqa_iter
        self.fusion_prior = fusion_prior
        self.thresh = thresh
        self.reversible_type = reversible_type
        self.vars_prior = vars_prior
        self.vars_weight = vars_weight
        self.random_state = random_state
        self.timing = timing
        self.n_hotstart = n_hotstart
        self.init_algo = init_algo
        self.n_features = -1
        self.stats = {}
        self._means_ = self._vars_ = self._transmat_ = self._populations_ = self._fit_logprob_ = None
        self._fit_time_ = 0.0

    # ---- fitted attributes ----
    means_ = property(lambda self: self._means_)
    vars_ = property(lambda self: self._vars_)
    transmat_ = property(lambda self: self._transmat_)
    populations_ = property(lambda self: self._populations_)
    fit_logprob_ = property(lambda self: self._fit_logprob_)

    @property
    def startprob(self):
        return np.tile(1.0 / int(self.n_states), int(self.n_states))

    @property
    def timescales_(self):
        """Relaxation timescales ``-1 / log(lambda)`` of ``transmat_``: one per positive eigenvalue below the stationary
        one, slowest first (None before a fit; NaNs when the eigenvalues cannot be computed)."""
        T = self._transmat_
        if T is None:
            return None
        try:
            spectrum = np.sort(np.linalg.eigvals(T))
        except np.linalg.LinAlgError:
            return np.full(int(self.n_states) - 1, np.nan)
        below = spectrum[-2::-1]   # descending, without the largest
        return -1.0 / np.log(below[below > 0])

    # ---- input ----
    def _validate_sequences(self, sequences):
        if len(sequences) == 0:
            raise ValueError('sequences is empty')
        check_iter_of_sequences(sequences)
        dtype = sequences[0].dtype
        if any(s.dtype != dtype for s in sequences):
            raise ValueError('All sequences must have the same data type')
        n_features = sequences[0].shape[1] if self.n_features == -1 else self.n_features
        if any(s.shape[1] != n_features for s in sequences):
            raise ValueError('All sequences must have %d features' % n_features)
        if str(dtype).replace('torch.', '') not in ('float32', 'float64'):
            raise ValueError('Unsupported data type: ' + str(dtype))
        if sum(int(s.shape[0]) for s in sequences) == 0 or any(int(s.shape[0]) == 0 for s in sequences):
            raise ValueError('sequences is empty')

    def _stage(self, sequences):
        """The rows of ``sequences`` as one device array (copied once; views lying back to back are used in place)."""
        import torch
        lengths = [int(s.shape[0]) for s in sequences]
        X = _lib.adjacent_view(sequences) if is_device_array(sequences[0]) else None
        if X is None:
            if all(is_device_array(s) for s in sequences):
                X = torch.cat(list(sequences)) if len(sequences) > 1 else sequences[0].contiguous()
            else:
                _lib.ensure_device()
                host = np.concatenate([s.cpu().numpy() if is_device_array(s) else np.asarray(s) for s in sequences])
                X = torch.from_numpy(np.ascontiguousarray(host)).to('cuda:%d' % _lib.ensure_device())
        return _Rows(X, lengths)

    # ---- hot start ----
    def _init(self, sequences):
        """Initial means (mini-batch k-means on the float32 rows of the first ``n_hotstart`` sequences), their column
        variances for every state, uniform populations and transition matrix (gaussian.pyx:498-523)."""
        if self.init_algo == 'GMM':
            raise NotImplementedError("init_algo='GMM' is not provided: the reference relies on sklearn.mixture.GMM, which "
                                      "no longer exists; use init_algo='kmeans'")
        from ..cluster.minibatchkmeans import _MiniBatchKMeans
        from ..preprocessing import column_statistics
        import warnings
        K = int(self.n_states)
        rows = self.__dict__.get('_staged')
        staged = rows if rows is not None and getattr(rows, 'sequences', None) is sequences else None
        if staged is None:
            staged = self._stage(sequences)
        n_hot = len(sequences) if self.n_hotstart == 'all' else min(len(sequences), int(self.n_hotstart))
        import torch
        small = staged.X[:int(staged.offsets[n_hot])].to(torch.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            centers = _MiniBatchKMeans(n_clusters=K, n_init=1, init='random', random_state=self.random_state).fit(small).cluster_centers_
        st = column_statistics([small])
        self._means_ = np.asarray(centers)
        self._vars_ = np.vstack([st['m2'] / st['n']] * K)
        self._populations_ = np.ones(K) / K
        self._transmat_ = np.empty((K, K))
        self._transmat_.fill(1.0 / K)

    # ---- fit ----
    def fit(self, sequences, y=None):
        """Estimate the model from a list of 2-D arrays (numpy or torch CUDA tensors) of one dtype, float32 or float64.
        ``n_init`` EM runs, each from its own ``_init``; the run whose last recorded log probability is the largest is
        kept."""
        self._validate_sequences(sequences)
        self.n_features = int(sequences[0].shape[1])
        K = int(self.n_states)
        limit = plan(1)['n_states_max']
        if K > limit:
            raise ValueError('n_states = %d is above %d, the largest number of states this build serves' % (K, limit))
        t0 = time.time()
        rows = self._stage(sequences)
        rows.sequences = sequences
        self._staged = rows
        self.stats = {}
        kept, kept_logprob, n_esteps = None, -np.inf, 0
        try:
            for _ in range(int(self.n_init)):
                self._init(sequences)
                self._fit_run(rows)
                recorded = self.stats['log_probability']
                n_esteps += len(recorded)
                if recorded[-1] > kept_logprob:
                    kept_logprob = recorded[-1]
                    kept = (self._means_, self._vars_, self._transmat_, self._populations_, recorded)
        finally:
            del self._staged
        if kept is None:
            raise ValueError('no EM run ended on a log probability that compares (NaN in every run)')
        self._means_, self._vars_, self._transmat_, self._populations_, self._fit_logprob_ = kept
        self._fit_time_ = time.time() - t0
        if self.timing:
            print('GaussianHMM.fit: %d frames x %d features, %d states; %d recorded E-steps in %.3f s = %.3f us per frame '
                  'and E-step' % (rows.n, self.n_features, K, n_esteps, self._fit_time_,
                                  1e6 * self._fit_time_ / (rows.n * max(n_esteps, 1))))
        return self

    def _fit_run(self, rows):
        """One EM run (HMMFitter.h:75-119): E-step, log probability, the |delta| < thresh test from the second iteration
        on, otherwise the M-step, which is also what records the statistics."""
        thresh = float(np.float32(self.thresh))   # the reference keeps it in a C float
        logs = []
        for i in range(int(self.n_iter)):
            st = estep(rows, self._means_, self._vars_, self._transmat_, self.startprob)
            logs.append(st['logprob'])
            if i > 0 and abs(logs[i] - logs[i - 1]) < thresh:
                break
            self.stats['trans'] = st['trans']
            self.stats['obs'] = st['obs']
            self.stats['obs**2'] = st['obs**2']
            self.stats['post'] = st['post']
            self.stats['log_probability'] = np.array(logs)
            self._do_mstep()

    def _transition_mstep(self, xi):
        """Reversible transition matrix and populations from the expected transition counts ``xi`` (floored at 1e-20):
        'mle' solves the reversible maximum-likelihood problem on the device, 'transpose' symmetrises the counts."""
        if self.reversible_type == 'mle':
            from ..msm.msm import _transmat_mle
            T, pi, _, _ = _transmat_mle(np.maximum(np.nan_to_num(xi), 1e-20), want_s=False)
            return T, pi
        if self.reversible_type == 'transpose':
            sym = np.maximum(xi + xi.T, 1e-20)
            weight = sym.sum(axis=0)
            return sym / sym.sum(axis=1, keepdims=True), weight / weight.sum()
        raise ValueError('Invalid value for reversible_type: %s '
                         'Must be either "mle" or "transpose"' % self.reversible_type)

    @staticmethod
    def _gaps(means):
        """|mu_k - mu_j| per feature, [K, K, F], floored at the merging distance."""
        return np.maximum(np.abs(means[:, None, :] - means[None, :, :]), _MERGE_GAP)

    def _fused_means(self, weight, wsum):
        """Means under the L1 fusion prior ``fusion_prior * sum_{k<j} |mu_k - mu_j|`` (per feature) by local quadratic
        approximation.  With w_k the posterior weight, s_k the weighted sum and v_k the current variance of state k the
        penalised objective of one feature is

            sum_k (w_k mu_k^2 / 2 - s_k mu_k) / v_k  +  lambda sum_{k<j} |mu_k - mu_j|,

        and |d| is replaced by d^2 / (2 |d_now|) around the current gaps.  ``lambda`` is adaptive: the prior divided by
        the gap of the UNPENALISED means, so pairs that start close are pulled hardest.  Each sweep therefore solves, per
        feature, (diag(w / v) + L) mu = s / v with L the Laplacian of the graph whose edge (k, j) weighs
        lambda_kj / |d_now,kj|.  Up to ``n_lqa_iter`` sweeps; a singular system ends the iteration after its sweep with the
        last solvable means.  Finally means whose gap, as measured before the last sweep, was at the merging distance are set
        equal (the later state's value, pairs in row order)."""
        K, F = wsum.shape
        means = wsum / (weight[:, None] + _WEIGHT_PAD)
        if not (float(self.fusion_prior) > 0 and int(self.n_lqa_iter) > 0):
            return means
        pull = float(self.fusion_prior) / self._gaps(means)
        pull[np.arange(K), np.arange(K), :] = 0.0
        target = wsum / self._vars_
        gaps, singular = None, False
        for _ in range(int(self.n_lqa_iter)):
            gaps = self._gaps(means)
            if singular or np.all(gaps <= _MERGE_GAP):
                break
            edges = pull / gaps
            for f in range(F):
                if np.all(gaps[:, :, f] <= _MERGE_GAP):
                    continue
                laplacian = np.diag(edges[:, :, f].sum(axis=1)) - edges[:, :, f]
                try:
                    means[:, f] = np.linalg.solve(laplacian + np.diag(weight / self._vars_[:, f]), target[:, f])
                except np.linalg.LinAlgError:
                    singular = True
        for f in range(F):
            for k in range(K):
                for j in range(k + 1, K):
                    if gaps[k, j, f] <= _MERGE_GAP:
                        means[k, f] = means[j, f]
        return means

    def _do_mstep(self):
        """New parameters from the E-step's sums in ``self.stats`` (host, float64; what gaussian.pyx:570-647 computes):
        the reversible transition matrix, the fused means, and variances
        ``(vars_prior + sum gamma (x - mu)^2) / (max(vars_weight - 1, 0) + sum gamma)`` with the square expanded over the
        accumulated sums."""
        st = self.stats
        self._transmat_, self._populations_ = self._transition_mstep(st['trans'])
        mu = self._fused_means(st['post'], st['obs'])
        self._means_ = mu
        prior, extra = (0.0, 0.0) if self.vars_prior is None else (self.vars_prior, max(self.vars_weight - 1, 0))
        mass = st['post'][:, None] + _WEIGHT_PAD
        scatter = st['obs**2'] - 2 * mu * st['obs'] + mu ** 2 * mass
        self._vars_ = (prior + scatter) / (extra + mass)

    # ---- use ----
    def _params64(self):
        return (np.asarray(self._means_, dtype=np.float64), np.asarray(self._vars_, dtype=np.float64),
                np.asarray(self._transmat_, dtype=np.float64))

    def score(self, sequences):
        """Log probability of ``sequences`` under the model (with the reference's ``+1 / n_states`` per trajectory)."""
        self._validate_sequences(sequences)
        return score(self._stage(sequences), *self._params64(), self.startprob)[1]

    def predict(self, sequences):
        """Viterbi: (log probability of the most likely paths, list of int32 state arrays)."""
        self._validate_sequences(sequences)
        rows = self._stage(sequences)
        states, _, lp = viterbi(rows, *self._params64(), self.startprob)
        return lp, [states[a:b].copy() for a, b in zip(rows.offsets[:-1], rows.offsets[1:])]

    def fit_predict(self, sequences, y=None):
        self.fit(sequences, y=y)
        return self.predict(sequences)

    def _emission_table(self, sequences):
        """(N x K emission log-likelihoods on the host, row offsets of the trajectories)."""
        rows = self._stage(sequences)
        return loglik(rows, self._means_, self._vars_), rows.offsets

    @staticmethod
    def _locate(offsets, global_rows):
        """(trajectory, frame) of rows numbered over the joined trajectories, as an int array [..., 2]."""
        global_rows = np.asarray(global_rows, dtype=np.int64)
        traj = np.searchsorted(offsets, global_rows, side='right') - 1
        return np.stack([traj, global_rows - offsets[traj]], axis=-1)

    @staticmethod
    def _host(x):
        return x.cpu().numpy() if is_device_array(x) else np.asarray(x)

    def draw_centroids(self, sequences):
        """Per state the frame whose emission likelihood under that state is the largest (the first such frame of the
        first such trajectory): ((n_states, 1, 2) int (trajectory, frame) pairs, (n_states, 1, n_features) its rows)."""
        table, offsets = self._emission_table(sequences)
        pairs = self._locate(offsets, table.argmax(axis=0))
        rows = np.stack([self._host(sequences[t][f]) for t, f in pairs])
        return pairs[:, None, :], rows[:, None, :]

    def draw_samples(self, sequences, n_samples, scheme="even", match_vars=False):
        """``scheme='even'``: every frame belongs to the state of its largest emission likelihood, and ``n_samples``
        frames are drawn per state, uniformly with replacement, one draw of ``random_state`` each: int array
        (n_states, n_samples, 2) of (trajectory, frame) pairs."""
        if scheme == 'maxent':
            raise NotImplementedError("draw_samples(scheme='maxent') is not provided: it needs the reference's "
                                      "discrete_approx module, which does not import on a current scipy; use scheme='even'")
        if scheme != 'even':
            raise ValueError("scheme must be one of ['even', 'maxent'])")
        rng = check_random_state(self.random_state)
        table, offsets = self._emission_table(sequences)
        owner = table.argmax(axis=1)
        drawn = []
        for state in range(int(self.n_states)):
            members = np.flatnonzero(owner == state)
            drawn.append([members[rng.choice(members.size)] for _ in range(n_samples)])
        return self._locate(offsets, drawn)

    def summarize(self):
        with np.printoptions(precision=4, suppress=True):
            return """Gaussian HMM
------------
n_states : {n_states}
logprob: {logprob}
fit_time: {fit_time:.3f}s

populations: {populations}
transmat:
{transmat}
timescales: {timescales}
    """.format(n_states=int(self.n_states), logprob=self._fit_logprob_[-1], populations=str(self._populations_),
               transmat=str(self._transmat_), timescales=self.timescales_, fit_time=self._fit_time_)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_staged', None)
        return state

    def __setstate__(self, state):
        if isinstance(state, tuple):   # the reference's pickle layout, also how a subclass fixes the start
            (self._means_, self._vars_, self._transmat_, self._populations_, self._fit_logprob_, self._fit_time_,
             self.n_features) = state
        else:
            self.__dict__.update(state)
