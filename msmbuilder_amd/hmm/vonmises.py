"""``VonMisesHMM`` of msmbuilder.hmm (reference: msmbuilder/hmm/vonmises.pyx, hmm/src/VonMisesHMMFitter.cpp): the
reversible hidden Markov model whose emissions are products of von Mises densities, the model for dihedral angles.

The log-emission of a frame under state k,

    l_t(k) = sum_f kappa_kf cos(x_tf - mu_kf) - sum_f (log 2 pi + log I0(kappa_kf)),

is LINEAR in the image ``Z = [cos X | sin X]`` of the angles: ``l_t(k) = cst_k + sum_j Z_tj w_kj`` with
``w = [kappa cos mu | kappa sin mu]``, and the M-step's statistics are ``gamma^T Z``.  The angles do not change over a
fit, so

* the rows are staged ONCE per ``fit`` and their image is formed ONCE (``msm_hmm_trig``, csrc/hmm.hip: the element
  widened exactly, cosine and sine in float64 for both row types), 16 bytes per angle; a ``fit`` whose image does not
  fit in device memory raises ``MemoryError``;
* every one of the ``n_init x n_iter`` E-steps (``msm_hmm_lin_estep``) is the time-parallel forward-backward of
  ``GaussianHMM`` with the linear emission over that image: no trigonometry, no subtraction, no squares;
* ``score`` (``msm_hmm_lin_score``) and ``predict`` (``msm_hmm_lin_viterbi``) form the image of what they are given;
* the hot start is the device ``MiniBatchKMeans`` on the float32 cast of the image;
* the M-step is K x F and K x K objects, numpy float64 on the host; the reversible transition matrix is
  ``GaussianHMM``'s (device solver of ``msm`` for ``reversible_type='mle'``).

Kept from the reference on purpose: the start probabilities handed over where their logarithms are expected (every
trajectory's log probability carries ``+1 / n_states``), ``thresh`` held as a float32, statistics and ``fit_logprob_``
recorded by the M-step only, the best run chosen by its last recorded log probability.

Different on purpose: the reference's k-means hot start is unseeded; here it takes ``random_state``, so a seeded ``fit``
repeats.  For float32 rows the reference takes cosine and sine in single precision; here the widened value gets float64
trigonometry.  ``log I0(kappa)`` is ``log(i0e(kappa)) + kappa``, which cannot overflow, and ``log 2 pi`` is a double.
"""
import ctypes as C
import time

import numpy as np
import scipy.special

from .. import _lib
from .._lib import check
from ..base import BaseEstimator
from .gaussian import GaussianHMM, _Rows, _f64, _sfx, plan, _WEIGHT_PAD  # noqa: F401  (plan: the same for both models)

__all__ = ['VonMisesHMM']

_LOG_2PI = float(np.log(2 * np.pi))


def log_i0(kappa):
    """``log I0(kappa)`` without overflow: ``i0e`` is ``exp(-|kappa|) I0(kappa)``."""
    kappa = np.asarray(kappa, dtype=np.float64)
    return np.log(scipy.special.i0e(kappa)) + np.abs(kappa)


def linear_form(means, kappas):
    """The emission as a linear form over the image: (w [K, 2F] = [kappa cos mu | kappa sin mu],
    cst [K] = -sum_f (log 2 pi + log I0(kappa)))."""
    means, kappas = _f64(means), _f64(kappas)
    if means.ndim != 2 or means.shape != kappas.shape:
        raise ValueError('means and kappas must both be (n_states, n_features)')
    w = np.hstack([kappas * np.cos(means), kappas * np.sin(means)])
    return _f64(w), _f64(-(_LOG_2PI + log_i0(kappas)).sum(axis=1))


def trig(rows, pad=0):
    """The image of ``rows`` (a ``_Rows`` of angles, host or device): a ``_Rows`` over a torch float64 device tensor
    ``[cos X | sin X]`` (``pad`` extra columns of pitch, never written)."""
    import torch
    n, F = rows.n, rows.F
    if n < 1:
        raise ValueError('sequences is empty')
    device = rows.X.device if rows.on_device else 'cuda:%d' % _lib.ensure_device()
    try:
        buf = torch.empty((n, 2 * F + int(pad)), dtype=torch.float64, device=device)
    except torch.cuda.OutOfMemoryError:
        raise MemoryError('the image [cos X | sin X] of %d frames x %d features needs %d bytes of device memory (16 per '
                          'angle) and does not fit' % (n, F, 16 * n * F))
    if pad:
        buf.fill_(float('nan'))
    fn = getattr(_lib.lib(), "msm_hmm_trig_" + _sfx(rows.itemsize))
    _lib.set_stream(torch.cuda.current_stream(buf.device).cuda_stream)   # (host rows too: the fill above is on this stream)
    check(fn(rows.ptr, n, F, rows.ld, buf.data_ptr(), int(buf.stride(0)), rows.on_device))
    return _Rows(buf[:, :2 * F], np.diff(rows.offsets))


def _check_form(zrows, w, cst, transmat=None, lsp=None):
    w, cst = _f64(w), _f64(cst)
    K = w.shape[0]
    if w.ndim != 2 or w.shape[1] != zrows.F or cst.shape != (K,):
        raise ValueError('parameter shapes do not match (n_states, 2 n_features) = (%d, %d)' % (K, zrows.F))
    if transmat is None:
        return K, w, cst
    transmat, lsp = _f64(transmat), _f64(lsp)
    if transmat.shape != (K, K) or lsp.shape != (K,):
        raise ValueError('parameter shapes do not match n_states = %d' % K)
    return K, w, cst, transmat, lsp


def lin_estep(zrows, w, cst, transmat, log_startprob, segment=0):
    """One E-step over the image ``zrows``: dict of ``traj_logprob``, ``post``, ``obs`` (K x 2F: ``cosobs | sinobs``),
    ``trans``, ``logprob``."""
    K, w, cst, transmat, lsp = _check_form(zrows, w, cst, transmat, log_startprob)
    D = zrows.F
    tl = np.zeros(max(zrows.n_traj, 1))
    post, obs, trans = np.zeros(K), np.zeros((K, D)), np.zeros((K, K))
    lp = C.c_double(0.0)
    check(_lib.lib().msm_hmm_lin_estep(zrows.ptr, zrows.n, D, zrows.ld, zrows.offsets.ctypes.data, zrows.n_traj, K, w.ctypes.data,
                                       cst.ctypes.data, transmat.ctypes.data, lsp.ctypes.data, int(segment), tl.ctypes.data,
                                       post.ctypes.data, obs.ctypes.data, trans.ctypes.data, C.byref(lp)))
    return {'traj_logprob': tl[:zrows.n_traj], 'post': post, 'obs': obs, 'trans': trans, 'logprob': lp.value}


def lin_score(zrows, w, cst, transmat, log_startprob, segment=0):
    """The forward half: (per-trajectory log probabilities, their sum)."""
    K, w, cst, transmat, lsp = _check_form(zrows, w, cst, transmat, log_startprob)
    tl = np.zeros(max(zrows.n_traj, 1))
    lp = C.c_double(0.0)
    check(_lib.lib().msm_hmm_lin_score(zrows.ptr, zrows.n, zrows.F, zrows.ld, zrows.offsets.ctypes.data, zrows.n_traj, K,
                                       w.ctypes.data, cst.ctypes.data, transmat.ctypes.data, lsp.ctypes.data, int(segment),
                                       tl.ctypes.data, C.byref(lp)))
    return tl[:zrows.n_traj], lp.value


def lin_loglik(zrows, w, cst):
    """The N x K emission log-likelihoods as a host float64 array."""
    import torch
    K, w, cst = _check_form(zrows, w, cst)
    out = torch.empty((max(zrows.n, 1), K), dtype=torch.float64, device=zrows.X.device)
    check(_lib.lib().msm_hmm_lin_loglik(zrows.ptr, zrows.n, zrows.F, zrows.ld, K, w.ctypes.data, cst.ctypes.data, out.data_ptr()))
    return out[:zrows.n].cpu().numpy()


def lin_viterbi(zrows, w, cst, transmat, log_startprob):
    """(states int32 [N], per-trajectory log probabilities, their sum)."""
    K, w, cst, transmat, lsp = _check_form(zrows, w, cst, transmat, log_startprob)
    states = np.zeros(max(zrows.n, 1), dtype=np.int32)
    tl = np.zeros(max(zrows.n_traj, 1))
    lp = C.c_double(0.0)
    check(_lib.lib().msm_hmm_lin_viterbi(zrows.ptr, zrows.n, zrows.F, zrows.ld, zrows.offsets.ctypes.data, zrows.n_traj, K,
                                         w.ctypes.data, cst.ctypes.data, transmat.ctypes.data, lsp.ctypes.data,
                                         states.ctypes.data, tl.ctypes.data, C.byref(lp)))
    return states[:zrows.n], tl[:zrows.n_traj], lp.value


class _InverseBesselRatio(object):
    """``A^-1`` for ``A(x) = I1(x) / I0(x)``, as the reference defines it: a cubic spline of ``log x`` over ``A(x)`` through
    512 nodes log-spaced on [1e-5, 700], its argument clipped to the nodes' range, then ``exp``.  The table is built on the
    first call, once per process."""
    N_NODES, X_MIN, X_MAX = 512, 1e-5, 700.0

    def __init__(self):
        self._spline = None

    @staticmethod
    def ratio(x):
        return scipy.special.iv(1, x) / scipy.special.iv(0, x)

    def _table(self):
        from scipy.interpolate import interp1d
        x = np.logspace(np.log10(self.X_MIN), np.log10(self.X_MAX), self.N_NODES)
        y = self.ratio(x)
        self.y_min, self.y_max = float(y.min()), float(y.max())
        self._spline = interp1d(y, np.log(x), kind='cubic')

    def __call__(self, y):
        if self._spline is None:
            self._table()
        return np.exp(self._spline(np.clip(np.asarray(y, dtype=np.float64), self.y_min, self.y_max)))


inverse_bessel_ratio = _InverseBesselRatio()


class VonMisesHMM(BaseEstimator):
    """Reversible hidden Markov model with von Mises emissions: drop-in for ``msmbuilder.hmm.VonMisesHMM`` (same
    arguments and defaults; see the module text for what is kept and what differs).

    Log probabilities (``fit_logprob_``, ``score``, ``predict``) carry the reference's ``+1 / n_states`` per trajectory in
    place of ``-log(n_states)``.

    Attributes
    ----------
    means_, kappas_ : [n_states, n_features]  (mean angle in (-pi, pi], concentration)
    transmat_ : [n_states, n_states]
    populations_ : [n_states]
    fit_logprob_ : the log probabilities of the best run's E-steps, as its M-steps recorded them
    timescales_, overlap_
    """

    def __init__(self, n_states, n_init=10, n_iter=10, thresh=1e-2, reversible_type='mle', random_state=None):
        self.n_states = n_states
        self.n_init = n_init
        self.n_iter = n_iter
        self.thresh = thresh
        self.reversible_type = reversible_type
        self.random_state = random_state
        self.n_features = -1
        self.stats = {}
        self._means_ = self._kappas_ = self._transmat_ = self._populations_ = self._fit_logprob_ = None
        self._fit_time_ = 0.0

    means_ = property(lambda self: self._means_)
    kappas_ = property(lambda self: self._kappas_)
    transmat_ = property(lambda self: self._transmat_)
    populations_ = property(lambda self: self._populations_)
    fit_logprob_ = property(lambda self: self._fit_logprob_)
    timescales_ = GaussianHMM.timescales_
    startprob = GaussianHMM.startprob

    @property
    def overlap_(self):
        """Normalised log overlap of the state densities, [n_states, n_states]: the logarithm of
        ``int f_i f_j / sqrt(int f_i^2 int f_j^2)``.  Per feature ``int f_i f_j`` is
        ``I0(kappa_ij) / (2 pi I0(kappa_i) I0(kappa_j))`` with
        ``kappa_ij^2 = kappa_i^2 + kappa_j^2 + 2 kappa_i kappa_j cos(mu_i - mu_j)``."""
        mu, kappa = _f64(self._means_), _f64(self._kappas_)
        li0 = log_i0(kappa)
        joint = np.sqrt(np.maximum(kappa[:, None, :] ** 2 + kappa[None, :, :] ** 2
                                   + 2 * kappa[:, None, :] * kappa[None, :, :] * np.cos(mu[:, None, :] - mu[None, :, :]), 0.0))
        pair = (log_i0(joint) - (_LOG_2PI + li0[:, None, :] + li0[None, :, :])).sum(axis=2)
        own = np.diag(pair)
        return pair - 0.5 * (own[:, None] + own[None, :])

    # ---- input ----
    _validate_sequences = GaussianHMM._validate_sequences
    _stage = GaussianHMM._stage
    _transition_mstep = GaussianHMM._transition_mstep

    def _image(self, sequences):
        """The image of ``sequences`` as a ``_Rows`` (the rows staged once, then ``msm_hmm_trig``)."""
        return trig(self._stage(sequences))

    # ---- hot start ----
    def _init(self, sequences):
        """Initial mean angles from a mini-batch k-means (device, seeded by ``random_state``) on the float32 cast of the
        image of all sequences: the angle of every centre's (cosine, sine) pair; ``kappas`` 1, uniform populations and
        transition matrix."""
        import torch
        import warnings
        from ..cluster.minibatchkmeans import _MiniBatchKMeans
        K = int(self.n_states)
        image = self.__dict__.get('_image_')
        if image is None or getattr(image, 'sequences', None) is not sequences:
            image = self._image(sequences)
        F = image.F // 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            centers = np.asarray(_MiniBatchKMeans(n_clusters=K, random_state=self.random_state)
                                 .fit(image.X.to(torch.float32).contiguous()).cluster_centers_, dtype=np.float64)
        self._means_ = np.arctan2(centers[:, F:], centers[:, :F])
        self._kappas_ = np.ones((K, F))
        self._populations_ = np.ones(K) / K
        self._transmat_ = np.full((K, K), 1.0 / K)

    # ---- fit ----
    def fit(self, sequences, y=None):
        """Estimate the model from a list of 2-D arrays of angles in radians (numpy or torch CUDA tensors) of one dtype,
        float32 or float64.  ``n_init`` EM runs, each from its own ``_init``; the run whose last recorded log probability
        is the largest is kept."""
        self._validate_sequences(sequences)
        if self.reversible_type not in ('mle', 'transpose'):
            raise ValueError('Invalid value for reversible_type: %s '
                             'Must be either "mle" or "transpose"' % self.reversible_type)
        self.n_features = int(sequences[0].shape[1])
        K = int(self.n_states)
        limit = plan(1)['n_states_max']
        if K > limit:
            raise ValueError('n_states = %d is above %d, the largest number of states this build serves' % (K, limit))
        t0 = time.time()
        image = self._image(sequences)
        image.sequences = sequences
        self._image_ = image
        self.stats = {}
        kept, kept_logprob = None, -np.inf
        try:
            for _ in range(int(self.n_init)):
                self._init(sequences)
                self._fit_run(image)
                recorded = self.stats['log_probability']
                if recorded[-1] > kept_logprob:
                    kept_logprob = recorded[-1]
                    kept = (self._means_, self._kappas_, self._transmat_, self._populations_, recorded)
        finally:
            del self._image_
        if kept is None:
            raise ValueError('no EM run ended on a log probability that compares (NaN in every run)')
        self._means_, self._kappas_, self._transmat_, self._populations_, self._fit_logprob_ = kept
        self._fit_time_ = time.time() - t0
        return self

    def _fit_run(self, image):
        """One EM run (HMMFitter.h:75-119): E-step, log probability, the |delta| < thresh test from the second iteration
        on, otherwise the M-step, which is also what records the statistics."""
        thresh = float(np.float32(self.thresh))   # the reference keeps it in a C float
        F = image.F // 2
        logs = []
        for i in range(int(self.n_iter)):
            st = lin_estep(image, *linear_form(self._means_, self._kappas_), self._transmat_, self.startprob)
            logs.append(st['logprob'])
            if i > 0 and abs(logs[i] - logs[i - 1]) < thresh:
                break
            self.stats['trans'] = st['trans']
            self.stats['cosobs'] = np.ascontiguousarray(st['obs'][:, :F])
            self.stats['sinobs'] = np.ascontiguousarray(st['obs'][:, F:])
            self.stats['post'] = st['post']
            self.stats['log_probability'] = np.array(logs)
            self._do_mstep()

    def _do_mstep(self):
        """New parameters from the E-step's sums in ``self.stats`` (host, float64).  With C = gamma^T cos X and
        S = gamma^T sin X the weighted log likelihood of one (state, feature) is kappa (C cos mu + S sin mu) -
        w log I0(kappa) (w the posterior weight), so mu = atan2(S, C) and kappa solves
        I1(kappa) / I0(kappa) = (C cos mu + S sin mu) / w; w is padded by 10 float32 epsilons."""
        st = self.stats
        self._transmat_, self._populations_ = self._transition_mstep(st['trans'])
        mu = np.arctan2(st['sinobs'], st['cosobs'])
        resultant = (st['cosobs'] * np.cos(mu) + st['sinobs'] * np.sin(mu)) / (st['post'][:, None] + _WEIGHT_PAD)
        self._means_ = mu
        self._kappas_ = inverse_bessel_ratio(resultant)

    # ---- use ----
    def _params(self):
        return linear_form(self._means_, self._kappas_) + (np.asarray(self._transmat_, dtype=np.float64), self.startprob)

    def score(self, sequences):
        """Log probability of ``sequences`` under the model (with the reference's ``+1 / n_states`` per trajectory)."""
        self._validate_sequences(sequences)
        return lin_score(self._image(sequences), *self._params())[1]

    def predict(self, sequences):
        """Viterbi: (log probability of the most likely paths, list of int32 state arrays)."""
        self._validate_sequences(sequences)
        image = self._image(sequences)
        states, _, lp = lin_viterbi(image, *self._params())
        return lp, [states[a:b].copy() for a, b in zip(image.offsets[:-1], image.offsets[1:])]

    def fit_predict(self, sequences, y=None):
        self.fit(sequences, y=y)
        return self.predict(sequences)

    def summarize(self):
        with np.printoptions(precision=4, suppress=True):
            return """VonMises HMM
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
        state.pop('_image_', None)
        return state

    def __setstate__(self, state):
        if isinstance(state, tuple):   # the reference's pickle layout, also how a subclass fixes the start
            (self._means_, self._kappas_, self._transmat_, self._populations_, self._fit_logprob_, self._fit_time_,
             self.n_features) = state
        else:
            self.__dict__.update(state)
