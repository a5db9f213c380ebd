"""``MarkovStateModel`` of msmbuilder.msm (reference: msmbuilder/msm/msm.py, msm/core.py) with the reversible
maximum-likelihood estimate and the eigensystem on the GPU.

What runs where:

* counting: ``_transition_counts`` (integer labels -- numpy or torch CUDA tensors such as ``KCenters.labels_`` --
  are counted on the device);
* ergodic trimming: ``scipy.sparse.csgraph`` on the K x K counts on the host (label bookkeeping);
* ``reversible_type='mle'``: ``msm_transmat_mle`` (csrc/msm_mle.hip), one launch: Anderson-accelerated fixed point
  on the populations, which also writes the symmetric ``S = D^-1/2 X D^-1/2`` that has T's eigenvalues;
* ``'mle'`` and ``'transpose'`` eigensystems: the top ``n_timescales + 1`` eigenpairs of S by rocSOLVER ``dsyevd``
  (``msm_syev_top``), mapped back with ``rv = y / sqrt(pi)``, ``lv = y * sqrt(pi)``;
* ``reversible_type=None``: T is not symmetrisable, so its eigensystem is ``scipy.linalg.eig`` on the host as in
  the reference -- the one host route of this estimator.

Not provided: ``sample_discrete``, ``draw_samples``, ``uncertainty_*``, ``score_ll``.
"""
import operator
import warnings

import numpy as np
import scipy.linalg
from scipy.sparse import csgraph, csr_matrix

from .. import _lib
from .._lib import check, is_device_array
from ..base import BaseEstimator
from .core import _transition_counts

__all__ = ['MarkovStateModel']

MAX_ITER = 100000


def _sequences_1d(y):
    """msmbuilder.utils.list_of_1d, with torch CUDA label tensors kept on the device."""
    if is_device_array(y):
        return [y] if y.dim() == 1 else list(y)
    if not hasattr(y, '__iter__') or len(y) == 0:
        raise ValueError('Bad input shape')
    if not hasattr(y[0], '__iter__') and not is_device_array(y[0]):
        return [np.array(y)]
    out = []
    for i, x in enumerate(y):
        v = x if is_device_array(x) else np.array(x)
        if v.ndim != 1:
            raise ValueError("Bad input shape. Element %d has shape %s, but should be 1D" % (i, str(tuple(v.shape))))
        out.append(v)
    return out


def _dict_compose(d1, d2):
    return {k: d2.get(v) for k, v in d1.items() if v in d2}


def _strongly_connected_subgraph(counts, weight=1, verbose=True):
    """The counts restricted to the most populated strongly connected component of the graph with an edge i -> j
    where ``counts[i, j] >= weight``; returns (counts, mapping old index -> new index, percent retained)."""
    n_in = counts.shape[0]
    n_comp, comp = csgraph.connected_components(csr_matrix(counts >= weight), connection="strong")
    pops = np.asarray(counts.sum(0)).ravel()
    comp_pops = np.array([pops[comp == c].sum() for c in range(n_comp)])
    best = comp_pops.argmax()
    total = comp_pops.sum()
    percent = 100 * comp_pops[best] / total if total != 0 else np.nan
    if verbose:
        print("MSM contains %d strongly connected component%s above weight=%.2f. Component %d selected, with "
              "population %f%%" % (n_comp, '' if n_comp == 1 else 's', weight, best, percent))
    keys = np.flatnonzero(comp == best)
    if n_comp == n_in and counts[keys[0], keys[0]] == 0:   # every state alone and no self-transition
        return np.zeros((0, 0)), {}, percent
    mapping = dict(zip(keys, range(len(keys))))
    return counts[np.ix_(keys, keys)].copy(), mapping, percent


def _transmat_mle(counts, prior=0.0, max_iter=MAX_ITER, want_s=True):
    """Device reversible MLE of ``counts + prior``: (T, pi, S or None, info).  The prior is added by the library,
    which solves in the dense form when it is nonzero (every entry is then filled) and in the sparse form otherwise."""
    K = counts.shape[0]
    C = np.ascontiguousarray(counts, dtype=np.float64)
    T = np.empty((K, K))
    pi = np.empty(K)
    S = np.empty((K, K)) if want_s else None
    info = np.zeros(4)
    _lib.ensure_device()
    check(_lib.lib().msm_transmat_mle(C.ctypes.data, K, float(prior), int(max_iter), T.ctypes.data, pi.ctypes.data,
                                      None if S is None else S.ctypes.data, info.ctypes.data))
    return T, pi, S, info


def _symmetric_top(S, k):
    """The k largest eigenvalues (descending) and orthonormal eigenvectors (columns) of the symmetric S, on the GPU."""
    n = S.shape[0]
    S = np.ascontiguousarray(S, dtype=np.float64)
    vals = np.empty(k)
    vecs = np.empty((k, n))
    _lib.ensure_device()
    check(_lib.lib().msm_syev_top(S.ctypes.data, n, k, vals.ctypes.data, vecs.ctypes.data, 0))
    return vals, vecs.T.copy()


def _normalize_eigensystem(u, lv, rv):
    """lv[:, 0] sums to 1; <lv_i, lv_i>_{1/lv_0} = 1; <lv_i, rv_i> = 1 (msm/core.py's scheme)."""
    lv[:, 0] = lv[:, 0] / np.sum(lv[:, 0])
    for i in range(1, lv.shape[1]):
        lv[:, i] = lv[:, i] / np.sqrt(np.dot(lv[:, i], lv[:, i] / lv[:, 0]))
    for i in range(rv.shape[1]):
        rv[:, i] = rv[:, i] / np.dot(lv[:, i], rv[:, i])
    return u, lv, rv


class MarkovStateModel(BaseEstimator):
    """Reversible Markov state model: drop-in for ``msmbuilder.msm.MarkovStateModel``.

    Parameters
    ----------
    lag_time : int
        The lag time of the model.
    n_timescales : int, optional
        Number of dynamical timescales to compute (default: n_states - 1).
    reversible_type : {'mle', 'transpose', None}
        'mle': reversible maximum-likelihood estimate (on the GPU); 'transpose': symmetrised counts; None: the
        non-reversible row-normalised counts.
    ergodic_cutoff : float or {'on', 'off'}
        Edge weight for the maximal strongly connected subgraph; 'on' is the smallest possible count
        (1 / lag_time with a sliding window, else 1), 'off' or 0 keeps every state.
    prior_counts : float
        Pseudo-counts added to every entry after trimming.
    sliding_window : bool
        Count every window of length ``lag_time`` (True) or the subsampled sequences only.
    verbose : bool
        Print the trimming summary.

    Attributes
    ----------
    n_states_, mapping_, countsmat_, transmat_, populations_, percent_retained_ as in the reference;
    ``mle_info_`` (reversible_type='mle'): iterations, converged, last relative step, KKT residual of the solve.
    """

    def __init__(self, lag_time=1, n_timescales=None, reversible_type='mle', ergodic_cutoff='on', prior_counts=0,
                 sliding_window=True, verbose=True):
        self.reversible_type = reversible_type
        self.lag_time = lag_time
        self.n_timescales = n_timescales
        self.prior_counts = prior_counts
        self.sliding_window = sliding_window
        self.verbose = verbose
        self.ergodic_cutoff = ergodic_cutoff

        self._is_dirty = True
        self._eigenvalues = None
        self._left_eigenvectors = None
        self._right_eigenvectors = None
        self._sym = None

        self.mapping_ = None
        self.countsmat_ = None
        self.transmat_ = None
        self.n_states_ = None
        self.populations_ = None
        self.percent_retained_ = None

    # ---- fitting -----------------------------------------------------------------------------------------------
    def _parse_ergodic_cutoff(self):
        ec = self.ergodic_cutoff
        if isinstance(ec, str) and ec.lower() == 'on':
            return 1.0 / self.lag_time if self.sliding_window else 1.0
        if isinstance(ec, str) and ec.lower() == 'off':
            return 0.0
        return ec

    def _build_counts(self, sequences):
        sequences = _sequences_1d(sequences)
        if int(self.lag_time) < 1:
            raise ValueError('Invalid lag_time: %s. Lag_time must be >= 1' % self.lag_time)
        raw, mapping = _transition_counts(sequences, int(self.lag_time), sliding_window=self.sliding_window)
        cutoff = self._parse_ergodic_cutoff()
        if cutoff > 0:
            self.countsmat_, mapping2, self.percent_retained_ = _strongly_connected_subgraph(raw, cutoff, self.verbose)
            self.mapping_ = _dict_compose(mapping, mapping2)
        else:
            self.countsmat_ = raw
            self.mapping_ = mapping
            self.percent_retained_ = 100
        self.n_states_ = self.countsmat_.shape[0]

    def fit(self, sequences, y=None):
        """Estimate the model from label sequences (numpy arrays, lists, or torch CUDA tensors)."""
        self._build_counts(sequences)
        methods = {'mle': self._fit_mle, 'transpose': self._fit_transpose, 'none': self._fit_asymetric}
        method = methods.get(str(self.reversible_type).lower())
        if method is None:
            raise ValueError('reversible_type must be one of %s: %s' % (', '.join(methods.keys()),
                                                                         self.reversible_type))
        self._sym = None
        self.transmat_, self.populations_ = method(self.countsmat_)
        self._is_dirty = True
        return self

    def _fit_mle(self, counts):
        if self._parse_ergodic_cutoff() <= 0 and self.prior_counts == 0:
            warnings.warn("reversible_type='mle' and ergodic_cutoff <= 0 are not generally compatible")
        if counts.shape[0] == 0:
            self.mle_info_ = np.zeros(4)
            return np.zeros((0, 0)), np.zeros(0)
        T, pi, S, self.mle_info_ = _transmat_mle(counts, prior=self.prior_counts)
        self._sym = S
        return T, pi

    def _fit_transpose(self, counts):
        rev = 0.5 * (counts + counts.T) + self.prior_counts
        populations = rev.sum(axis=0)
        populations /= populations.sum(dtype=float)
        rs = rev.sum(axis=1)
        transmat = rev.astype(float) / rs[:, None]
        with np.errstate(invalid='ignore', divide='ignore'):
            q = 1.0 / np.sqrt(rs)
        self._sym = rev * q[:, None] * q[None, :]
        return transmat, populations

    def _fit_asymetric(self, counts):
        rc = counts + self.prior_counts
        transmat = rc.astype(float) / rc.sum(axis=1)[:, None]
        u, lv = scipy.linalg.eig(transmat, left=True, right=False)
        order = np.argsort(-np.real(u))
        lv = np.real_if_close(lv[:, order])
        populations = lv[:, 0]
        populations /= populations.sum(dtype=float)
        return transmat, populations

    # ---- eigensystem -------------------------------------------------------------------------------------------
    def _get_eigensystem(self):
        if not self._is_dirty:
            return self._eigenvalues, self._left_eigenvectors, self._right_eigenvectors
        n_timescales = min(self.n_timescales if self.n_timescales is not None else self.n_states_ - 1,
                           self.n_states_ - 1)
        k = n_timescales + 1
        if self._sym is not None and k >= 1:
            if not np.all(np.isfinite(self._sym)):   # 'transpose' with a zero-count state: scipy.linalg.eig's refusal
                raise ValueError("array must not contain infs or NaNs")
            u, y = _symmetric_top(self._sym, k)
            root = np.sqrt(self.populations_)
            lv = y * root[:, None]
            rv = y / root[:, None]
            u, lv, rv = _normalize_eigensystem(u, lv, rv)
        else:   # reversible_type=None: the host route
            u, lv, rv = scipy.linalg.eig(self.transmat_, left=True, right=True)
            order = np.argsort(-np.real(u))
            u = np.real_if_close(u[order[:k]])
            lv = np.real_if_close(lv[:, order[:k]])
            rv = np.real_if_close(rv[:, order[:k]])
            u, lv, rv = _normalize_eigensystem(u, lv, rv)
        self._eigenvalues, self._left_eigenvectors, self._right_eigenvectors = u, lv, rv
        self._is_dirty = False
        return u, lv, rv

    @property
    def eigenvalues_(self):
        """Eigenvalues of the transition matrix, largest first."""
        return self._get_eigensystem()[0]

    @property
    def left_eigenvectors_(self):
        """Left eigenvectors (columns): lv[:, 0] = populations, <lv_i, lv_i>_{1/pi} = 1."""
        return self._get_eigensystem()[1]

    @property
    def right_eigenvectors_(self):
        """Right eigenvectors (columns): <lv_i, rv_i> = 1."""
        return self._get_eigensystem()[2]

    @property
    def timescales_(self):
        """Implied relaxation timescales, -lag_time / log(eigenvalue), in units of the input's time step."""
        u = self._get_eigensystem()[0]
        with np.errstate(invalid='ignore', divide='ignore'):
            return -self.lag_time / np.log(u[1:])

    @property
    def score_(self):
        """Training GMRQ: the sum of the computed eigenvalues."""
        return self.eigenvalues_.sum()

    @property
    def state_labels_(self):
        return [k for k, v in sorted(self.mapping_.items(), key=operator.itemgetter(1))]

    def score(self, sequences, y=None):
        """Generalized matrix Rayleigh quotient of this model's right eigenvectors on a model fitted to ``sequences``."""
        V = self.right_eigenvectors_
        m2 = self.__class__(**self.get_params())
        m2.fit(sequences)
        if self.mapping_ != m2.mapping_:
            V = self._map_eigenvectors(V, m2.mapping_)
        S = np.diag(m2.populations_)
        C = S.dot(m2.transmat_)
        try:
            return np.trace(V.T.dot(C.dot(V)).dot(np.linalg.inv(V.T.dot(S.dot(V)))))
        except np.linalg.LinAlgError:
            return np.nan

    def _map_eigenvectors(self, V, other_mapping):
        inverse = {v: k for k, v in self.mapping_.items()}
        src, dst = zip(*_dict_compose(inverse, other_mapping).items())
        out = np.zeros((len(other_mapping), V.shape[1]))
        out[dst, :] = np.take(V, src, axis=0)
        return out

    def summarize(self):
        """Diagnostic summary, the reference's text."""
        counts_nz = np.count_nonzero(self.countsmat_)
        cnz = self.countsmat_[np.nonzero(self.countsmat_)]
        lines = [
            'Markov state model',
            '------------------',
            'Lag time         : {}'.format(self.lag_time),
            'Reversible type  : {}'.format(self.reversible_type),
            'Ergodic cutoff   : {}'.format(self.ergodic_cutoff),
            'Prior counts     : {}'.format(self.prior_counts),
            '',
            'Number of states : {}'.format(self.n_states_),
            'Number of nonzero entries in counts matrix : {} ({}%)'.format(
                counts_nz, 100 * counts_nz / self.countsmat_.size),
            'Nonzero counts matrix entries:',
        ]
        for name, v in (('Min.   ', np.min(cnz)), ('1st Qu.', np.percentile(cnz, 25)),
                        ('Median ', np.percentile(cnz, 50)), ('Mean   ', np.mean(cnz)),
                        ('3rd Qu.', np.percentile(cnz, 75)), ('Max.   ', np.max(cnz))):
            lines.append('    {}: {:.1f}'.format(name, v))
        lines += [
            '',
            'Total transition counts :',
            '    {} counts'.format(np.sum(cnz)),
            'Total transition counts / lag_time:',
            '    {} units'.format(np.sum(cnz) / self.lag_time),
            'Timescales:',
            '    [{}]  units'.format(', '.join(['{:.2f}'.format(t) for t in self.timescales_])),
        ]
        return '\n'.join(lines) + '\n'

    # ---- label mapping -----------------------------------------------------------------------------------------
    def partial_transform(self, sequence, mode='clip'):
        """One sequence of labels to internal indices: 'fill' -> one array (NaN where unmapped), 'clip' -> the
        list of mapped runs."""
        if mode not in ['clip', 'fill']:
            raise ValueError('mode must be one of ["clip", "fill"]: %s' % mode)
        sequence = sequence.cpu().numpy() if is_device_array(sequence) else np.asarray(sequence)
        if sequence.ndim != 1:
            raise ValueError("Each sequence must be 1D")
        get = self.mapping_.get
        a = np.array([get(k, np.nan) for k in sequence], dtype=float)
        if mode == 'fill':
            return a.astype(int) if np.all(np.mod(a, 1) == 0) else a
        return [a[s].astype(int) for s in np.ma.clump_unmasked(np.ma.masked_invalid(a))]

    def transform(self, sequences, mode='clip'):
        """Label sequences to internal indices (see ``partial_transform``)."""
        if mode not in ['clip', 'fill']:
            raise ValueError('mode must be one of ["clip", "fill"]: %s' % mode)
        result = []
        for y in _sequences_1d(sequences):
            if mode == 'fill':
                result.append(self.partial_transform(y, mode))
            else:
                result.extend(self.partial_transform(y, mode))
        return result

    def inverse_transform(self, sequences):
        """Internal indices back to labels."""
        inverse = {v: k for k, v in self.mapping_.items()}
        f = np.vectorize(inverse.get)
        result = []
        for y in _sequences_1d(sequences):
            y = y.cpu().numpy() if is_device_array(y) else y
            uq = np.unique(y)
            if not np.all(np.logical_and(0 <= uq, uq < self.n_states_)):
                raise ValueError('sequence must be between 0 and n_states-1')
            result.append(f(y))
        return result

    def eigtransform(self, sequences, right=True, mode='clip'):
        """Project label sequences on the first ``n_timescales`` dynamical eigenvectors (right or left)."""
        op = (self.right_eigenvectors_ if right else self.left_eigenvectors_)[:, 1:]
        result = []
        for y in self.transform(sequences, mode=mode):
            finite = np.isfinite(y)
            if not np.all(finite):
                value = np.empty((y.shape[0], op.shape[1]))
                value[finite, :] = np.take(op, y[finite].astype(int), axis=0)
                value[~finite, :] = np.nan
            else:
                value = np.take(op, y, axis=0)
            result.append(value)
        return result
