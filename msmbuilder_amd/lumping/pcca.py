"""Perron cluster cluster analysis on MI355X: drop-in for ``msmbuilder.lumping.PCCA`` (reference:
msmbuilder/lumping/pcca.py; Deuflhard, Huisinga, Fischer and Schuette, Linear Algebra Appl. 315, 39 (2000)).

PCCA lumps the microstates of a Markov state model by the signs of its slow right eigenvectors: eigenvector after
eigenvector, the macrostate over which that eigenvector spreads widest is split where the eigenvector reaches
``pcca_tolerance``.  The transition matrix comes from the device MLE and its eigenvectors from the device eigensolver
(``MarkovStateModel``); the splitting itself is O(n m) work on n numbers at a time and runs in vectorised numpy on the host.

Differences to the reference, both deliberate:

* ``from_msm`` carries the fitted model's symmetrised matrix over, so the eigensystem is solved on the device and not by
  ``scipy.linalg.eig``; it drops the lumping parameters from ``msm.get_params()`` (the msm may itself be a lumper) and takes
  further constructor keywords (``pcca_tolerance``; ``PCCAPlus``: ``do_minimization``, ``random_state``).
* where the model's ``n_timescales`` yields fewer than ``n_macrostates`` eigenvectors, ``ValueError`` says so (the reference
  fails with an ``IndexError`` inside the loop).

The MSM attributes of a ``PCCA`` object describe the MICROSTATE model, as in the reference; fit a new
``MarkovStateModel`` on ``transform``'s output for the macrostate model.
"""
import numpy as np

from ..msm import MarkovStateModel

__all__ = ['PCCA']

_OWN = ['n_macrostates', 'objective_function', 'pcca_tolerance', 'do_minimization', 'random_state']


def split_by_sign(vectors, n_macrostates, tolerance):
    """The reference's splitting on the non-Perron eigenvectors (columns of ``vectors``): the mapping as an int array."""
    n = vectors.shape[0]
    mapping = np.zeros(n, dtype=int)
    for i in range(n_macrostates - 1):
        v = vectors[:, i]
        top = np.full(i + 1, -np.inf)
        bottom = np.full(i + 1, np.inf)
        np.maximum.at(top, mapping, v)
        np.minimum.at(bottom, mapping, v)
        if np.any(np.isinf(top)):
            raise ValueError('PCCA: macrostate %d is empty after %d splits; fewer macrostates can be told apart at '
                             'pcca_tolerance=%g' % (int(np.flatnonzero(np.isinf(top))[0]), i, tolerance))
        split = int(np.argmax(top - bottom))
        mapping[(mapping == split) & (v >= tolerance)] = i + 1
    return mapping


class PCCA(MarkovStateModel):
    """Perron cluster cluster analysis (PCCA) for coarse-graining (lumping) microstates into macrostates.

    Parameters
    ----------
    n_macrostates : int
        The number of macrostates in the lumped model.
    objective_function : None
        PCCA has none; anything else raises ``AttributeError``.
    pcca_tolerance : float, default=1e-5
        A state joins the new macrostate where the splitting eigenvector is at least this.
    **kwargs
        Passed to :class:`MarkovStateModel`.

    Attributes
    ----------
    microstate_mapping_ : int array, [n_states_]
    """

    def __init__(self, n_macrostates, objective_function=None, pcca_tolerance=1e-5, **kwargs):
        self.n_macrostates = n_macrostates
        self.objective_function = objective_function
        if self.objective_function is not None:
            raise AttributeError("PCCA does not use an objective function")
        self.pcca_tolerance = pcca_tolerance
        super(PCCA, self).__init__(**kwargs)

    @classmethod
    def _get_param_names(cls):
        return sorted(['n_macrostates', 'objective_function', 'pcca_tolerance'] + MarkovStateModel._get_param_names())

    def fit(self, sequences, y=None):
        """Fit the microstate MSM on sequences of cluster assignments, then lump it."""
        super(PCCA, self).fit(sequences, y=y)
        self._do_lumping()
        return self

    def fit_transform(self, sequences, y=None):
        """``fit`` then ``transform`` (mode ``'clip'``): the macrostate labels of the runs of known microstates."""
        return self.fit(sequences, y=y).transform(sequences)

    def _lumping_eigenvectors(self):
        """The first ``n_macrostates`` right eigenvectors, or the ``ValueError`` that says why there are fewer."""
        m = int(self.n_macrostates)
        if m < 1:
            raise ValueError('n_macrostates must be at least 1, got %s' % (self.n_macrostates,))
        if not self.n_states_ or self.n_states_ < 1:
            raise ValueError('the model has no states to lump')
        vectors = np.asarray(self.right_eigenvectors_)
        if vectors.shape[1] < m:
            raise ValueError('n_macrostates=%d needs %d eigenvectors, but n_timescales=%s on %d states yields %d'
                             % (m, m, self.n_timescales, self.n_states_, vectors.shape[1]))
        return np.ascontiguousarray(np.real(vectors[:, :m]), dtype=np.float64)

    def _do_lumping(self):
        vectors = self._lumping_eigenvectors()
        self.microstate_mapping_ = split_by_sign(vectors[:, 1:], int(self.n_macrostates), self.pcca_tolerance)

    def partial_transform(self, sequence, mode='clip'):
        """One sequence of microstate labels to macrostate labels: ``'clip'`` -> the list of mapped runs, ``'fill'`` ->
        one array with NaN where a label is not in the model."""
        if mode not in ('clip', 'fill'):
            raise ValueError('mode must be one of ["clip", "fill"]: %s' % mode)
        trimmed = super(PCCA, self).partial_transform(sequence, mode)
        if mode == 'clip':
            return [self.microstate_mapping_[seq] for seq in trimmed]
        trimmed = np.asarray(trimmed, dtype=float)
        known = np.isfinite(trimmed)
        if np.all(known):
            return np.asarray(self.microstate_mapping_[trimmed.astype(int)])
        out = np.full(len(trimmed), np.nan)
        out[known] = self.microstate_mapping_[trimmed[known].astype(int)]
        return out

    @classmethod
    def from_msm(cls, msm, n_macrostates, objective_function=None, **kwargs):
        """A lumped model from a fitted MSM.  ``kwargs``: further keywords of this class's constructor."""
        params = msm.get_params()
        for own in _OWN:
            params.pop(own, None)   # (msm may itself be a lumper)
        params.update(kwargs)
        lumper = cls(n_macrostates=n_macrostates, objective_function=objective_function, **params)
        lumper.transmat_ = msm.transmat_
        lumper.populations_ = msm.populations_
        lumper.mapping_ = msm.mapping_
        lumper.countsmat_ = msm.countsmat_
        lumper.n_states_ = msm.n_states_
        lumper._sym = getattr(msm, '_sym', None)   # the eigensystem then takes the device route
        lumper._is_dirty = True
        lumper._do_lumping()
        return lumper
