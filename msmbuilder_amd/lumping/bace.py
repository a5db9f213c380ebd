"""Bayesian agglomerative clustering engine on MI355X: drop-in for ``msmbuilder.lumping.BACE`` (reference:
msmbuilder/lumping/bace.py; Bowman, J. Chem. Phys. 137, 134111 (2012)).

BACE lumps the microstates of a Markov state model by repeatedly merging the two connected states whose transition counts
are least distinguishable: for every connected pair it evaluates a Bayes factor, n logarithms twice over per pair, merges the
pair with the smallest one and evaluates the merged state's row again.  The reference runs this in nested Python loops.
Here the count matrix is uploaded once after the filter step and stays on the device: a tile kernel computes the initial
matrix, and the merge loop -- selection, count updates, the merged state's row, the per-row maxima -- is queued on the
stream without reading anything back (csrc/bace.hip).  The record of merges comes back once; maps and Bayes factors are
built from it on the host.

Differences to the reference, all deliberate:

* ``microstate_mapping_`` is always set and equals ``map_dict[n_macrostates]``; where ``n_macrostates`` is at least the
  number of states the filter keeps, it is the map after the filter step.  (The reference assigns it one merge early and
  relies on aliasing, which leaves it unset when one merge or none is needed.)
* ``map_dict`` and ``bayesFactors`` are reset by every ``fit`` / ``from_msm``.
* Where the next merge would find no connected pair, ``ValueError`` is raised.  (The reference merges state 0 with itself.)
* A pruned state whose largest count is its own self-transition goes to the first maximum over the other columns (the
  reference produces a wrong label there), and a pruned state with no counts to any other state raises ``ValueError``.

``n_proc`` and ``chunk_size`` are accepted and kept, and change nothing.  At most 16,384 states.

The MSM attributes of a ``BACE`` object describe the MICROSTATE model, as in the reference.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Arr, check
from ..msm import MarkovStateModel

__all__ = ['BACE']

MAX_STATES = 16384
_OWN = ['n_macrostates', 'filter', 'save_all_maps', 'n_proc', 'chunk_size']


def _counts_arr(counts):
    """An ``Arr`` over a square float64 count matrix (numpy or torch CUDA), size-checked."""
    if not _lib.is_device_array(counts):
        counts = np.ascontiguousarray(counts, dtype=np.float64)
    if counts.ndim != 2 or counts.shape[0] != counts.shape[1]:
        raise ValueError('the counts must form a square matrix')
    if counts.shape[0] > MAX_STATES:
        raise ValueError('BACE takes at most %d states, got %d' % (MAX_STATES, counts.shape[0]))
    return Arr(counts, np.float64)


def bace_pairs(counts, w, unmerged, alive, row=None, return_d=False):
    """``msm_bace_pairs``: the stored values ``float32(1 / float32(d))`` of all candidate pairs ``i < j`` (the tile kernel)
    or, with ``row``, of that state against every other kept state (the row kernel); with ``return_d`` also d itself
    (float64).  ``counts`` is a numpy array or a torch CUDA tensor, and the results are placed like it."""
    a = _counts_arr(counts)
    n = a.shape[0]
    w = np.ascontiguousarray(w, dtype=np.float64)
    unmerged = np.ascontiguousarray(unmerged, dtype=np.int32)
    alive = np.ascontiguousarray(alive, dtype=np.int32)
    if not (w.shape == unmerged.shape == alive.shape == (n,)):
        raise ValueError('w, unmerged and alive must have one entry per state')
    out = _lib.empty_like_placement(a, (n, n), np.float32)
    d = _lib.empty_like_placement(a, (n, n), np.float64) if return_d else None
    ao, ad = Arr(out, np.float32), (Arr(d, np.float64) if return_d else None)
    check(_lib.lib().msm_bace_pairs(a.vp, w.ctypes.data, unmerged.ctypes.data, alive.ctypes.data, n, -1 if row is None else int(row),
                                    ao.vp, ad.vp if return_d else None, a.on_device))
    return (out, d) if return_d else out


def bace_merges(counts, w, keep, n_macrostates, timings=False):
    """``msm_bace_fit``: (merges [m + 1, 2] int32, values [m + 1] float32) -- the selection after 0, 1, ..., m merges, the
    last one being the look-ahead; ``(-1, -1, 0)`` where no connected pair was left.  With ``timings`` also the times of
    the initial matrix, the loop and both, in milliseconds."""
    a = _counts_arr(counts)
    n = a.shape[0]
    w = np.ascontiguousarray(w, dtype=np.float64)
    keep = np.ascontiguousarray(keep, dtype=np.int32)
    if not (w.shape == keep.shape == (n,)):
        raise ValueError('w and keep must have one entry per state')
    capacity = max(int(np.count_nonzero(keep)) - int(n_macrostates), 0) + 1
    merges = np.full((capacity, 2), -1, dtype=np.int32)
    values = np.zeros(capacity, dtype=np.float32)
    count = C.c_int64(0)
    ms = (C.c_float * 3)()
    check(_lib.lib().msm_bace_fit(a.vp, w.ctypes.data, keep.ctypes.data, n, int(n_macrostates), merges.ctypes.data, values.ctypes.data,
                                  capacity, C.byref(count), C.cast(ms, C.c_void_p) if timings else None, a.on_device))
    merges, values = merges[:count.value], values[:count.value]
    return (merges, values, tuple(ms)) if timings else (merges, values)


def _renumbered(macro_map, drop):
    macro_map = macro_map.copy()
    macro_map[macro_map >= drop] -= 1
    return macro_map


def _filter_states(c, threshold):
    """The filter step on the host (n^2 logarithms in all), in the reference's own expression: every state's Bayes factor
    against the pseudo-state 1/n; the states below ``threshold`` are pruned in ascending order into the state they have the
    most counts to.  Changes c in place; returns (macro_map, kept states)."""
    n = c.shape[0]
    w = np.array(c.sum(axis=1)).flatten() + 1
    pseud = np.ones(n, dtype=np.float32) / n
    unmerged = np.ones(n, dtype=np.float32)
    d = np.zeros(n, dtype=np.float32)
    p1 = pseud / 1
    with np.errstate(all='ignore'):
        for s in range(n):
            c2 = c[s, :] + unmerged[s] * unmerged * 1.0 / n
            p2 = c2 / w[s]
            cp = (pseud + c2) / (1 + w[s])
            d[s] = pseud.dot(np.log(p1 / cp)) + c2.dot(np.log(p2 / cp))
    macro_map = np.arange(n, dtype=np.int32)
    for s in np.where(d < threshold)[0]:
        dest = int(c[s, :].argmax())
        if dest == s or not c[s, dest] > 0:
            others = c[s, :].copy()
            others[s] = -np.inf
            dest = int(others.argmax())
            if not others[dest] > 0:
                raise ValueError('BACE: state %d falls below the filter and has no counts to any other state to be '
                                 'pruned into' % s)
        c[dest, :] += c[s, :]
        c[s, :] = 0
        c[:, s] = 0
        macro_map = _renumbered(macro_map, macro_map[s])
        macro_map[s] = macro_map[dest]
    return macro_map, np.where(d >= threshold)[0]


class BACE(MarkovStateModel):
    """Bayesian agglomerative clustering engine (BACE) for coarse-graining (lumping) microstates into macrostates.

    Parameters
    ----------
    n_macrostates : int or None
        The number of macrostates in the lumped model.  ``None`` is accepted by ``from_msm`` only (nothing is lumped);
        ``fit`` raises ``RuntimeError`` after fitting the MSM.
    filter : float, default=1.1
        States whose Bayes factor against the pseudo-state is below this are pruned into their kinetically closest state
        before the merging begins.  For MSMs not built on pairwise RMSD the reference recommends 0.
    save_all_maps : bool, default=True
        Keep the map at every number of macrostates passed on the way in ``map_dict``.
    n_proc, chunk_size : int
        Accepted for compatibility; they change nothing.
    **kwargs
        Passed to :class:`MarkovStateModel`.

    Attributes
    ----------
    microstate_mapping_ : int32 array, [n_states_]
    map_dict : {number of macrostates: mapping}, with ``save_all_maps``
    bayesFactors : {number of macrostates: numpy.float32}
        The Bayes factor of the pair that is merged next at that many plus one states.
    """

    def __init__(self, n_macrostates, filter=1.1, save_all_maps=True, n_proc=1, chunk_size=100, **kwargs):
        self.n_macrostates = n_macrostates
        self.filter = filter
        self.save_all_maps = save_all_maps
        self.n_proc = n_proc
        self.chunk_size = chunk_size
        if self.save_all_maps:
            self.map_dict = {}
        super(BACE, self).__init__(**kwargs)

    @classmethod
    def _get_param_names(cls):
        return sorted(_OWN + MarkovStateModel._get_param_names())

    def fit(self, sequences, y=None):
        """Fit the microstate MSM on sequences of cluster assignments, then lump it."""
        super(BACE, self).fit(sequences, y=y)
        if self.n_macrostates is None:
            raise RuntimeError('n_macrostates must not be None to fit')
        self._do_lumping()
        return self

    def _do_lumping(self):
        if int(self.n_macrostates) < 1:
            raise ValueError('n_macrostates must be at least 1, got %s' % (self.n_macrostates,))
        shape = np.shape(self.countsmat_)
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError('the counts must form a square matrix')
        n = shape[0]
        if n > MAX_STATES:
            raise ValueError('BACE takes at most %d states, got %d' % (MAX_STATES, n))
        if n < 2:
            raise ValueError('BACE needs at least 2 states, got %d' % n)
        c = np.array(self.countsmat_, dtype=np.float64)
        if not np.all(np.isfinite(c)) or np.any(c < 0):
            raise ValueError('the counts must be non-negative and finite')
        if self.sliding_window:
            c *= self.lag_time
        macro_map, keep = _filter_states(c, self.filter)
        w = np.array(c.sum(axis=1)).flatten()
        w[keep] += 1
        flags = np.zeros(n, dtype=np.int32)
        flags[keep] = 1
        merges, values = bace_merges(c, w, flags, self.n_macrostates)
        if self.save_all_maps:
            self.map_dict = {}
        self.bayesFactors = {}
        left = len(keep)
        with np.errstate(all='ignore'):
            factors = np.float32(1.0) / values
        for step, (x, y) in enumerate(merges):
            self.bayesFactors[left - 1] = factors[step]
            if step == len(merges) - 1:
                break
            if x < 0:
                raise ValueError('BACE: no pair of connected states is left to merge at %d states; n_macrostates=%d '
                                 'cannot be reached' % (left, self.n_macrostates))
            change = macro_map == macro_map[y]
            macro_map = _renumbered(macro_map, macro_map[y])
            macro_map[change] = macro_map[x]
            left -= 1
            if self.save_all_maps:
                self.map_dict[left] = macro_map.copy()
        self.microstate_mapping_ = macro_map

    def partial_transform(self, sequence, mode='clip'):
        """One sequence of microstate labels to macrostate labels: ``'clip'`` -> the list of mapped runs, ``'fill'`` ->
        one array with NaN where a label is not in the model."""
        if self.n_macrostates is None:
            raise RuntimeError('n_macrostates must not be None to transform')
        if mode not in ('clip', 'fill'):
            raise ValueError('mode must be one of ["clip", "fill"]: %s' % mode)
        trimmed = super(BACE, self).partial_transform(sequence, mode)
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
    def from_msm(cls, msm, n_macrostates, filter=1.1, save_all_maps=True, n_proc=1, chunk_size=100):
        """A lumped model from a fitted MSM."""
        params = msm.get_params()
        for own in _OWN:
            params.pop(own, None)   # (msm may itself be a BACE)
        lumper = cls(n_macrostates, filter, save_all_maps, n_proc, chunk_size, **params)
        lumper.transmat_ = msm.transmat_
        lumper.populations_ = msm.populations_
        lumper.mapping_ = msm.mapping_
        lumper.countsmat_ = msm.countsmat_
        lumper.n_states_ = msm.n_states_
        if n_macrostates is not None:
            lumper._do_lumping()
        return lumper
