"""Everything that runs after labelling in a MiniBatchKMeans step (csrc/kmeans_update_dev.h, kmeans_small_dev.h), through
the C ABI, against tests/mbk_step_ref.py: an independent numpy computation of the same step.

  * centres and counts: BIT-EQUAL to the reference (scikit-learn's streaming mean in the rows' type, members in batch
    order) -- mbk_update_kernel and mbk_small_update_kernel, float32 and float64, handle and stateless entries;
  * batch sums and counts of apply_update = 0 (what a rank of a sharded fit exports): exact;
  * batch inertia: within kmeans_label_ref.inertia_rtol of the exact inertia under the pre-update centres
    (kmeans_inertia_kernel with and without its candidate merge, mbk_small_label_kernel's own, mbk_finish_kernel);
  * the norms an update refreshes in place: labelling ~20,000 unstructured probe rows through the stepped handle gives
    bit-identical labels and inertia to a fresh handle that was handed the updated centres (norms by
    kmeans_cnorm_kernel) -- and the same after msm_mbk_reassign and msm_mbk_apply_packed;
  * msm_mbk_apply_packed: bit-equal (float32 handles) / inside the derived forward-error bound (float64 handles);
  * msm_mbk_run: the device's convergence bookkeeping (mbk_converge) is exactly scikit-learn's on the device's own
    inertias, and centres and counts are those of `steps_done` reference steps: nothing queued behind the stop ran.

No row is left out anywhere: the inputs are blobs on which the labelling rule has no near-tie (asserted on the host for
every labelled batch before the device's result is looked at; tests/test_mbk_step_ref.py), so the kernels' labels must be
the exact argmin, and one wrong label shows in the counts.  Every case first asks msm_kmeans_label_plan for the label
kernel and centre splits it was chosen for (mbk_step_ref.STEP_F32 ...), so that a change of dispatch fails it loudly.
The update kernel follows the batch size alone: the handle entries take mbk_small_update_kernel up to 1,024 rows and
mbk_update_kernel above, the stateless entries always the latter.
"""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_label_ref as R  # noqa: E402
import mbk_step_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL_NAMES = ("scalar", "v4", "v4-xcd", "label64", "small", "f64")      # MSM_KM_* of include/msmhip.h, in order
F32, F64 = np.float32, np.float64


def _dt(f64):
    return F64 if f64 else F32


def _assert_plan(B, m, K, f64, handle_entry, want, gathered=False):
    from msmbuilder_amd import _lib
    assert os.environ.get("MSM_MBK_SMALL") is None and os.environ.get("MSM_LABEL_XCD") is None
    kernel, ns, span = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    _lib.check(_lib.lib().msm_kmeans_label_plan(B, m, K, int(f64), int(handle_entry), 1, 1, int(gathered), C.byref(kernel),
                                                C.byref(ns), C.byref(span)))
    assert (KERNEL_NAMES[kernel.value], ns.value) == tuple(want), (B, m, K, f64, KERNEL_NAMES[kernel.value], ns.value, want)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _placements(X):
    import torch
    return (("host", X), ("device", torch.from_numpy(np.array(X)).cuda()))    # (X is read-only: a copy)


class Handle:
    """An msm_mbk handle of K centres x m features of `dtype`, straight through ctypes."""

    def __init__(self, K, m, dtype):
        from msmbuilder_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.K, self.m, self.dtype = K, m, np.dtype(dtype)
        self.h = C.c_void_p()
        _lib.check((self.L.msm_mbk_create_f64 if self.dtype == F64 else self.L.msm_mbk_create)(C.byref(self.h), K, m))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.msm_mbk_destroy(self.h)
        self.h = None

    def set(self, cen, w):
        cen, w = np.ascontiguousarray(cen, dtype=self.dtype), np.ascontiguousarray(w, dtype=self.dtype)
        assert cen.shape == (self.K, self.m) and w.shape == (self.K,)
        self._lib.check(self.L.msm_mbk_set(self.h, cen.ctypes.data, w.ctypes.data))

    def get(self):
        cen, w = np.empty((self.K, self.m), dtype=self.dtype), np.empty(self.K, dtype=self.dtype)
        self._lib.check(self.L.msm_mbk_get(self.h, cen.ctypes.data, w.ctypes.data))
        return cen, w

    def step(self, X, idx, apply_update):
        ax = self._lib.Arr(X, self.dtype)
        inertia = C.c_double(float("nan"))
        counts_out = np.full(self.K, np.nan, dtype=self.dtype)
        self._lib.check(self.L.msm_mbk_step(self.h, ax.vp, ax.shape[0], idx.ctypes.data, len(idx), C.byref(inertia),
                                            counts_out.ctypes.data, apply_update, ax.on_device))
        return inertia.value, counts_out

    def label(self, P):
        labels = np.full(P.shape[0], -1, dtype=np.int32)
        inertia = C.c_double(float("nan"))
        self._lib.check(self.L.msm_mbk_label(self.h, P.ctypes.data, P.shape[0], labels.ctypes.data, C.byref(inertia), 0))
        return labels, inertia.value

    def export_packed(self):
        buf = np.full(int(self.L.msm_mbk_packed_size(self.h)), np.nan)
        assert len(buf) == self.K * self.m + self.K + 1
        self._lib.check(self.L.msm_mbk_export_packed(self.h, buf.ctypes.data, 0))
        return buf

    def apply_packed(self, buf):
        counts_out = np.full(self.K, np.nan, dtype=self.dtype)
        self._lib.check(self.L.msm_mbk_apply_packed(self.h, buf.ctypes.data, counts_out.ctypes.data, 0))
        return counts_out

    def zero_packed(self):
        self._lib.check(self.L.msm_mbk_zero_packed(self.h))

    def reassign(self, X, rows, which, new_count):
        ax = self._lib.Arr(X, self.dtype)
        self._lib.check(self.L.msm_mbk_reassign(self.h, ax.vp, ax.shape[0], rows.ctypes.data, which.ctypes.data, len(rows),
                                                float(new_count), ax.on_device))


@functools.lru_cache(maxsize=None)
def _probe_rows(m, K, f64):
    return _frozen(R.gen_unstructured(M.PROBE_ROWS, m, K, _dt(f64), seed=m + K)[0])[0]


_PROBE_REF = {}


def _probe_check(h, cen):
    """The handle's norms are those of its centres `cen` (= h.get()[0]): labelling unstructured probe rows through it is
    bit-identical to a fresh handle that got `cen` by msm_mbk_set, and right by the labelling rule."""
    f64 = h.dtype == F64
    P = _probe_rows(h.m, h.K, f64)
    lab, inertia = h.label(P)
    with Handle(h.K, h.m, h.dtype) as fresh:
        fresh.set(cen, np.zeros(h.K, dtype=h.dtype))
        lab2, inertia2 = fresh.label(P)
    np.testing.assert_array_equal(lab, lab2)
    assert inertia == inertia2, (inertia, inertia2)
    key = (hashlib.sha1(cen.tobytes()).hexdigest(), h.m, h.K, f64)
    if key not in _PROBE_REF:
        _PROBE_REF[key] = R.exact_argmin(P, cen)[:2]
    ref, dref = _PROBE_REF[key]
    R.check_labels(lab, P, cen, ref, dref)
    np.testing.assert_allclose(inertia, R.exact_inertia(P, cen, lab), rtol=R.inertia_rtol(h.dtype), atol=0)


@functools.lru_cache(maxsize=None)
def _step_ref(kind, key, f64):
    """(X, C0, w0, idx, StepResult) of a step case or an edge case, computed once."""
    if kind == "edge":
        X, C0, w0, idx, _ = M.edge_case(key, _dt(f64))
    else:
        X, C0, w0, idx = M.step_case(*key, _dt(f64))
    r = M.step(np.ascontiguousarray(X[idx]), C0, w0)
    _frozen(X, C0, w0, idx, *r)
    return X, C0, w0, idx, r


def _assert_step(got_cen, got_w, counts_out, inertia, r, dtype):
    assert got_cen.dtype == dtype and got_w.dtype == dtype
    np.testing.assert_array_equal(got_w, r.counts)
    np.testing.assert_array_equal(counts_out, r.counts)
    bad = np.nonzero((got_cen != r.centers).any(axis=1))[0]
    assert len(bad) == 0, ("centres differ", len(bad), bad[:5], r.cnts[bad[:5]],
                           np.abs(got_cen[bad[:5]].astype(F64) - r.centers[bad[:5]]).max())
    assert got_cen.tobytes() == r.centers.tobytes()            # the untouched bits of member-less centres included
    np.testing.assert_allclose(inertia, r.inertia, rtol=R.inertia_rtol(dtype), atol=0)


def _run_handle_step(kind, key, f64, plan):
    dtype = _dt(f64)
    X, C0, w0, idx, r = _step_ref(kind, key, f64)
    B, (K, m) = len(idx), C0.shape
    _assert_plan(B, m, K, f64, True, plan[:2])
    assert (B <= 1024) == (plan[2] == "small")                 # MSU_CAP: which update kernel the handle launches
    assert r.near_ties == 0.0                                  # no row may be left out: the labels are the exact argmin
    for _, rows in _placements(X):
        with Handle(K, m, dtype) as h:
            h.set(C0, w0)
            inertia, counts_out = h.step(rows, idx, 1)
            cen, w = h.get()
            _assert_step(cen, w, counts_out, inertia, r, dtype)
            _probe_check(h, cen)


@pytest.mark.parametrize("B,m,K", sorted(M.STEP_F32))
def test_handle_step_f32(gpu, B, m, K):
    _run_handle_step("step", (B, m, K), False, M.STEP_F32[(B, m, K)])


@pytest.mark.parametrize("B,m,K", sorted(M.STEP_F64))
def test_handle_step_f64(gpu, B, m, K):
    _run_handle_step("step", (B, m, K), True, M.STEP_F64[(B, m, K)])


@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("name", sorted(M.EDGES))
def test_handle_step_edges(gpu, name, f64):
    """Member counts 0, 1, 2, 3, 5 and a batch size that is no multiple of 64 with mixed initial counts ("tails"); one
    centre that takes the whole batch from all-zero counts ("whole"); repeated rows in both; at both update kernels."""
    _run_handle_step("edge", name, f64, M.EDGE_PLANS[(name, f64)])


@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("B,m,K", [(1024, 32, 40), (1025, 32, 40)])
def test_reassign_after_a_step(gpu, B, m, K, f64):
    """msm_mbk_reassign: the chosen rows and new_count in the chosen centres, nothing else changed, norms recomputed."""
    dtype = _dt(f64)
    X, C0, w0, idx, r = _step_ref("step", (B, m, K), f64)
    assert r.near_ties == 0.0
    rows = np.array([5, X.shape[0] - 1, 5, 17], dtype=np.int64)
    which = np.array([K - 1, 0, 9, 20], dtype=np.int64)
    want_cen, want_w = r.centers.copy(), r.counts.copy()
    want_cen[which] = X[rows]
    want_w[which] = 7.0
    for _, xs in _placements(X):
        with Handle(K, m, dtype) as h:
            h.set(C0, w0)
            h.step(xs, idx, 1)
            h.reassign(xs, rows, which, 7.0)
            cen, w = h.get()
            assert cen.tobytes() == want_cen.tobytes() and w.tobytes() == want_w.tobytes()
            _probe_check(h, cen)


@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("B,m,K", sorted(M.STATELESS))
def test_stateless_step(gpu, B, m, K, f64):
    """msm_mbk_step_f32 / _f64 (always mbk_update_kernel): host rows, and device rows read through the index list."""
    from msmbuilder_amd import _lib
    dtype = _dt(f64)
    X, C0, w0, idx, r = _step_ref("step", (B, m, K), f64)
    assert r.near_ties == 0.0
    fn = getattr(_lib.lib(), "msm_mbk_step_" + ("f64" if f64 else "f32"))
    for where, rows in _placements(X):
        _assert_plan(B, m, K, f64, False, M.STATELESS[(B, m, K)][f64], gathered=where == "device")
        ax = _lib.Arr(rows, dtype)
        for apply_update in (1, 0):
            cen, w = C0.copy(), w0.copy()
            inertia = C.c_double(float("nan"))
            sums, cnts = np.full((K, m), np.nan), np.full(K, np.nan)
            _lib.check(fn(ax.vp, ax.shape[0], m, idx.ctypes.data, B, cen.ctypes.data, w.ctypes.data, K, C.byref(inertia),
                          sums.ctypes.data, cnts.ctypes.data, apply_update, ax.on_device))
            np.testing.assert_array_equal(cnts, r.cnts)
            assert sums.tobytes() == r.sums.tobytes(), np.abs(sums - r.sums).max()
            np.testing.assert_allclose(inertia.value, r.inertia, rtol=R.inertia_rtol(dtype), atol=0)
            if apply_update:
                _assert_step(cen, w, r.counts, inertia.value, r, dtype)
            else:
                assert cen.tobytes() == C0.tobytes() and w.tobytes() == w0.tobytes()


@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("B,m,K", [(1000, 10, 1000), (4097, 40, 300)])
def test_packed_halves(gpu, B, m, K, f64):
    """What one rank of a sharded fit does: step(apply_update = 0), export, (all-reduce: here two ranks that drew the same
    rows, so the buffer doubled on the host), apply."""
    dtype = _dt(f64)
    X, C0, w0, idx, r = _step_ref("step", (B, m, K), f64)
    _assert_plan(B, m, K, f64, True, (M.STEP_F64 if f64 else M.STEP_F32)[(B, m, K)][:2])
    assert r.near_ties == 0.0
    with Handle(K, m, dtype) as h:
        h.set(C0, w0)
        h.step(X, idx, 0)
        packed = h.export_packed()
        assert packed[:K * m].tobytes() == r.sums.tobytes(), np.abs(packed[:K * m].reshape(K, m) - r.sums).max()
        np.testing.assert_array_equal(packed[K * m:K * m + K], r.cnts)
        np.testing.assert_allclose(packed[-1], r.inertia, rtol=R.inertia_rtol(dtype), atol=0)
        cen, w = h.get()
        assert cen.tobytes() == C0.tobytes() and w.tobytes() == w0.tobytes()
        # a rank that owns no row of the batch: a zeroed buffer changes nothing
        h.zero_packed()
        zero = h.export_packed()
        assert not zero.any()
        counts_out = h.apply_packed(zero)
        cen, w = h.get()
        assert cen.tobytes() == C0.tobytes() and w.tobytes() == w0.tobytes() and counts_out.tobytes() == w0.tobytes()
        _probe_check(h, cen)
        both = 2.0 * packed
        want_cen, want_w = M.apply_packed(C0, w0, both)
        counts_out = h.apply_packed(both)
        cen, w = h.get()
        np.testing.assert_array_equal(w, want_w)
        np.testing.assert_array_equal(counts_out, want_w)
        if f64:
            v, bound = M.apply_packed_bound(C0, w0, both)
            err = np.abs(cen - v)
            assert (err <= bound).all(), (int((err > bound).sum()), float((err - bound).max()))
            untouched = r.cnts == 0
            assert cen[untouched].tobytes() == C0[untouched].tobytes()
        else:
            assert cen.tobytes() == want_cen.tobytes(), np.abs(cen.astype(F64) - want_cen).max()
        _probe_check(h, cen)


@functools.lru_cache(maxsize=None)
def _run_ref(name, f64):
    X, C0, w0, idx = M.run_case(name, _dt(f64))
    steps = M.run_reference(name, _dt(f64))
    _frozen(X, C0, w0, idx)
    return X, C0, w0, idx, steps


CARRIED = (0.09, 0.09, 2.0, 1.0, 1.0)     # a state carried over from earlier steps (first_step > 0)


@pytest.mark.parametrize("name,f64,halves", [(nm, f, False) for nm in sorted(M.RUNS) for f in (False, True)] +
                         [("b1024", False, True), ("b4100", True, True)])
def test_queued_run(gpu, name, f64, halves):
    """msm_mbk_run (halves: msm_mbk_run_begin + msm_mbk_run_end): S steps queued on the device."""
    import torch
    from msmbuilder_amd import _lib
    L = _lib.lib()
    dtype = _dt(f64)
    n, m, K, B, S, mni, first_step, _ = M.RUNS[name]
    _assert_plan(B, m, K, f64, True, M.RUN_PLANS[(name, f64)])
    X, C0, w0, idx, refs = _run_ref(name, f64)
    assert all(r.near_ties == 0.0 for r in refs)
    alpha = min(1.0, 2.0 * B / (n + 1))
    state5 = CARRIED if first_step > 0 else (0.0, 0.0, 0.0, 0.0, 0.0)
    Xd = torch.from_numpy(np.array(X)).cuda()
    ax = _lib.Arr(Xd, dtype)
    with Handle(K, m, dtype) as h:
        h.set(C0, w0)
        state6 = np.array(state5 + (-1.0,))
        steps_done, converged = C.c_int64(-1), C.c_int(-1)
        inertias = np.full(S, np.nan)
        counts_out = np.full(K, np.nan, dtype=dtype)
        if halves:
            _lib.check(L.msm_mbk_run_begin(h.h, ax.vp, n, idx.ctypes.data, S, B, first_step, alpha, mni, state6.ctypes.data))
            _lib.check(L.msm_mbk_run_end(h.h, state6.ctypes.data, C.byref(steps_done), C.byref(converged), inertias.ctypes.data,
                                         counts_out.ctypes.data))
        else:
            _lib.check(L.msm_mbk_run(h.h, ax.vp, n, idx.ctypes.data, S, B, first_step, alpha, mni, state6.ctypes.data,
                                     C.byref(steps_done), C.byref(converged), inertias.ctypes.data, counts_out.ctypes.data))
        cen, w = h.get()
        done = steps_done.value
        assert 1 <= done <= S and converged.value in (0, 1)
        assert np.isnan(inertias[done:]).all()
        for s in range(done):
            np.testing.assert_allclose(inertias[s], refs[s].inertia, rtol=R.inertia_rtol(dtype), atol=0, err_msg="step %d" % s)
        # the device's bookkeeping on the device's OWN inertias: exactly scikit-learn's
        st, want_done, fired = M.replay_convergence(inertias[:done], B, alpha, mni, first_step, state5)
        assert want_done == done and int(fired) == converged.value
        assert fired or done == S                              # ... and it stopped for no other reason
        assert tuple(state6.tolist()) == st, (state6, st)
        if name == "b4100":
            assert 0 < done < S and converged.value == 1       # this stream stops early: steps are queued behind the stop
        if name == "b256":
            assert first_step == 0 and done >= 2 and state6[3] == 1.0    # step 0 is excluded from the average
        # centres and counts of exactly `done` reference steps: nothing queued behind the stop ran
        last = refs[done - 1]
        np.testing.assert_array_equal(w, last.counts)
        np.testing.assert_array_equal(counts_out, last.counts)
        assert cen.tobytes() == last.centers.tobytes(), np.abs(cen.astype(F64) - last.centers).max()
        if done < S:
            assert cen.tobytes() != refs[done].centers.tobytes()
        _probe_check(h, cen)
