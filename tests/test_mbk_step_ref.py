"""CPU tier of the mini-batch step reference (tests/mbk_step_ref.py): its arithmetic IS scikit-learn's (centres and counts
bit for bit against sklearn.cluster._kmeans._mini_batch_step), its convergence replay IS scikit-learn's
_mini_batch_convergence, and no input of tests/test_gpu_mbk_step.py holds a near-tie -- at any step of a multi-step
case -- which is what lets the GPU tests hold the kernels' labels to the exact argmin on every row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_label_ref as R  # noqa: E402
import mbk_step_ref as M  # noqa: E402

DTYPES = (np.float32, np.float64)
SKLEARN_SHAPES = [(1000, 10, 300), (1025, 32, 40), (4097, 8, 6), (1024, 513, 60), (300, 64, 100)]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("B,m,K", SKLEARN_SHAPES)
def test_step_is_scikit_learns_mini_batch_step(B, m, K, dtype):
    km = pytest.importorskip("sklearn.cluster._kmeans")
    X, C0, w0, idx = M.step_case(B, m, K, dtype)
    Xb = np.ascontiguousarray(X[idx])
    r = M.step(Xb, C0, w0)
    assert r.near_ties == 0.0
    centers_new = np.empty_like(C0)
    weight_sums = w0.copy()
    km._mini_batch_step(Xb, np.ones(B, dtype=dtype), C0.copy(), centers_new, weight_sums, np.random.RandomState(0),
                        random_reassign=False, n_threads=1)
    assert centers_new.dtype == dtype and weight_sums.dtype == dtype
    np.testing.assert_array_equal(r.counts, weight_sums)
    np.testing.assert_array_equal(r.centers, centers_new)
    np.testing.assert_array_equal(r.centers[r.cnts == 0], C0[r.cnts == 0])


def test_step_pieces_on_a_hand_case():
    """Three rows, two centres, numbers whose sums round in float32: the order of the adds is visible in the bits."""
    T = np.float32
    Xb = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=T)
    C = np.array([[1.0], [100.0]], dtype=T)
    w = np.array([1.0, 4.0], dtype=T)
    r = M.step(Xb, C, w)
    assert r.labels.tolist() == [0, 0, 0] and r.cnts.tolist() == [3.0, 0.0]
    # (1 + 1) + 2^-24 + 2^-24 in float32, in batch order: both small terms are lost one after the other
    assert r.centers[0, 0] == T(2.0) * (T(1) / T(4)) and r.counts.tolist() == [4.0, 4.0]
    assert r.centers[1, 0] == 100.0
    assert r.sums[0, 0] == 1.0 + 2.0 ** -23 and r.sums[1, 0] == 0.0      # float64: exact here
    assert r.inertia == 2 * (1.0 - 2.0 ** -24) ** 2


def test_batch_with_counts_gives_the_prescribed_members():
    for name in M.EDGES:
        for dtype in DTYPES:
            X, C0, w0, idx, counts = M.edge_case(name, dtype)
            r = M.step(X[idx], C0, w0)
            assert r.near_ties == 0.0
            np.testing.assert_array_equal(r.cnts, counts)
            assert len(idx) % 64 != 0 or name.startswith("whole")
            assert len(np.unique(idx)) < len(idx)                        # rows repeat
            if name.startswith("tails"):
                assert sorted(set(counts[:10].tolist())) == [0, 1, 2, 3, 5]
                assert (w0 == 0).any() and w0.max() == 100000 and (w0 == np.round(w0)).all()
            else:
                assert (counts > 0).sum() == 1 and not w0.any()


def test_apply_packed_against_exact_rationals():
    rs = np.random.RandomState(3)
    for dtype in DTYPES:
        C = rs.randn(6, 5).astype(dtype)
        w = np.array([0, 1, 7, 100000, 3, 0], dtype=dtype)
        packed = np.concatenate([rs.randn(30) * 3, [2, 0, 5, 1, 0, 4], [1.5]])
        cen, cnt = M.apply_packed(C, w, packed)
        assert cen.dtype == dtype and cnt.dtype == dtype
        np.testing.assert_array_equal(cnt, w + np.array([2, 0, 5, 1, 0, 4], dtype=dtype))
        np.testing.assert_array_equal(cen[[1, 4]], C[[1, 4]])
        v, bound = M.apply_packed_bound(C, w, packed)
        if dtype == np.float64:
            assert (np.abs(cen - v) <= bound).all() and (bound[[1, 4]] == 0).all()
        else:
            assert (np.abs(cen - v) <= 2.0 ** -24 * np.abs(v) + bound).all()     # ... and the rounding to float32
    # a zeroed buffer changes nothing
    cen, cnt = M.apply_packed(C, w, np.zeros(37))
    np.testing.assert_array_equal(cen, C)
    np.testing.assert_array_equal(cnt, w)


def _sklearn_replay(inertias, B, n_samples, max_no_improvement, first_step, state5):
    """MiniBatchKMeans._mini_batch_convergence itself, driven step by step."""
    sk = pytest.importorskip("sklearn.cluster")
    est = sk.MiniBatchKMeans(n_clusters=2, batch_size=B, max_no_improvement=max_no_improvement, tol=0.0, verbose=0)
    est._batch_size = B
    est._tol = 0.0
    est._ewa_inertia = state5[0] if state5[3] else None
    est._ewa_inertia_min = state5[1] if state5[4] else None
    est._no_improvement = int(state5[2])
    steps, fired = 0, False
    for s, inertia in enumerate(inertias):
        steps += 1
        if est._mini_batch_convergence(first_step + s, 10 ** 6, n_samples, 0.0, float(inertia)):
            fired = True
            break
    return est._ewa_inertia, est._ewa_inertia_min, est._no_improvement, steps, fired


@pytest.mark.parametrize("first_step,state5,mni", [
    (0, (0.0, 0.0, 0.0, 0.0, 0.0), 3), (0, (0.0, 0.0, 0.0, 0.0, 0.0), None), (5, (0.071, 0.0705, 1.0, 1.0, 1.0), 2),
    (1, (0.0, 0.0, 0.0, 0.0, 0.0), 0), (7, (3.25, 3.0, 0.0, 1.0, 1.0), 10)])
def test_replay_convergence_is_scikit_learns(first_step, state5, mni):
    rs = np.random.RandomState(first_step + 11)
    B, n = 1000, 7777
    alpha = min(B * 2.0 / (n + 1), 1)
    inertias = (70.0 + 3.0 * rs.rand(40)) * np.linspace(1.0, 1.02, 40)       # noisy, drifting up: the criterion fires
    inertias[10] = inertias[9]                                                 # and an exact repeat
    want = _sklearn_replay(inertias, B, n, mni, first_step, state5)
    st, steps, fired = M.replay_convergence(inertias, B, alpha, -1 if mni is None else mni, first_step, state5)
    assert (steps, fired) == want[3:]
    assert st[5] == steps and st[2] == want[2]
    if want[0] is not None:
        assert st[3] == 1.0 and st[0] == want[0]
    else:
        assert st[3] == 0.0
    if want[1] is not None:
        assert st[4] == 1.0 and st[1] == want[1]
    else:
        assert st[4] == 0.0
    if mni is not None and mni <= 3:
        assert fired and steps < 40
    if mni is None:
        assert not fired and steps == 40
        assert M.replay_convergence(inertias, B, alpha, None, first_step, state5) == (st, steps, fired)


def test_alpha_of_one_and_batch_size_one():
    """alpha = min(2 B / (n + 1), 1) = 1: the average IS the last batch's inertia."""
    st, steps, fired = M.replay_convergence([5.0, 4.0, 3.0, 3.0], 2, 1.0, 1, 0, (0, 0, 0, 0, 0))
    assert st == (1.5, 1.5, 1.0, 1.0, 1.0, 4.0) and steps == 4 and fired


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_gpu_step_inputs_hold_no_near_tie(dtype):
    """Every batch that tests/test_gpu_mbk_step.py labels, by kmeans_label_ref.near_tie_share itself."""
    shapes = set(M.STEP_F64 if dtype == np.float64 else M.STEP_F32) | set(M.STATELESS)
    for B, m, K in sorted(shapes):
        X, C0, w0, idx = M.step_case(B, m, K, dtype)
        assert len(np.unique(idx)) < B                                       # sampled with replacement: rows repeat
        assert R.near_tie_share(X[idx], C0) == 0.0, (B, m, K)
    for name in M.EDGES:
        X, C0, w0, idx, _ = M.edge_case(name, dtype)
        assert R.near_tie_share(X[idx], C0) == 0.0, name


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("name", sorted(M.RUNS))
def test_gpu_run_inputs_hold_no_near_tie_at_any_step(name, dtype):
    """... and at every step of every queued run; the run that must stop early does (on the reference's inertias)."""
    n, m, K, B, S, mni, first_step, _ = M.RUNS[name]
    assert 5 <= S <= 12
    X, C, w, idx = M.run_case(name, dtype)
    steps = M.run_reference(name, dtype)
    for s, r in enumerate(steps):
        assert r.near_ties == 0.0
        assert R.near_tie_share(X[idx[s]], C) == 0.0, (name, s)
        C = r.centers
    if name == "b4100":
        alpha = min(1.0, 2.0 * B / (n + 1))
        _, done, fired = M.replay_convergence([r.inertia for r in steps], B, alpha, mni, first_step, (0, 0, 0, 0, 0))
        assert fired and done == 4 and done < S


KERNEL_NAMES = ("scalar", "v4", "v4-xcd", "label64", "small", "f64")      # MSM_KM_* of include/msmhip.h, in order


def test_cases_sit_on_the_label_kernels_they_name(monkeypatch):
    """The (label kernel, centre splits) that the case tables of mbk_step_ref name are what the library's dispatch
    (msm_kmeans_label_plan: needs no device) gives; the GPU tests assert the same before they run a case."""
    import ctypes
    from msmbuilder_amd import _lib
    monkeypatch.delenv("MSM_LABEL_XCD", raising=False)

    def plan(B, m, K, f64, handle_entry, gathered=False):
        kernel, ns, span = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
        _lib.check(_lib.lib().msm_kmeans_label_plan(B, m, K, int(f64), int(handle_entry), 1, 1, int(gathered), ctypes.byref(kernel),
                                                    ctypes.byref(ns), ctypes.byref(span)))
        return KERNEL_NAMES[kernel.value], ns.value

    for f64, table in ((False, M.STEP_F32), (True, M.STEP_F64)):
        for (B, m, K), want in table.items():
            assert plan(B, m, K, f64, True) == want[:2], (B, m, K, f64)
            assert want[2] == ("small" if B <= 1024 else "general")
    assert {w[:2] for w in M.STEP_F32.values()} >= {("small", 32), ("label64", 1), ("v4", 3), ("scalar", 1), ("small", 1)}
    for (B, m, K), by_type in M.STATELESS.items():
        for f64, want in by_type.items():
            for gathered in (False, True):
                assert plan(B, m, K, f64, False, gathered) == want, (B, m, K, f64, gathered)
    for (name, f64), want in M.EDGE_PLANS.items():
        B, m, K = M.EDGES[name]
        assert plan(B, m, K, f64, True) == want[:2], (name, f64)
        assert want[2] == ("small" if B <= 1024 else "general")
    for (name, f64), want in M.RUN_PLANS.items():
        n, m, K, B = M.RUNS[name][:4]
        assert plan(B, m, K, f64, True) == want, (name, f64)
    assert sorted(M.RUNS[k][3] <= 1024 for k in M.RUNS) == [False, False, True, True]     # both update kernels are queued
