"""CPU tier of the k-means labelling parity rule (tests/kmeans_label_ref.py): the exact reference is what it says it is,
the rule rejects what it must, it stays decidable on the data the GPU tests use, the cases of
tests/test_gpu_kmeans_label_paths.py sit on the seams its docstring names, and the library's own dispatch (km_plan,
asked through msm_kmeans_label_plan: needs no device) is the one that module restates in launch_plan."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_label_ref as R  # noqa: E402
import test_gpu_kmeans_label_paths as P  # noqa: E402

MAX_UNDECIDABLE = 0.02


def _brute(X, C):
    d = ((X[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(-1)
    return d.argmin(1), d


@pytest.mark.parametrize("gen,n,m,K", [("unstructured", 3000, 31, 129), ("lattice", 3000, 4, 130), ("lattice", 500, 64, 513),
                                       ("unstructured", 50, 3, 5)])
def test_exact_argmin_is_the_brute_force_argmin(gen, n, m, K):
    X, C = R.GENERATORS[gen](n, m, K)
    C[K - 1] = C[0]
    ref, dref, sec, dsec = R.exact_argmin(X, C)
    want, d = _brute(X, C)
    np.testing.assert_array_equal(ref, want)            # (numpy's argmin: the first of equal minima)
    np.testing.assert_array_equal(dref, d.min(1))
    np.testing.assert_array_equal(dsec, np.sort(d, axis=1)[:, 1])
    np.testing.assert_array_equal(d[np.arange(n), sec], dsec)
    assert (sec != ref).all()


def test_exact_argmin_many_fold_ties():
    """More equal centres than the shortlist holds: the row falls back to every centre and still gets index 0."""
    X = np.zeros((40, 16), dtype=np.float32)
    C = np.ones((700, 16), dtype=np.float32)
    ref, dref, sec, dsec = R.exact_argmin(X, C)
    assert (ref == 0).all() and (sec == 1).all() and (dref == 16).all() and (dsec == 16).all()


def test_rule_rejects_wrong_labels_and_accepts_only_near_ties():
    n, m, K = 400, 36, 129
    X, C = R.gen_unstructured(n, m, K)
    C[4] = C[1]
    C[100] = C[7]
    C[100, 0] = np.nextafter(C[100, 0], np.float32(np.inf))     # one ulp in one coordinate from centre 7
    X[0] = C[1]
    X[1] = C[7]
    ref, dref, sec, dsec = R.exact_argmin(X, C)
    assert ref[0] == 1 and ref[1] == 7 and sec[1] == 100
    assert R.check_labels(ref.astype(np.int32), X, C, ref, dref) == 0
    lab = ref.copy()
    lab[1] = 100                                        # inside the bound: accepted, and counted
    assert R.check_labels(lab, X, C, ref, dref) == 1
    lab = ref.copy()
    lab[0] = 4                                          # a bit-for-bit copy of the exact centre, higher index: never
    with pytest.raises(AssertionError):
        R.check_labels(lab, X, C, ref, dref)
    clear = np.nonzero(dsec - dref > 1e-3)[0]
    assert len(clear) > n // 2
    lab = ref.copy()
    lab[clear[0]] = sec[clear[0]]                       # ONE row on its runner-up: no allowance for a number of rows
    with pytest.raises(AssertionError):
        R.check_labels(lab, X, C, ref, dref)
    lab = ref.copy()
    lab[5] = K
    with pytest.raises(AssertionError):
        R.check_labels(lab, X, C, ref, dref)


def _shapes():
    out = set()
    for n, m, K in P.F32_SCALAR + P.F32_V4 + P.F32_XCD + P.INERTIA + P.MBK_F32 + [(385, 64, 130)]:
        out.add(("unstructured", m, K, False))
    for n, m, K in P.F64 + P.MBK_F64:
        out.add(("unstructured", m, K, True))
    for n, m, K, f64 in P.NAN + P.MERGE:
        out.add(("unstructured", m, K, f64))
    for n, m, K in P.OFFSET:
        out.add(("offset", m, K, False))
    return sorted(out)


@pytest.mark.parametrize("gen,m,K,f64", _shapes())
def test_rule_decides_nearly_every_row(gen, m, K, f64):
    """At most 2 % of rows may have their exact best and second-best centre within the two bounds of each other -- beyond
    that the rule would accept too much to mean anything.  A property of the generator at (m, K) (its rows are
    independent draws): estimated on 8,192 rows.  (The lattice generator is not held to the rule but to equality.)"""
    X, C = R.GENERATORS[gen](8192, m, K, np.float64 if f64 else np.float32)
    assert R.near_tie_share(X, C) <= MAX_UNDECIDABLE


def test_offset_shift_is_the_largest_that_stays_decidable():
    """Of the shifts 10, 3, 1 the offset generator uses the largest that keeps every shape it is used at under the 2 % cap,
    measured at the shape's own row count (capped at 20,000).  Measured shares: +10: 1.9 % at (257,36,129), 4.1 % at
    (.,64,513): over; +3: 0.8 % and 0.4 %: chosen."""
    def worst(shift):
        return max(R.near_tie_share(*R.gen_offset(min(n, 20000), m, K, shift=shift)) for n, m, K in P.OFFSET)
    assert worst(10.0) > MAX_UNDECIDABLE
    assert worst(3.0) <= MAX_UNDECIDABLE
    assert R.OFFSET_SHIFT == 3.0


KERNEL_NAMES = ("scalar", "v4", "v4-xcd", "label64", "small", "f64")      # MSM_KM_* of include/msmhip.h, in order


def library_plan(n, m, K, f64=False, entry="label", inertia=True, aligned=True, gathered=False):
    """(kernel, centre splits, centres per split) as the library's km_plan decides them; MSM_LABEL_XCD is read per call."""
    from msmbuilder_amd import _lib
    kernel, ns, span = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    _lib.check(_lib.lib().msm_kmeans_label_plan(n, m, K, int(f64), int(entry == "mbk"), int(inertia), int(aligned), int(gathered),
                                                ctypes.byref(kernel), ctypes.byref(ns), ctypes.byref(span)))
    return KERNEL_NAMES[kernel.value], ns.value, span.value


SWEEP_N = (1, 64, 127, 128, 129, 4096, 4097, 32640, 32641, 65408, 65409, 65536, 65537, 131072)
SWEEP_M = (1, 3, 4, 31, 32, 33, 36, 64, 512)
SWEEP_K = (1, 2, 16, 17, 128, 129, 257, 300, 513, 1000, 2048, 2049, 8321)


def test_library_plan_equals_the_restated_dispatch(monkeypatch):
    """msm_kmeans_label_plan against launch_plan over the full product of the seam values: every threshold of the
    dispatch from both sides, both row types, both entries, with and without inertia, aligned or not, and the four
    settings of MSM_LABEL_XCD the tests use."""
    monkeypatch.delenv("MSM_MBK_SMALL", raising=False)
    checked = 0
    for xcd in (None, "0", "1", "3"):
        if xcd is None:
            monkeypatch.delenv("MSM_LABEL_XCD", raising=False)
        else:
            monkeypatch.setenv("MSM_LABEL_XCD", xcd)
        tiles = 4 if xcd is None else int(xcd)
        for n, m, K, f64, entry, inertia, aligned in itertools.product(SWEEP_N, SWEEP_M, SWEEP_K, (False, True), ("label", "mbk"),
                                                                        (True, False), (True, False)):
            want = P.launch_plan(n, m, K, f64=f64, entry=entry, inertia=inertia, xcd_tiles=tiles, aligned=aligned)
            got = library_plan(n, m, K, f64=f64, entry=entry, inertia=inertia, aligned=aligned)
            assert got == want, (n, m, K, f64, entry, inertia, aligned, xcd, got, want)
            checked += 1
    assert checked == 4 * len(SWEEP_N) * len(SWEEP_M) * len(SWEEP_K) * 16


def test_cases_sit_on_their_seams(monkeypatch):
    """The dispatch restated in launch_plan (row blocks and centre tiles of 128; XCD launch from 512 row blocks, m >= 64
    and 5..16 tiles; float64 / handle splits below 256 row blocks; the handle's small-batch kernels) puts every case on the
    path its module docstring names -- and so does the library's own plan."""
    monkeypatch.delenv("MSM_LABEL_XCD", raising=False)
    monkeypatch.delenv("MSM_MBK_SMALL", raising=False)
    for (n, m, K, f64, entry), (kernel, ns) in P.SEAMS.items():
        assert P.launch_plan(n, m, K, f64=f64, entry=entry)[:2] == (kernel, ns), (n, m, K, f64, entry)
        assert library_plan(n, m, K, f64=f64, entry=entry)[:2] == (kernel, ns), (n, m, K, f64, entry)
    listed = {k[:4] + (k[4],) for k in P.SEAMS}
    for n, m, K in P.F32_SCALAR + P.F32_V4 + P.F32_XCD:
        assert (n, m, K, False, "label") in listed
    for n, m, K in P.F64:
        assert (n, m, K, True, "label") in listed
    for n, m, K in P.MBK_F32:
        assert (n, m, K, False, "mbk") in listed
    for n, m, K, f64 in P.MERGE + P.NAN:
        assert P.launch_plan(n, m, K, f64=f64)[1] > 1           # split shapes: candidates are merged
    assert P.launch_plan(65537, 64, 513, xcd_tiles=1)[1:] == (5, 128)
    assert P.launch_plan(65537, 64, 513, xcd_tiles=3)[1:] == (2, 384)
    assert P.launch_plan(65409, 64, 513)[2] == 384              # tiles 0-2 | tiles 3-4, the last with one centre
    assert P.launch_plan(385, 64, 130, aligned=False)[0] == "scalar"
    assert P.launch_plan(100, 4, 8321, f64=True)[1] > 64        # the merge loop takes a second round of 64 lanes
    # planted pairs that take centre K - 1 give the case a second variant with K - 1 unique
    assert P.variants(129, P.launch_plan(257, 31, 129)) == ("dups", "last")
    assert P.variants(257, P.launch_plan(32640, 4, 257, f64=True)) == ("dups", "last")
    assert P.variants(513, P.launch_plan(65409, 64, 513)) == ("dups",)
