"""Every launch path of the k-means labelling code (csrc/kmeans.hip, kmeans_*_dev.h) against an exact float64 argmin.

The reference and the acceptance rule live in tests/kmeans_label_ref.py (plain numpy, by direct difference): a label that
differs from the exact one passes only inside the derived forward-error bound of the GEMM form, never between bit-identical
centres, and EVERY row is checked.  Inertia: the exact sum over the kernel's own labels, rtol 3 * 2^-24 (float32 rows) or
1e-12 (float64 rows).  The data is unstructured (randn rows, randn centres) so that near-ties are ordinary; tests/test_kmeans_label_rule.py
keeps the rule from becoming vacuous on it (at most 2 % of rows undecidable).

Planted in every case (``_case``):
  * C[4] = C[1] (K > 4), C[128] = C[127] (K > 128: the pair straddles a 128-centre tile), C[b] = C[b - 1] at every
    boundary b between two centre splits of the launch the shape takes (``launch_plan``);
  * rows that are exact copies of centres (the lower one of a duplicated pair: the label must be the LOWER index) at the
    first and last row of row block 0 and of a middle row block, and row n - 1 = C[K - 1];
  * centre K - 1 is then the unique nearest centre of row n - 1 -- unless K - 1 itself belongs to a planted pair
    (K = 129: the tile pair; K = 257 in two float64 splits: the split pair).  Those shapes run a second time as variant
    "last" without that pair, so that a dropped one-centre tail tile is caught there.

Which case reaches which seam (``launch_plan`` is an independent restatement of the dispatch, the library's km_plan;
test_kmeans_label_rule.py pins this table against both and holds km_plan, through msm_kmeans_label_plan, to launch_plan):
  * kmeans_label_kernel (m % 4 != 0): (129,1,2) one feature, (257,31,129) partial K-step + one-centre tail tile,
    (300,33,257) one full K-step + remainder 1, (385,130,130) four full steps + remainder 2, two-centre tail tile;
    and the misaligned device view (m = 64, base 4 bytes into its allocation): the 16-byte kernel must be refused.
  * kmeans_label_v4_kernel: (300,4,130) one 16-byte group, (257,36,129) full step + one group, (1000,512,1000) 16 steps x
    8 tiles, (128,64,128) exactly one full block and tile, (129,64,129) one row and one centre beyond them.
  * XCD-grouped launch (m = 64): (65408,513) 511 row blocks, not XCD; (65409,512) 512 blocks but 4 tiles, no split;
    (65409,513) 512 blocks (last one partial), 5 tiles in 2 splits, last tile holds one centre; (65537,513) and
    (65537,2048) 513 blocks padded to 520 (phantom blocks), 2 and 4 splits; (65537,2049) 17 tiles, not XCD;
    MSM_LABEL_XCD = 1 / 3 at (65537,513): 5 and 2 splits.
  * kmeans_inertia_kernel: n in {1,2,7,8,9,16384,16385,16391} x m in {6 (scalar), 8 (16-byte)}: the odd tail of the
    two-rows-per-wave loop (has1) and the 2,048-partial cap (n > 16,384).
  * kmeans_label_f64_kernel: (32640,4,257) 255 row blocks, 2 splits; (32641,4,257) 256 blocks, no split; (100,4,129)
    2 splits; (100,4,8321) 66 splits: the q0 += 64 loop of the inertia kernel's merge; (300,17,300) 3 splits.
  * both merge routes: msm_kmeans_label_* with a null inertia pointer merges in kmeans_label_reduce_kernel, with one in
    kmeans_inertia_kernel: identical labels required on the split shapes.
  * msm_mbk_label: (4096,64,300) kmeans_label64_kernel in 5 splits of 64, (4097,64,300) the general kernel in 3 splits,
    (65536,32,100) mbk_small_label_kernel, (65537,32,100) the general kernel; (100,4,8321) float64; (300,33,100) and
    (200,67,60) kmeans_label64_kernel at widths that are no multiple of 4 (the last, partial group of four features of
    a row), the second in ONE split (K <= 64): the kernel writes the labels itself, nothing is merged.
  * offset data (everything + 3): (257,36,129), (65409,64,513).
  * NaN rows (labels only): an all-NaN row and a row with one NaN, each at the first row of a block and at row n - 1.
  * integer lattices: every float32 operation of the GEMM form is exact, exact ties between DIFFERENT centres are common
    (also across tile and split seams): the label must equal the exact one on every row.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_label_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KR = KCT = 128


def _cdiv(a, b):
    return -(-a // b)


def _small_splits(n, K):
    """Centre splits of a small batch: (number of centre splits, centres per split)."""
    rowblocks, ctiles = _cdiv(n, KR), _cdiv(K, KCT)
    ns = min(ctiles, max(1, 512 // rowblocks)) if rowblocks < 256 and ctiles > 1 else 1
    tiles_per = _cdiv(ctiles, ns)
    return _cdiv(ctiles, tiles_per), tiles_per * KCT


def _xcd_splits(n, m, K, tiles_per=4, aligned=True):
    """The XCD-grouped launch: (number of centre splits or 0, centres per split)."""
    rowblocks, ctiles = _cdiv(n, KR), _cdiv(K, KCT)
    if tiles_per <= 0 or not aligned or m % 4 or m < 64 or ctiles < 2 or ctiles > 16 or rowblocks < 512:
        return 0, 0
    ns = _cdiv(ctiles, tiles_per)
    return (ns, _cdiv(ctiles, ns) * KCT) if ns > 1 else (0, 0)


def launch_plan(n, m, K, f64=False, entry="label", inertia=True, xcd_tiles=4, aligned=True):
    """(kernel, centre splits, centres per split) of a labelling call, restated from the dispatch in kmeans.hip (km_plan)."""
    v4 = "v4" if (m % 4 == 0 and aligned) else "scalar"
    if f64:
        ns, span = _small_splits(n, K)
        return "f64", ns, span
    if entry == "mbk":
        if inertia and m <= 32 and n <= 65536:
            ns = max(1, min(_cdiv(512, _cdiv(n, 64)), _cdiv(K, 16)))
            cper = min(_cdiv(K, ns), 128)
            return "small", _cdiv(K, cper), cper
        if n <= 4096 and m > 32:
            rb, ct = _cdiv(n, 64), _cdiv(K, 64)
            tiles_per = _cdiv(ct, min(ct, max(1, _cdiv(512, rb))))
            return "label64", _cdiv(ct, tiles_per), tiles_per * 64
        ns, span = _small_splits(n, K)
        if ns > 1:
            return v4, ns, span
    ns, span = _xcd_splits(n, m, K, xcd_tiles, aligned)
    if ns:
        return "v4-xcd", ns, span
    return v4, 1, K


def _pairs(K, plan, variant):
    """Duplicated centre pairs (lower, upper) of a case."""
    _, ns, span = plan
    pairs = []
    if K > 4:
        pairs.append((1, 4))
    if K > 128:
        pairs.append((127, 128))
    for s in range(1, ns):
        b = s * span
        if 0 < b < K and (b - 1, b) not in pairs:
            pairs.append((b - 1, b))
    if variant == "last":
        pairs = [p for p in pairs if K - 1 not in p]
    return pairs


def variants(K, plan):
    """("dups",), and "last" too where a planted pair takes centre K - 1."""
    return ("dups", "last") if any(K - 1 in p for p in _pairs(K, plan, "dups")) else ("dups",)


@functools.lru_cache(maxsize=None)
def _case(gen, n, m, K, f64, plan, variant):
    """Planted data of a case and its exact reference, computed once: X, C, ref, d_ref, planted rows."""
    dtype = np.float64 if f64 else np.float32
    X, C = R.GENERATORS[gen](n, m, K, dtype, seed=n + K)
    pairs = _pairs(K, plan, variant)
    for lo, hi in pairs:
        C[hi] = C[lo]
    mid = KR * ((n - 1) // KR // 2)
    rows = sorted({r for r in (0, KR - 1, mid, mid + KR - 1) if r < n - 1})
    targets = [lo for lo, _ in pairs] + [K - 1]
    for k, r in enumerate(rows):
        X[r] = C[targets[k % len(targets)]]
    X[n - 1] = C[K - 1]
    ref, dref, _, _ = R.exact_argmin(X, C)
    assert dref[n - 1] == 0.0 and all(dref[r] == 0.0 for r in rows)
    if gen != "lattice" and not any(K - 1 in p for p in pairs):   # (a lattice may hold a copy of C[K - 1] by chance)
        assert ref[n - 1] == K - 1
    for a in (X, C, ref, dref):
        a.setflags(write=False)
    return X, C, ref, dref, tuple(rows) + (n - 1,)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _placements(X):
    import torch
    return (("host", X), ("device", torch.from_numpy(np.array(X)).cuda()))   # (X is read-only: a copy)


def _label_c(rows, Cn, want_inertia):
    """msm_kmeans_label_f32 / _f64 straight through ctypes (a null inertia pointer: labels only)."""
    from msmbuilder_amd import _lib
    ax = _lib.Arr(rows, Cn.dtype)
    labels = _lib.empty_like_placement(ax, (ax.shape[0],), np.int32)
    al = _lib.Arr(labels, np.int32)
    inertia = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_kmeans_label_" + ("f64" if Cn.dtype == np.float64 else "f32"))
    _lib.check(fn(ax.vp, ax.shape[0], ax.shape[1], Cn.ctypes.data, Cn.shape[0], al.vp,
                  C.byref(inertia) if want_inertia else None, ax.on_device))
    return _np(labels), (inertia.value if want_inertia else None)


def _mbk_label(rows, Cn, want_inertia=True):
    """msm_mbk_label on a handle that holds the centres Cn."""
    from msmbuilder_amd import _lib
    L = _lib.lib()
    ax = _lib.Arr(rows, Cn.dtype)
    K, m = Cn.shape
    h = C.c_void_p()
    _lib.check((L.msm_mbk_create_f64 if Cn.dtype == np.float64 else L.msm_mbk_create)(C.byref(h), K, m))
    try:
        counts = np.zeros(K, dtype=Cn.dtype)
        cen = np.ascontiguousarray(Cn)
        _lib.check(L.msm_mbk_set(h, cen.ctypes.data, counts.ctypes.data))
        labels = _lib.empty_like_placement(ax, (ax.shape[0],), np.int32)
        al = _lib.Arr(labels, np.int32)
        inertia = C.c_double(0.0)
        _lib.check(L.msm_mbk_label(h, ax.vp, ax.shape[0], al.vp, C.byref(inertia) if want_inertia else None, ax.on_device))
        _lib.synchronize()
    finally:
        L.msm_mbk_destroy(h)
    return _np(labels), (inertia.value if want_inertia else None)


def _check(lab, inertia, X, Cn, ref, dref, planted=(), strict=False):
    assert lab.dtype == np.int32 and lab.shape == (X.shape[0],)
    if strict:
        np.testing.assert_array_equal(lab, ref)
    R.check_labels(lab, X, Cn, ref, dref)
    for r in planted:              # exact copies of a centre: nothing is near 0, the exact label or nothing
        assert lab[r] == ref[r], (r, lab[r], ref[r])
    if inertia is not None:
        np.testing.assert_allclose(inertia, R.exact_inertia(X, Cn, lab), rtol=R.inertia_rtol(X.dtype), atol=0)


def _run_case(n, m, K, f64=False, gen="unstructured", entry="label", strict=False):
    from msmbuilder_amd.cluster.minibatchkmeans import label_inertia
    plan = launch_plan(n, m, K, f64=f64, entry=entry)
    for variant in variants(K, plan):
        X, Cn, ref, dref, planted = _case(gen, n, m, K, f64, plan, variant)
        for _, rows in _placements(X):
            if entry == "mbk":
                lab, inertia = _mbk_label(rows, Cn)
            else:
                lab, inertia = label_inertia(rows, Cn)
                lab = _np(lab)
            _check(lab, inertia, X, Cn, ref, dref, planted, strict)


F32_SCALAR = [(129, 1, 2), (257, 31, 129), (300, 33, 257), (385, 130, 130)]
F32_V4 = [(300, 4, 130), (257, 36, 129), (1000, 512, 1000), (128, 64, 128), (129, 64, 129)]
F32_XCD = [(65408, 64, 513), (65409, 64, 512), (65409, 64, 513), (65537, 64, 513), (65537, 64, 2048), (65537, 64, 2049)]
INERTIA = [(n, m, 10) for m in (6, 8) for n in (1, 2, 7, 8, 9, 16384, 16385, 16391)]
F64 = [(32640, 4, 257), (32641, 4, 257), (100, 4, 129), (100, 4, 8321), (300, 17, 300)]
MBK_F32 = [(4096, 64, 300), (4097, 64, 300), (65536, 32, 100), (65537, 32, 100), (300, 33, 100), (200, 67, 60)]
MBK_F64 = [(100, 4, 8321)]
OFFSET = [(257, 36, 129), (65409, 64, 513)]
NAN = [(65409, 64, 513, False), (100, 4, 8321, True), (32640, 4, 257, True)]
LATTICE = [(300, 4, 130, False), (257, 3, 129, False), (65409, 64, 513, False), (100, 4, 8321, True), (32640, 4, 257, True)]
MERGE = [(65409, 64, 513, False), (100, 4, 8321, True), (32640, 4, 257, True), (300, 17, 300, True)]

# (n, m, K, f64, entry) -> the path the case is there for (pinned against launch_plan by tests/test_kmeans_label_rule.py)
SEAMS = {
    (129, 1, 2, False, "label"): ("scalar", 1), (257, 31, 129, False, "label"): ("scalar", 1),
    (300, 33, 257, False, "label"): ("scalar", 1), (385, 130, 130, False, "label"): ("scalar", 1),
    (300, 4, 130, False, "label"): ("v4", 1), (257, 36, 129, False, "label"): ("v4", 1),
    (1000, 512, 1000, False, "label"): ("v4", 1), (128, 64, 128, False, "label"): ("v4", 1),
    (129, 64, 129, False, "label"): ("v4", 1),
    (65408, 64, 513, False, "label"): ("v4", 1), (65409, 64, 512, False, "label"): ("v4", 1),
    (65409, 64, 513, False, "label"): ("v4-xcd", 2), (65537, 64, 513, False, "label"): ("v4-xcd", 2),
    (65537, 64, 2048, False, "label"): ("v4-xcd", 4), (65537, 64, 2049, False, "label"): ("v4", 1),
    (32640, 4, 257, True, "label"): ("f64", 2), (32641, 4, 257, True, "label"): ("f64", 1),
    (100, 4, 129, True, "label"): ("f64", 2), (100, 4, 8321, True, "label"): ("f64", 66),
    (300, 17, 300, True, "label"): ("f64", 3),
    (4096, 64, 300, False, "mbk"): ("label64", 5), (4097, 64, 300, False, "mbk"): ("v4", 3),
    (65536, 32, 100, False, "mbk"): ("small", 1), (65537, 32, 100, False, "mbk"): ("v4", 1),
    (100, 4, 8321, True, "mbk"): ("f64", 66),
    (300, 33, 100, False, "mbk"): ("label64", 2), (200, 67, 60, False, "mbk"): ("label64", 1),
}


@pytest.mark.parametrize("n,m,K", F32_SCALAR + F32_V4)
def test_label_f32_tile_kernels(gpu, n, m, K):
    _run_case(n, m, K)


@pytest.mark.parametrize("n,m,K", F32_XCD)
def test_label_f32_xcd_launch(gpu, n, m, K):
    _run_case(n, m, K)


def test_label_f32_xcd_tiles_per_workgroup(gpu, monkeypatch):
    """MSM_LABEL_XCD = 1 (five splits of one tile) and 3 (two splits) at (65537, 64, 513): the default's labels."""
    from msmbuilder_amd.cluster.minibatchkmeans import label_inertia
    n, m, K = 65537, 64, 513
    X, Cn, ref, dref, planted = _case("unstructured", n, m, K, False, launch_plan(n, m, K), "dups")
    monkeypatch.delenv("MSM_LABEL_XCD", raising=False)
    lab0, inertia0 = label_inertia(X, Cn)
    _check(lab0, inertia0, X, Cn, ref, dref, planted)
    for tiles_per in ("1", "3"):
        monkeypatch.setenv("MSM_LABEL_XCD", tiles_per)
        lab, inertia = label_inertia(X, Cn)
        np.testing.assert_array_equal(lab, lab0)
        np.testing.assert_allclose(inertia, inertia0, rtol=1e-12, atol=0)


def test_label_f32_misaligned_device_view(gpu):
    """Device rows that start 4 bytes into their allocation (m = 64): the wrapper hands the view on as it is (no copy to
    an aligned buffer), and labelling must be right on it -- neither the 16-byte label kernel nor the 16-byte path of
    the inertia kernel may be taken for such a base."""
    import torch
    from msmbuilder_amd import _lib
    from msmbuilder_amd.cluster.minibatchkmeans import label_inertia
    n, m, K = 385, 64, 130
    X, Cn, ref, dref, planted = _case("unstructured", n, m, K, False, launch_plan(n, m, K, aligned=False), "dups")
    buf = torch.empty(n * m + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(n, m)
    view.copy_(torch.from_numpy(np.array(X)))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + 4 and view.is_contiguous()
    assert _lib.Arr(view, np.float32).ptr == view.data_ptr()
    lab, inertia = label_inertia(view, Cn)
    _check(_np(lab), inertia, X, Cn, ref, dref, planted)


@pytest.mark.parametrize("n,m,K", INERTIA)
def test_inertia_kernel_tails_and_partials_cap(gpu, n, m, K):
    _run_case(n, m, K)


@pytest.mark.parametrize("n,m,K", F64)
def test_label_f64_centre_splits(gpu, n, m, K):
    _run_case(n, m, K, f64=True)


@pytest.mark.parametrize("n,m,K,f64", MERGE)
def test_label_both_merge_routes(gpu, n, m, K, f64):
    """A null inertia pointer sends the splits' candidates through kmeans_label_reduce_kernel, a non-null one through the
    merge inside kmeans_inertia_kernel: the same labels, and right ones."""
    plan = launch_plan(n, m, K, f64=f64)
    assert plan[1] > 1
    X, Cn, ref, dref, planted = _case("unstructured", n, m, K, f64, plan, "dups")
    for _, rows in _placements(X):
        lab_r, none = _label_c(rows, Cn, False)
        lab_i, inertia = _label_c(rows, Cn, True)
        assert none is None
        np.testing.assert_array_equal(lab_r, lab_i)
        _check(lab_r, inertia, X, Cn, ref, dref, planted)


@pytest.mark.parametrize("n,m,K,f64", [s + (False,) for s in MBK_F32] + [s + (True,) for s in MBK_F64])
def test_mbk_label_handle(gpu, n, m, K, f64):
    _run_case(n, m, K, f64=f64, entry="mbk")
    # ... and without an inertia (the reduce kernel after label64 / split launches; the general kernels for narrow rows)
    plan = launch_plan(n, m, K, f64=f64, entry="mbk")
    X, Cn, ref, dref, planted = _case("unstructured", n, m, K, f64, plan, "dups")
    lab, _ = _mbk_label(X, Cn, want_inertia=False)
    _check(lab, None, X, Cn, ref, dref, planted)


@pytest.mark.parametrize("n,m,K", OFFSET)
def test_label_offset_data(gpu, n, m, K):
    """Rows and centres moved away from the origin by kmeans_label_ref.OFFSET_SHIFT = 3 (the largest of 10, 3, 1 that
    leaves at most 2 % of rows undecidable at these shapes: tests/test_kmeans_label_rule.py)."""
    _run_case(n, m, K, gen="offset")


@pytest.mark.parametrize("n,m,K,f64", LATTICE)
def test_label_exact_ties_on_a_lattice(gpu, n, m, K, f64):
    _run_case(n, m, K, f64=f64, gen="lattice", strict=True)


@pytest.mark.parametrize("n,m,K,f64", NAN)
def test_label_nan_rows(gpu, n, m, K, f64):
    """An all-NaN row and a row with a single NaN, each at the first row of a block and at row n - 1 (one call per
    placement): label 0 there, every other row still by the rule.  (The inertia of such a call is NaN: not checked.)"""
    from msmbuilder_amd.cluster.minibatchkmeans import label_inertia
    plan = launch_plan(n, m, K, f64=f64)
    X, Cn, ref, dref, planted = _case("unstructured", n, m, K, f64, plan, "dups")
    first = KR * ((n - 1) // KR)          # the first row of the last row block ...
    if first == n - 1:
        first -= KR                       # ... or of the one before it, where the last block is that one row
    for nan_rows in ((first, n - 1), (n - 1, first)):      # (all-NaN row, single-NaN row)
        Xn = X.copy()
        Xn[nan_rows[0]] = np.nan
        Xn[nan_rows[1], m // 2] = np.nan
        for _, rows in _placements(Xn):
            for lab in (_np(label_inertia(rows, Cn)[0]), _label_c(rows, Cn, False)[0]):
                assert lab[nan_rows[0]] == 0 and lab[nan_rows[1]] == 0
                R.check_labels(lab, X, Cn, ref, dref, skip=nan_rows)
                for r in planted:
                    assert r in nan_rows or lab[r] == ref[r]
