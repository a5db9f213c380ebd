"""The device k-means++ seeding (csrc/kpp.hip: scan, two-level inverse-CDF pick, the two distance kernels, the candidate
gather, the first-minimum pick) through its C entries, against tests/kpp_ref.py: an int64 replay of scikit-learn's
``_kmeans_plusplus`` that the device must reproduce ID FOR ID on lattice rows -- no tolerance, no row left out.

Every case of kpp_ref.CASES runs ``msm_kmeans_plusplus_f32`` / ``_f64`` directly, with the case's own ``first``, ``L`` and
uniforms, on host rows and on device rows, and asserts

  * ``ids`` equal to the replay's (the wrapper throws them away; with duplicate rows equal centres do not imply equal ids);
  * ``centers`` bit for bit ``X[ids]``;
  * the same from both placements.

The table walks the seams: n around the 1024-row scan block and the 32 rows of a wave-per-row workgroup, K == n, F around
the kernel switch (32), the lane stride (64), the gather stride (256) and the 16-byte loads, L = 1 and L = 16 and the
60,000-byte staging tile either side, the pick kernel's chunked prefix (nb = 256, 257, 513, 514) with draws built to land
exactly on block, quad and chunk boundaries and one float above them, the block prefix in device memory (nb = 7168 / 7169),
ties, duplicates, zero potential, u = 0 and the clip to row n - 1.  tests/test_kpp_ref.py shows on the host that each of
them reaches the path it is named for, and that the replay is scikit-learn's own result.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kpp_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def seed(lib, X, K, first, u, L, placement="host"):
    """(centers, ids) of msm_kmeans_plusplus_<type of X> on the rows X, host or device resident; u may be None."""
    n, F = X.shape
    fn = getattr(lib.lib(), "msm_kmeans_plusplus_" + ("f64" if X.dtype == np.float64 else "f32"))
    centers = np.full((max(K, 1), F), np.nan, dtype=X.dtype)
    ids = np.full(max(K, 1), -1, dtype=np.int64)
    if u is not None:
        u = np.ascontiguousarray(u, dtype=np.float64)
        assert u.size >= max(K - 1, 0) * L
    up = u.ctypes.data if u is not None and u.size else None
    if placement == "device":
        import torch
        rows = torch.from_numpy(np.array(X)).cuda()   # (X is read-only: a copy)
        ptr = rows.data_ptr()
    else:
        assert placement == "host" and X.flags.c_contiguous
        ptr = X.ctypes.data
    lib.check(fn(ptr, n, F, K, first, up, L, centers.ctypes.data, ids.ctypes.data, int(placement == "device")))
    return centers[:K], ids[:K]


def assert_is_replay(lib, name, dtype, placements=("host", "device")):
    X, K, first, u, L, _ = P.case_inputs(name, dtype)
    want, _ = P.case_replay(name, dtype)
    for placement in placements:
        centers, ids = seed(lib, X, K, first, u, L, placement)
        wrong = np.nonzero(ids != want)[0]
        assert len(wrong) == 0, (name, dtype, placement, "first wrong round", int(wrong[0]), ids[wrong[:4]], want[wrong[:4]])
        assert np.array_equal(_bits(centers), _bits(X[want])), (name, dtype, placement)


@pytest.mark.parametrize("name,dtype", P.case_ids())
def test_seeding_is_the_replay(gpu, name, dtype):
    assert_is_replay(gpu, name, dtype)


@pytest.mark.parametrize("n,F,K,amp,dtype,placement,rs", [(500, 3, 25, None, np.float32, "host", 0),
                                                          (3000, 33, 50, None, np.float64, "device", 1),
                                                          (1025, 2, 40, 2, np.float32, "device", 2)])
def test_wrapper_draws_what_the_replay_is_given(gpu, n, F, K, amp, dtype, placement, rs):
    """minibatchkmeans.kmeans_plusplus: the same stream, split by wrapper_draws, gives X[replay ids] and the same end state."""
    from msmbuilder_amd.cluster.minibatchkmeans import kmeans_plusplus
    X = P.lattice(n, F, 200 + rs, dtype, amp)
    g_mine, g_ref = np.random.RandomState(rs), np.random.RandomState(rs)
    first, u, L = P.wrapper_draws(n, K, g_ref, dtype)
    want, _ = P.replay(X, K, first, u, dtype)
    rows = X
    if placement == "device":
        import torch
        rows = torch.from_numpy(X).cuda()
    got = kmeans_plusplus(rows, K, g_mine)
    assert got.dtype == dtype and np.array_equal(_bits(got), _bits(X[want]))
    a, b = g_mine.get_state(), g_ref.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    centers, ids = seed(gpu, X, K, first, u, L, "host")   # and the C entry with the same draws: the ids too
    assert np.array_equal(ids, want) and np.array_equal(_bits(centers), _bits(got))


def test_pooled_workspace_reuse(gpu):
    """`best`, the parity of the distance buffers and `pot` live in a pooled workspace: a large call, a small one of the other
    type, the large one again, and every result is the replay's."""
    big, small = ("pick_nb257", "float32"), ("wave_n33_F33", "float64")
    X, K, first, u, L, _ = P.case_inputs(*big)
    c1, i1 = seed(gpu, X, K, first, u, L, "host")
    assert_is_replay(gpu, *small)
    c2, i2 = seed(gpu, X, K, first, u, L, "host")
    assert_is_replay(gpu, *small, placements=("device",))
    c3, i3 = seed(gpu, X, K, first, u, L, "device")
    want, _ = P.case_replay(*big)
    for c, i in ((c1, i1), (c2, i2), (c3, i3)):
        assert np.array_equal(i, want) and np.array_equal(_bits(c), _bits(X[want]))


REFUSALS = [("L=0", dict(L=0)), ("L=17", dict(L=17)), ("K=0", dict(K=0)), ("K>n", dict(K=1026)), ("first=-1", dict(first=-1)),
            ("first=n", dict(first=1025)), ("null u", dict(u=None))]


@pytest.mark.parametrize("dtype", P.BOTH)
@pytest.mark.parametrize("what,change", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refusals_leave_the_next_call_exact(gpu, what, change, dtype):
    name = "n1025_F3"
    X, K, first, u, L, _ = P.case_inputs(name, dtype)
    assert X.shape[0] == 1025 and K > 1
    args = dict(K=K, first=first, u=u, L=L)
    args.update(change)
    if args["u"] is not None:   # a buffer, never null, large enough for the shape asked for: the refusal is the library's own
        args["u"] = np.zeros((max(args["K"] - 1, 1), max(args["L"], 1)))
    with pytest.raises(ValueError, match="kmeans_plusplus"):
        seed(gpu, X, args["K"], args["first"], args["u"], args["L"], "host")
    assert_is_replay(gpu, name, dtype, placements=("host",))


@pytest.mark.parametrize("dtype", P.BOTH)
def test_one_centre_needs_no_uniforms(gpu, dtype):
    X = P.lattice(1025, 3, 5, dtype)
    for first in (0, 512, 1024):
        centers, ids = seed(gpu, X, 1, first, None, 2, "host")
        assert ids.tolist() == [first] and np.array_equal(_bits(centers), _bits(X[[first]]))
