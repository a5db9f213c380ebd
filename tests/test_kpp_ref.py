"""CPU tier of the k-means++ replay (tests/kpp_ref.py): on float64 lattice rows it IS scikit-learn's
``kmeans_plusplus`` id for id, generator state included; on float32 lattice rows it IS the float64 restatement the large
device comparisons use (oracle/kpp_oracle.py); every named case of the table reaches the path it is named for -- a GPU
case that silently missed its path would test nothing; and the replay refuses inputs on which it would not be exact."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kpp_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, F, K, amp): shapes with ties and zero potentials first, then the small shapes of the case table
SKLEARN_SHAPES = [(500, 3, 25, None), (1025, 2, 40, None), (3000, 33, 50, None), (40, 32, 40, None), (50, 2, 50, 1),
                  (1025, 2, 40, 2)]
SKLEARN_SHAPES += sorted({(c.n, c.F, c.K, c.amp) for c in P.CASES.values() if c.small} - set(SKLEARN_SHAPES),
                         key=lambda t: (t[0], t[1], t[2], t[3] or 0))
ORACLE_SHAPES = [(500, 3, 25, None), (1025, 2, 40, 2), (50, 2, 50, 1), (300, 257, 6, None), (2000, 938, 20, None),
                 (300000, 2, 6, None)]


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("n,F,K,amp", SKLEARN_SHAPES)
def test_replay_is_scikit_learns_kmeans_plusplus(n, F, K, amp):
    import sklearn.cluster as sk   # (a dependency of the package itself)
    for seed in (0, 1, 2):
        X = P.lattice(n, F, 100 + seed, np.float64, amp)
        g_mine, g_ref = np.random.RandomState(seed), np.random.RandomState(seed)
        first, u, L = P.wrapper_draws(n, K, g_mine, np.float64)
        ids, _ = P.replay(X, K, first, u, np.float64)
        ref, ref_ids = sk.kmeans_plusplus(X, K, random_state=g_ref)
        assert np.array_equal(ids, ref_ids), (seed, np.nonzero(ids != ref_ids)[0][:5])
        assert np.array_equal(X[ids], ref)
        assert _same_state(g_mine, g_ref)


def test_scikit_learn_comparison_sees_ties_and_zero_potential():
    """The comparison above is not only of generic rounds: (50, 2, K = 50) at amplitude 1 has tied and zero-potential
    rounds under the wrapper's draws as well."""
    X = P.lattice(50, 2, 100, np.float64, 1)
    first, u, L = P.wrapper_draws(50, 50, np.random.RandomState(0), np.float64)
    _, stats = P.replay(X, 50, first, u, np.float64)
    assert stats["tied_rounds"] >= 10 and stats["zero_pot_rounds"] >= 10 and stats["zero_bin"] >= 10


@pytest.mark.parametrize("n,F,K,amp", ORACLE_SHAPES)
def test_replay_is_the_float64_restatement_on_float32_rows(n, F, K, amp):
    from oracle.kpp_oracle import kmeans_plusplus_f64
    X = P.lattice(n, F, 7, np.float32, amp)
    g_mine, g_ref = np.random.RandomState(3), np.random.RandomState(3)
    first, u, L = P.wrapper_draws(n, K, g_mine, np.float32)
    ids, _ = P.replay(X, K, first, u, np.float32)
    ref, ref_ids = kmeans_plusplus_f64(X, K, g_ref)
    assert np.array_equal(ids, ref_ids)
    assert np.array_equal(X[ids], ref) and _same_state(g_mine, g_ref)


@pytest.mark.parametrize("name,dtype", [(n, d) for n, d in P.case_ids() if P.CASES[n].expect])
def test_named_case_reaches_its_path(name, dtype):
    case = P.CASES[name]
    X, K, first, u, L, plan = P.case_inputs(name, dtype)
    ids, stats = P.case_replay(name, dtype)
    for key, least in case.expect.items():
        assert stats[key] >= least, (key, stats[key], least)
    if case.draws == "edge":
        # every constructed draw lands on the row it was built for, the 'edge' ones with u * pot == cum[row] exactly
        assert len(plan) >= 2 * min(K - 1, 2)
        for p in plan:
            assert stats["cands"][p.round][p.slot] == p.row, p
        assert stats["on_edge"] >= sum(p.kind == "edge" for p in plan)
        assert all(abs(p.row - p.want) <= 8 for p in plan if p.kind == "edge")   # a target moves to a neighbour at most
        assert ((0 <= u) & (u < 1)).all()


def test_edge_uniforms_products_are_exact():
    """Independently of replay's counters: walk edge_small by hand and check each constructed product against the int64
    cumulative sums."""
    X, K, first, u, L, plan = P.case_inputs("edge_small", "float32")
    Xi = X.astype(np.int64)
    closest = ((Xi - Xi[first]) ** 2).sum(1)
    ids, stats = P.case_replay("edge_small", "float32")
    by_round = {}
    for p in plan:
        by_round.setdefault(p.round, []).append(p)
    for rnd in range(K - 1):
        cum = np.cumsum(closest)
        pot = np.float64(np.float32(np.float64(int(cum[-1]))))
        for p in by_round.get(rnd, []):
            r = u[rnd, p.slot] * pot
            if p.kind == "edge":
                assert r == float(cum[p.row]) and closest[p.row] > 0
            else:
                edge = u[rnd, p.slot - 1] * pot
                assert edge < r < edge + 1 and (p.row == len(cum) - 1 or (cum[p.row - 1] < r <= cum[p.row]))
        closest = np.minimum(closest, ((Xi - Xi[ids[rnd + 1]]) ** 2).sum(1))
    assert len(plan) == 2 * (L // 2) * (K - 1)


def test_replay_refuses_inexact_inputs():
    u = np.full((1, 2), 0.5)
    X = P.lattice(20, 2, 0, np.float64)
    P.replay(X, 2, 0, u, np.float64)
    with pytest.raises(AssertionError, match="integer-valued"):
        P.replay(X + 0.5, 2, 0, u, np.float64)
    with pytest.raises(AssertionError, match="finite"):
        P.replay(np.where(np.arange(40).reshape(20, 2) == 3, np.nan, X), 2, 0, u, np.float64)
    far = np.array([[-2048.0], [2048.0], [0.0]])   # 4096^2 = 2^24: not below it
    with pytest.raises(AssertionError, match="does not fit"):
        P.replay(far.astype(np.float32), 2, 0, u, np.float32)
    ids, _ = P.replay(far, 2, 0, u, np.float64)   # float64 rows: exact, and the far row is drawn
    assert ids.tolist() == [0, 1]
    with pytest.raises(AssertionError, match="2\\^53"):
        P._round(2 ** 53, np.float64)
    with pytest.raises(AssertionError):
        P.lattice(10, 938, 0, np.float32, amp=67)     # 938 x 134^2 > 2^24
    assert 938 * (2 * P.max_amp(938)) ** 2 < 2 ** 24 <= 938 * (2 * (P.max_amp(938) + 1)) ** 2


def test_clip_needs_a_potential_rounded_up():
    """The clip case: where float32 rounds the potential UP, (1 - 2^-53) pot lies beyond the last bin and the draw is row
    n - 1; u = 0 in the same call is row 0; float64 rows cannot clip."""
    for name in ("clip_seed0", "clip_seed4"):
        X, K, first, u, L, _ = P.case_inputs(name, "float32")
        ids, stats = P.case_replay(name, "float32")
        assert stats["clipped"] >= 1 and all(c[0] == 0 for c in stats["cands"])
        _, s64 = P.replay(X.astype(np.float64), K, first, u, np.float64)
        assert s64["clipped"] == 0
    # the first round of clip_visible by hand: the total rounds up, so the product exceeds it
    X, K, first, u, L, _ = P.case_inputs("clip_visible", "float32")
    total = int(((X.astype(np.int64) - X[first].astype(np.int64)) ** 2).sum())
    assert float(np.float32(np.float64(total))) > total
    assert u[0, 0] * np.float64(np.float32(np.float64(total))) > total
    # clip_visible: the clipped draw is the pick, and a draw that is not clipped is a different row
    ids, stats = P.case_replay("clip_visible", "float32")
    assert ids.tolist() == [first, len(X) - 1, len(X) - 1]


def test_case_table_straddles_the_kernels_thresholds():
    """The seam sizes of the table are those of msmbuilder_amd/csrc/kpp.hip as it stands."""
    src = open(os.path.join(ROOT, "msmbuilder_amd", "csrc", "kpp.hip")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (const("KPP_NT"), const("KPP_RPB"), const("KPP_LMAX"), const("KPP_WROWS")) == (P.NT, P.RPB, P.LMAX, 32)
    assert int(re.search(r"sizeof\(T\) > (\d+);", src).group(1)) == P.TILE_BYTES
    assert int(re.search(r"longpre = nb > (\d+);", src).group(1)) == P.LONGPRE_NB
    assert re.search(r"wrows = F >= 32 ", src)
    assert 937 * 16 * 4 <= P.TILE_BYTES < 938 * 16 * 4 and 468 * 16 * 8 <= P.TILE_BYTES < 469 * 16 * 8
    nb = lambda name: -(-P.CASES[name].n // P.RPB)
    assert [nb("pick_nb%d" % b) for b in (256, 257, 513, 514)] == [256, 257, 513, 514]
    assert nb("longpre_nb7168") == P.LONGPRE_NB and nb("longpre_nb7169") == P.LONGPRE_NB + 1
    names = set(P.CASES)
    assert {"tile_F937", "tile_F938", "tile_F940", "tile_F468", "tile_F469", "L1_narrow", "L16_wave"} <= names
