"""GPU tier of the packed sum/difference kernel (csrc/tica_sym_units.h, tica_sym_f32_kernel<.., PACK>): the widths whose
handle packs diagonal blocks -- 512 (one group of four diagonal tiles), 640 (a group and a plain diagonal tile), 768 (a group
and two), 1024 (two groups) -- through the C ABI, on about 200 ragged trajectories of lag + 1 to 700 frames: several chunks
per cohort, edge half-steps in most of them, columns with different non-zero means.

Every case first asserts that msm_tica_last_plan reports the path `sym`, T (T+1)/2 - T//4 workgroups per cohort and as many
cohorts as two resident workgroups per compute unit hold: the packed kernel is what ran, on every slot.

* exact: rows of small integers, no mean shift -- every fp32 product and partial sum is an integer below 2^24 (|u|, |d| <= 6,
  so a partial of at most 8,192 + 700 frames stays below 36 * 8,892 < 2^19), the fp64 merges and the halvings are exact, so
  C (symmetrised), G and both column sums EQUAL the integer oracle bit for bit, folded column sums or not, and the unpacked
  kernel (MSM_TICA_SYM_PACK=0) gives the identical arrays.  The oracle is formed in float64 on the device: sums of integers
  this small (|C|, |G| <= 18 * 70,000) are exact there in any order.
  MSM_TICA_FOLD=2 and =0 run on the same rows, all of them; the plan does not fold trajectories between lag and 2 lag
  frames, so a third leg repeats MSM_TICA_FOLD=2 on the trajectories of at least 2 lag frames, where it does fold.
* default: float rows, shift on, against the float64 oracle at the tolerances tests/test_gpu_tica_plan.py states for mode f32.
* long run: 480,001 frames of 512 features (more than two chunks of 4,096 per cohort: the fp32 partials are merged mid-run)
  against a mode-f64 handle on the same device rows.
* control: 384 features (three tiles per side: no group) stays unpacked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_plan_ref as R  # noqa: E402
from test_gpu_tica import ATOL_SCALE, RTOL  # noqa: E402
from test_gpu_tica_plan import SWITCHES, Handle  # noqa: E402

pytestmark = pytest.mark.gpu

LAG = 10
WIDTHS = (512, 640, 768, 1024)
N_SEQ = 200
K_EIG = 5


def lengths():
    """200 lengths in lag + 1 .. 700, both sides of 2 lag among them, and one of lag frames (skipped)."""
    rs = np.random.RandomState(11)
    fixed = [LAG + 1, LAG + 2, 2 * LAG - 1, 2 * LAG, 2 * LAG + 1, LAG, 700, 33, 64, 65]
    return fixed + list(rs.randint(LAG + 1, 701, size=N_SEQ - len(fixed)))


@pytest.fixture
def switches(gpu, monkeypatch):
    for name in SWITCHES + ("MSM_TICA_SYM_PACK",):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


_ROWS = {}


def rows(F, kind):
    """The trajectories of a width as views of one device tensor (float32, 16-byte aligned rows), made once."""
    import torch
    if (F, kind) not in _ROWS:
        lens = lengths()
        g = torch.Generator(device="cuda").manual_seed(1000 + F)
        n = int(sum(lens))
        if kind == "int":
            X = torch.randint(-3, 4, (n, F), generator=g, device="cuda").float()
        else:
            # six slow latent coordinates mixed into F columns, noise, a different mean per column
            t = torch.arange(n, device="cuda", dtype=torch.float32)[:, None]
            period = torch.tensor([40.0, 65.0, 90.0, 130.0, 170.0, 230.0], device="cuda")
            Z = torch.sin(2 * np.pi * t / period + torch.rand(6, generator=g, device="cuda"))
            X = Z @ torch.randn(6, F, generator=g, device="cuda") + 0.5 * torch.randn(n, F, generator=g, device="cuda")
            X = X + torch.linspace(-3.0, 3.0, F, device="cuda") + 0.25
        torch.cuda.synchronize()
        _ROWS[(F, kind)] = list(torch.split(X, [int(k) for k in lens]))
    return _ROWS[(F, kind)]


_ORACLES = {}


def oracle(F, kind, seqs, tag):
    """(C, G, s0, stau, n_observations, n_sequences) in float64, formed on the device from the rows the handle reads."""
    import torch
    if (F, kind, tag) not in _ORACLES:
        valid = [s for s in seqs if s.shape[0] > LAG]
        A = torch.cat([s[:-LAG] for s in valid]).double()
        B = torch.cat([s[LAG:] for s in valid]).double()
        out = (A.T @ B, A.T @ A + B.T @ B, A.sum(0), B.sum(0))
        _ORACLES[(F, kind, tag)] = tuple(o.cpu().numpy() for o in out) + (sum(s.shape[0] for s in valid), len(valid))
    return _ORACLES[(F, kind, tag)]


def geometry_and_plan(h):
    geom, plan, nchunks, nsuper = R.last_plan(h.h)
    return geom, dict(zip(R.PLAN_FIELDS, plan)), geom, plan, nchunks


def check_launch(h, F, packed, fold):
    """The plan of the handle's last launch: the sum/difference path, the expected workgroups per cohort on every resident
    slot, and the library's own plan of the handle's geometry."""
    import torch
    g, p, geom, plan, nchunks = geometry_and_plan(h)
    T = F // 128
    want_units = T * (T + 1) // 2 - (T // 4 if packed else 0)
    assert R.PATHS[p["path"]] == "sym" and p["flavour"] == (R.FL_FOLD if fold else 0), (p, g)
    assert g["ntiles_sym"] == want_units, g
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count      # two 64-KiB workgroups per compute unit
    assert g["sym_cohorts"] == slots // want_units and g["sym_grid"] == g["sym_cohorts"] * want_units == p["G"], (g, p)
    assert g["S_sym"] == g["sym_cohorts"] == p["S"]
    assert p["fold"] == int(fold)
    assert nchunks > 2 * p["S"], (nchunks, p)        # several chunks per cohort
    env = os.environ.get("MSM_TICA_FOLD")
    assert R.library_plan(geom, h.launch["dtype_bytes"], h.launch["ld"], h.launch["n_rows"], ptr16=h.launch["ptr16"],
                          ptr16_all=h.launch["ptr16_all"], fold_env=None if env is None else int(env)) == plan


def fit(F, seqs, packed, fold, mode="f32"):
    """Fresh handle, one launch; the exported state [C | G | s0 | stau | n_observations | n_sequences]."""
    h = Handle(F, mode, lag=LAG)
    try:
        h.accumulate(seqs)
        if mode == "f32":
            check_launch(h, F, packed, fold)
            assert h.flag("msm_tica_lagged_symmetrised") == 1
        return h.packed()
    finally:
        h.close()


def split(packed, F):
    return (packed[:F * F].reshape(F, F), packed[F * F:2 * F * F].reshape(F, F), packed[2 * F * F:2 * F * F + F],
            packed[2 * F * F + F:2 * F * F + 2 * F], list(packed[-2:]))


def eigenvalues(C, G, s0, st, n_pairs):
    """Top generalized eigenvalues of (offset correlation, covariance) of the moments (tica.py:234-245, no shrinkage)."""
    import scipy.linalg
    F = len(s0)
    mu = (s0 + st) / (2.0 * n_pairs)
    oc = (C + C.T) / (2.0 * n_pairs) - np.outer(mu, mu)
    cov = G / (2.0 * n_pairs) - np.outer(mu, mu)
    return scipy.linalg.eigh(oc, cov, eigvals_only=True, subset_by_index=[F - K_EIG, F - 1])[::-1]


def check_default(F, packed_state, ora):
    C, G, s0, st, nobs, nseq = ora
    gotC, gotG, got0, gott, counts = split(packed_state, F)
    Cs = 0.5 * (C + C.T)
    tol = dict(rtol=0, atol=ATOL_SCALE["f32"] * np.abs(G).max())
    np.testing.assert_allclose(0.5 * (gotC + gotC.T), Cs, **tol)
    np.testing.assert_allclose(gotG, G, **tol)
    np.testing.assert_allclose(got0, s0, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(gott, st, rtol=1e-12, atol=1e-9)
    assert counts == [nobs, nseq]
    n_pairs = nobs - LAG * nseq
    np.testing.assert_allclose(eigenvalues(gotC, gotG, got0, gott, n_pairs), eigenvalues(Cs, G, s0, st, n_pairs), rtol=RTOL["f32"])


LEGS = {"fold2": ("2", False), "fold0": ("0", False), "fold2-foldable": ("2", True)}


@pytest.mark.parametrize("leg", sorted(LEGS))
@pytest.mark.parametrize("F", WIDTHS)
def test_integer_rows_equal_the_integer_oracle_bit_for_bit(switches, F, leg):
    """fold2 / fold0: MSM_TICA_FOLD=2 and =0 on the SAME rows, all of them (trajectories between lag and 2 lag frames among
    them: the plan then declines to fold, and both take the plain packed kernel).  fold2-foldable: MSM_TICA_FOLD=2 on the
    trajectories of at least 2 lag frames, which the plan folds: the packed kernel with the folded column sums."""
    env, foldable = LEGS[leg]
    switches.setenv("MSM_TICA_SHIFT", "0")
    switches.setenv("MSM_TICA_FOLD", env)
    seqs = rows(F, "int")
    assert any(LAG < s.shape[0] < 2 * LAG for s in seqs)
    if foldable:
        seqs = [s for s in seqs if s.shape[0] >= 2 * LAG or s.shape[0] <= LAG]
    C, G, s0, st, nobs, nseq = oracle(F, "int", seqs, "foldable" if foldable else "all")
    for a in (C, G, s0, st):
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() < 2 ** 24      # integers, exact in every format on the way
    state = fit(F, seqs, packed=True, fold=foldable)
    gotC, gotG, got0, gott, counts = split(state, F)
    assert np.array_equal(gotC, 0.5 * (C + C.T))         # (halves of integers: exact)
    assert np.array_equal(gotG, G)
    assert np.array_equal(got0, s0) and np.array_equal(gott, st)
    assert counts == [nobs, nseq]
    switches.setenv("MSM_TICA_SYM_PACK", "0")            # read at create: the same rows through the unpacked kernel
    assert np.array_equal(fit(F, seqs, packed=False, fold=foldable), state)


@pytest.mark.parametrize("F", WIDTHS)
def test_float_rows_meet_the_float64_oracle(switches, F):
    seqs = rows(F, "float")
    check_default(F, fit(F, seqs, packed=True, fold=False), oracle(F, "float", seqs, "all"))


def test_three_tiles_per_side_stay_unpacked(switches):
    F = 384
    seqs = rows(F, "float")
    state = fit(F, seqs, packed=False, fold=False)
    check_default(F, state, oracle(F, "float", seqs, "all"))


def test_long_run_merges_partials_mid_run_and_meets_the_f64_handle(switches):
    import torch
    F, lens = 512, (200000, 160000, 120001)
    g = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randn(sum(lens), F, generator=g, device="cuda") + torch.linspace(-3.0, 3.0, F, device="cuda") + 0.25
    seqs = list(torch.split(X, list(lens)))
    torch.cuda.synchronize()
    h = Handle(F, "f32", lag=LAG)
    try:
        h.accumulate(seqs)
        check_launch(h, F, packed=True, fold=True)           # 2^26 elements and more: folded by default
        gp, p, geom, plan, nchunks = geometry_and_plan(h)
        # a cohort's share is more frames than one fp32 partial holds (8,192 under the shift), in chunks of at most 4,096
        assert p["total"] > p["S"] * p["kflush"] and p["kflush"] == 8192 and p["kc"] <= 4096 and nchunks > 2 * p["S"]
        got = h.packed()
    finally:
        h.close()
    want = fit(F, seqs, packed=False, fold=False, mode="f64")
    gotC, gotG, got0, gott, counts = split(got, F)
    C, G, s0, st, wcounts = split(want, F)
    tol = dict(rtol=0, atol=ATOL_SCALE["f32"] * np.abs(G).max())
    np.testing.assert_allclose(0.5 * (gotC + gotC.T), 0.5 * (C + C.T), **tol)
    np.testing.assert_allclose(gotG, G, **tol)
    np.testing.assert_allclose(got0, s0, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(gott, st, rtol=1e-12, atol=1e-9)
    assert counts == wcounts == [sum(lens), len(lens)]
