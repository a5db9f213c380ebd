"""The device MLE (csrc/msm_mle.hip) and msm_syev_top at their seams, against solvers they share nothing with.

mle_solve_kernel is one workgroup of 1,024 threads; it changes behaviour at K = 64 s (sliced-ELL slices, partial last
slice), K = 1,024 (second trip of the strided loops), K = 6,144 (d leaves LDS) and K = 16,384 (refused above).  The
checkers are oracle/mle_oracle.py's long-double fixed point, the reference's own C solver (another algorithm), the closed
form T(pi), exact invariances, and numpy.linalg.eigh.  Inputs: tests/golden/make_golden_msm.py's seeded, asymmetric
generators (a symmetric C is already a fixed point: 0 iterations).

Tolerances.  Fixed: 1e-12 KKT, sparse/dense A/B and closed-form T; bit identity under powers of two.  Measured in the
test itself, never from the device's output: against the long-double solve the device may be 8x as far as the float64
stand-in on the same input (floor 1e-13; summation order and a residual that varies a few x under one stopping rule);
against the reference 4x the distance between the reference at 1e-10 and at 1e-12 (geometric decay); under a
relabelling 8x what the float64 stand-in moves under the same relabelling (floor 1e-12).

Measured on an MI355X (max relative difference; "stand-in" is the float64 yardstick computed on the CPU in the test):

    to the long-double solve       stand-in pi / T      device pi / T
    ragged K=65                    3.8e-14 / 2.9e-14    4.0e-14 / 3.1e-14
    ragged K=1025                  1.5e-12 / 1.3e-12    2.2e-13 / 1.9e-13
    blocks (40, 30, 1)             4.2e-13 / 4.7e-13    3.1e-13 / 3.7e-13
    meta299 counts (3.9 decades)   2.1e-9  / 1.8e-10    5.3e-10 / 4.8e-11
    wide_range(200) (9.9 decades)  5.0e-6  / 2.6e-7     5.5e-9  / 1.6e-10
    to the reference at 1e-12      ref(1e-10) T / pi    device T / pi
    ring K=65                      2.2e-9 / 1.8e-9      3.9e-11 / 3.2e-11
    ring K=129                     4.5e-9 / 4.7e-9      8.2e-11 / 8.5e-11
    ring K=1025                    2.7e-9 / 3.5e-9      5.3e-11 / 6.8e-11
    well_counts(60, 2) + 0.5       2.2e-8 / 2.2e-8      2.8e-8  / 2.8e-8
    under a relabelling            stand-in pi / T      device pi / T
    hub K=1025                     2.1e-13 / 9.9e-15    3.7e-13 / 2.3e-14
    ragged K=1025                  1.7e-14 / 2.2e-15    5.6e-15 / 7.2e-16
    hub K=6145                     7.6e-12 / 2.5e-13    1.2e-12 / 4.9e-14
    ragged K=6145                  3.8e-15 / 6.1e-16    8.1e-15 / 7.5e-16

(every case prints its own line with -s).  With the stopping rule of the first version -- max|g - x| / max g < 1e-14 alone,
which the stand-in still has -- the device was 1.3e-4 from the long-double populations on wide_range(200) (27x the stand-in)
and T was 4.5e-12 / 4.2e-12 off its closed form on hub K=6145 / star(100, 7): test_rare_states_against_long_double[wide200],
test_seam_sweep_sparse[hub-6145], test_relabelling_the_states[6145-hub] and test_fallback_branches failed.  The solve now
also asks every state's own relative step to be below 1e-13.  Wall time of the module: about 50 s.
"""
import sys
import time
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_msm as G  # noqa: E402
from oracle import mle_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

needs_ref = pytest.mark.skipif(O.ref_mle(np.eye(2)) is None, reason="oracle/_ref/libref_mle.so has not been built")
needs_ld = pytest.mark.skipif(not O.have_extended_precision(), reason="numpy.longdouble is not an extended precision here")

GEN = {"ring": lambda K: G.ring_links(K, 3, K), "hub": lambda K: G.hub(K, K), "ragged": lambda K: G.ragged(K, K)}
SWEEP_K = (2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049, 6143, 6144, 6145, 12289)
SWEEP = [("ring", K) for K in SWEEP_K] + [(g, K) for g in ("hub", "ragged") for K in (65, 1025, 6145)]


def mle(C, **kw):
    from msmbuilder_amd.msm.msm import _transmat_mle
    return _transmat_mle(C, **kw)


def last_stats():
    from msmbuilder_amd import _lib
    out = np.zeros(3, dtype=np.int64)
    _lib.check(_lib.lib().msm_mle_last_stats(out.ctypes.data_as(_lib._i64p)))
    return out


def meta299_counts():
    y = G.cases()['meta299'][0][0]
    C = np.zeros((299, 299))
    np.add.at(C, (y[:-1], y[1:]), 1.0)
    return C


def rel(a, b):
    return float((np.abs(a - b) / np.abs(b)).max())


def certify(C, T, pi, S, info):
    """The certificates of the seam sweep, entry by entry on the pattern of C + C^T (O(nnz) work beside a few K^2 passes)."""
    K = C.shape[0]
    assert info[1] == 1.0 and info[3] <= 1e-12
    P = O._Pattern(C, np.float64)
    assert np.abs(P.g(pi) - pi).max() / pi.max() <= 1e-12
    if K <= 2049:
        assert G.kkt_residual(C, pi) <= 1e-12
        if O.have_extended_precision():
            assert O.kkt_longdouble(C, pi) <= 1e-12
    r, c = P.rows, P.cols
    Tp = T[r, c]
    closed = P.vals / (P.c[r] + P.c[c] * (pi[r] / pi[c]))
    assert (Tp != 0).all() and np.count_nonzero(T) == len(r)       # exactly zero off the pattern, nonzero on it
    assert rel(Tp, closed) <= 1e-12
    if S is not None:
        assert np.count_nonzero(S) == len(r)
        # S = X / sqrt(r_i r_j) and T = X / r_i, pi = r / sum r: a handful of roundings apart
        assert rel(S[r, c], np.sqrt(pi[r] / pi[c]) * Tp) <= 1e-13
        assert np.array_equal(S, S.T)
    np.testing.assert_allclose(T.sum(1), 1.0, rtol=0, atol=1e-13)
    flux = pi[r] * Tp
    assert np.abs(flux - pi[c] * T[c, r]).max() <= 1e-13 * flux.max()
    assert abs(pi.sum() - 1.0) <= 1e-13 and (pi > 0).all()


@pytest.mark.parametrize("gen,K", SWEEP)
def test_seam_sweep_sparse(gpu, gen, K):
    C = GEN[gen](K)
    assert not np.array_equal(C, C.T)
    t0 = time.time()
    T, pi, S, info = mle(C)
    t1 = time.time()
    assert info[0] > 0
    certify(C, T, pi, S, info)
    line = "sweep %s K=%d: %d its, solve %.2f s, checks %.2f s" % (gen, K, info[0], t1 - t0, time.time() - t1)
    if K <= 1025 and O.have_extended_precision():
        Tl, pil, _ = O.mle_longdouble(C)
        Tn, pin, _ = G.mle_numpy(C)
        nz = Tl != 0
        yard_pi, yard_T = rel(pin, pil), rel(Tn[nz], Tl[nz])
        d_pi, d_T = rel(pi, pil), rel(T[nz], Tl[nz])
        line += "; to long double: stand-in pi %.1e T %.1e, device pi %.1e T %.1e" % (yard_pi, yard_T, d_pi, d_T)
        print(line)
        assert d_pi <= max(8 * yard_pi, 1e-13) and d_T <= max(8 * yard_T, 1e-13)
    else:
        print(line)


@pytest.mark.parametrize("K", [63, 64, 65, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("prior", [0.0, 0.5])
def test_seam_sweep_dense_against_sparse(gpu, monkeypatch, K, prior):
    """test_sparse_dense_ab's construction at the seams: the dense form (library prior, or MSM_MLE_DENSE=1) against the
    sparse form over the same numbers."""
    C = G.ring_links(K, 3, K)
    T1, pi1, S1, info1 = mle(C + prior)
    if prior == 0.0:
        monkeypatch.setenv("MSM_MLE_DENSE", "1")
    T2, pi2, S2, info2 = mle(C, prior=prior)
    assert info1[1] == info2[1] == 1.0
    np.testing.assert_allclose(T2, T1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(pi2, pi1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(S2, S1, rtol=1e-12, atol=0)
    assert np.array_equal(S1, S1.T) and np.array_equal(S2, S2.T)
    certify(C + prior, T2, pi2, S2, info2)


def test_dense_past_the_lds_copy(gpu, monkeypatch):
    """The dense form with d in global memory (K = 6,145) against the sparse form."""
    C = G.ring_links(6145, 3, 6145)
    T1, pi1, _, info1 = mle(C, want_s=False)
    monkeypatch.setenv("MSM_MLE_DENSE", "1")
    t0 = time.time()
    T2, pi2, _, info2 = mle(C, want_s=False)
    print("dense K=6145: %d its, %.2f s" % (info2[0], time.time() - t0))
    assert info1[1] == info2[1] == 1.0
    np.testing.assert_allclose(pi2, pi1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(T2, T1, rtol=1e-12, atol=0)
    certify(C, T2, pi2, None, info2)


@pytest.mark.parametrize("K", [65, 1025])
@pytest.mark.parametrize("dense", [False, True])
def test_scaling_by_powers_of_two_is_bit_exact(gpu, monkeypatch, K, dense):
    """Every operation of the solve is homogeneous in the counts and powers of two are exact."""
    C = G.hub(K, K)
    if dense:
        monkeypatch.setenv("MSM_MLE_DENSE", "1")
    T, pi, S, info = mle(C)
    for f in (2.0 ** 20, 2.0 ** -20):
        T2, pi2, S2, info2 = mle(C * f)
        assert info2[0] == info[0]
        assert np.array_equal(T2, T) and np.array_equal(pi2, pi) and np.array_equal(S2, S)


@pytest.mark.parametrize("gen", ["hub", "ragged"])
@pytest.mark.parametrize("K", [1025, 6145])
def test_relabelling_the_states(gpu, gen, K):
    """A random permutation of the states moves every row to another slice and lane; the result is the permuted one up
    to summation order.  Yardstick: the float64 stand-in (oracle.mle_fixed_point: mle_numpy's iteration over the
    pattern, affordable at K = 6,145) under the same permutation."""
    C = GEN[gen](K)
    p = np.random.RandomState(K).permutation(K)
    Cp = C[np.ix_(p, p)]
    Tn, pin, _ = O.mle_fixed_point(C)
    Tnp, pinp, _ = O.mle_fixed_point(Cp)
    yard_pi, yard_T = rel(pinp, pin[p]), float(np.abs(Tnp - Tn[np.ix_(p, p)]).max())
    del Tn, Tnp
    T, pi, S, info = mle(C)
    T2, pi2, S2, info2 = mle(Cp)
    d_pi, d_T, d_S = rel(pi2, pi[p]), float(np.abs(T2 - T[np.ix_(p, p)]).max()), float(np.abs(S2 - S[np.ix_(p, p)]).max())
    print("relabel %s K=%d: stand-in pi %.1e T %.1e; device pi %.1e T %.1e S %.1e" % (gen, K, yard_pi, yard_T, d_pi, d_T, d_S))
    assert d_pi <= max(8 * yard_pi, 1e-12)
    assert d_T <= max(8 * yard_T, 1e-12) and d_S <= max(8 * yard_T, 1e-12)
    certify(Cp, T2, pi2, S2, info2)


@needs_ref
@pytest.mark.parametrize("name", ["ring65", "ring129", "ring1025", "well60_prior"])
def test_against_the_reference_solver(gpu, name):
    prior = 0.5 if name == "well60_prior" else 0.0
    C = G.well_counts(60, 2) if prior else G.ring_links(int(name[4:]), 3, int(name[4:]))
    n10, T10, pi10 = O.ref_mle(C + prior, 1e-10)
    n12, T12, pi12 = O.ref_mle(C + prior, 1e-12)
    assert 0 < n10 <= n12
    T, pi, _, info = mle(C, prior=prior, want_s=False)
    nz = T12 != 0
    assert np.array_equal(T != 0, nz)
    yard_T, yard_pi = rel(T10[nz], T12[nz]), rel(pi10, pi12)
    d_T, d_pi = rel(T[nz], T12[nz]), rel(pi, pi12)
    print("reference %s: sweeps %d / %d; ref(1e-10) to ref(1e-12) T %.1e pi %.1e; device to ref(1e-12) T %.1e pi %.1e"
          % (name, n10, n12, yard_T, yard_pi, d_T, d_pi))
    assert yard_T > 0 and yard_pi > 0
    assert d_T <= 4 * yard_T and d_pi <= 4 * yard_pi
    Cp = C + prior
    ll = float((Cp[Cp > 0] * np.log(T[Cp > 0])).sum())
    ll_ref = float((Cp[Cp > 0] * np.log(T12[Cp > 0])).sum())
    assert ll >= ll_ref - 1e-9 * abs(ll_ref)


@needs_ld
def test_reducible_counts(gpu):
    """Block-diagonal counts, one block a single self-looping state: T is unique and block-diagonal, the blocks' relative
    weights in pi are not (they are whatever the start leaves them)."""
    sizes = (40, 30, 1)
    C = G.blocks(sizes, 0)
    T, pi, S, info = mle(C)
    certify(C, T, pi, S, info)
    Tl, pil, _ = O.mle_longdouble(C)
    Tn, pin, _ = G.mle_numpy(C)
    nz = Tl != 0
    assert np.array_equal(T != 0, nz) and T[70, 70] == 1.0
    yard_T, d_T = rel(Tn[nz], Tl[nz]), rel(T[nz], Tl[nz])
    o, yard_pi, d_pi = 0, 0.0, 0.0
    for n in sizes:
        s = slice(o, o + n)
        assert not T[s, :o].any() and not T[s, o + n:].any()
        w = pil[s] / pil[s].sum()
        yard_pi = max(yard_pi, rel(pin[s] / pin[s].sum(), w))
        d_pi = max(d_pi, rel(pi[s] / pi[s].sum(), w))
        o += n
    print("reducible: stand-in pi %.1e T %.1e, device pi %.1e T %.1e" % (yard_pi, yard_T, d_pi, d_T))
    assert d_T <= max(8 * yard_T, 1e-13) and d_pi <= max(8 * yard_pi, 1e-13)


def test_reducible_model_fits_with_a_warning(gpu):
    from msmbuilder_amd import MarkovStateModel
    rs = np.random.RandomState(11)
    seqs = [G.metastable_labels(rs, 3000, 4, 0.9), G.metastable_labels(rs, 2000, 3, 0.9) + 10, np.full(50, 99)]
    with pytest.warns(UserWarning, match="not generally compatible"):
        m = MarkovStateModel(ergodic_cutoff='off', verbose=False).fit(seqs)
    assert m.n_states_ == 8 and m.mle_info_[1] == 1.0
    T = m.transmat_
    assert not T[:4, 4:].any() and not T[4:, :4].any() and not T[7, :7].any() and T[7, 7] == 1.0
    np.testing.assert_allclose(T.sum(1), 1.0, rtol=0, atol=1e-13)
    assert G.kkt_residual(m.countsmat_, m.populations_) <= 1e-12


@needs_ld
@pytest.mark.parametrize("name", ["wide200", "meta299"])
def test_rare_states_against_long_double(gpu, name):
    """Per-state relative error, the smallest populations included.  meta299: the measurement behind
    test_golden_parity's rtol of 1e-8 on the populations."""
    C = G.wide_range(200, 0) if name == "wide200" else meta299_counts()
    T, pi, S, info = mle(C)
    assert info[1] == 1.0 and info[3] <= 1e-12 and G.kkt_residual(C, pi) <= 1e-12
    Tl, pil, _ = O.mle_longdouble(C)
    Tn, pin, _ = G.mle_numpy(C)
    nz = Tl != 0
    assert np.array_equal(T != 0, nz)
    yard_pi, yard_T, d_pi, d_T = rel(pin, pil), rel(Tn[nz], Tl[nz]), rel(pi, pil), rel(T[nz], Tl[nz])
    print("rare %s: %.1f decades; stand-in pi %.1e T %.1e (%d its), device pi %.1e T %.1e (%d its)"
          % (name, np.log10(float(pil.max() / pil.min())), yard_pi, yard_T, _, d_pi, d_T, info[0]))
    assert d_pi <= max(8 * yard_pi, 1e-13) and d_T <= max(8 * yard_T, 1e-13)
    if name == "wide200":
        assert pil.max() / pil.min() >= 1e9


def test_fallback_branches(gpu):
    """The plain-step fallbacks of the mixing, counted by msm_mle_last_stats.

    Non-positive mixed step (tot[1] != 0): reached.  make_golden_msm.star -- a start far from the solution -- makes
    mle_numpy reject 1 - 2 mixed steps per solve, and the device rejects as many (MI355X: 1, 1, 2, 2 on the four inputs).
    Singular or non-finite solve (small_solve returning false): NOT reached by any input found.  mle_numpy takes its
    LinAlgError branch at K = 2 and K = 3 (the residuals span K - 1 dimensions, so a deeper history is rank-deficient and
    LAPACK meets an exactly zero pivot), but on the same eight inputs the device's elimination of the same Gram matrix
    never lands on an exact zero and accepts every mixed step (measured: singular = 0 on all).  The count is printed and
    the certificates are asserted either way; only the non-positive branch is asserted to have run."""
    sing = nonpos = mixed = 0
    for C in [G.ring_links(2, 1, s) for s in (1, 3, 4)] + [G.ring_links(3, 1, s) for s in range(5)]:
        T, pi, S, info = mle(C)
        st = last_stats()
        print("K=%d: %d its, accepted %d, non-positive %d, singular %d" % (C.shape[0], info[0], st[0], st[1], st[2]))
        assert st.sum() == max(info[0] - 1, 0)      # every iteration after the first either mixes or falls back
        certify(C, T, pi, S, info)
        sing += st[2]
        mixed += st[0]
    for K, seed in ((20, 1), (20, 4), (100, 3), (100, 7)):
        C = G.star(K, seed)
        T, pi, S, info = mle(C)
        st = last_stats()
        print("star(%d, %d): %d its, accepted %d, non-positive %d, singular %d" % (K, seed, info[0], st[0], st[1], st[2]))
        assert st.sum() == max(info[0] - 1, 0)
        certify(C, T, pi, S, info)
        nonpos += st[1]
        mixed += st[0]
    print("fallbacks over all inputs: accepted %d, non-positive %d, singular %d" % (mixed, nonpos, sing))
    assert mixed > 0
    assert nonpos > 0


def test_failure_and_recovery(gpu):
    small = G.ring_links(130, 3, 7)
    before = mle(small)
    C = G.well_counts(1000, 7)
    with pytest.raises(ValueError, match=r"^Likelihood not converged\. Error code=-3$"):
        mle(C, max_iter=5)
    after = mle(small)          # smaller than the failed call: stale contents of the pooled buffers would show
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match=r"^Likelihood not converged\. Error code=-3$"):
        mle(small, max_iter=0)
    sym = small + small.T
    T, pi, S, info = mle(sym, max_iter=0)
    assert info[0] == 0 and info[1] == 1.0
    certify(sym, T, pi, S, info)
    for a, b in zip(before, mle(small)):
        assert np.array_equal(a, b)


def test_too_many_states_is_refused_before_any_work(gpu):
    C = np.zeros((16385, 16385))     # untouched pages: nothing is read before the refusal
    t0 = time.time()
    with pytest.raises(ValueError, match=r"^msm_transmat_mle: need 1 <= n <= 16384$"):
        mle(C)
    assert time.time() - t0 < 1.0


def test_nonfinite_counts_are_a_domain_error(gpu):
    """The reference's solver returns -2 on NaN and on infinite counts (tests/test_msm_oracle.py pins that) and its wrapper
    has no words of its own for it: here they carry the wording of that code."""
    for bad in (np.nan, np.inf):
        for prior in (0.0, 0.5):
            C = G.ring_links(5, 1, 0)
            C[1, 2] = bad
            with pytest.raises(ValueError, match=r"^Domain error\. C must be positive\. Error code=-2$"):
                mle(C, prior=prior)
    T, pi, S, info = mle(G.ring_links(5, 1, 0))
    assert info[1] == 1.0


# ---- msm_syev_top -----------------------------------------------------------------------------------------------------
def _sym_matrix(kind, n):
    rs = np.random.RandomState(n + 17)
    if kind == "random":
        A = rs.randn(n, n)
        return (A + A.T) / 2, None
    Q = np.linalg.qr(rs.randn(n, n))[0]
    w = np.sort(rs.rand(n))[::-1] * 2 - 0.5
    if kind == "repeated" and n >= 5:        # a pair at the top and a triple right below it
        w[0] = w[1] = 1.75
        w[2] = w[3] = w[4] = 1.5
    if kind == "repeated" and n == 2:
        w[:] = 1.75
    if kind == "negative":                   # the largest magnitudes are negative
        w = -3.0 * rs.rand(n) - 0.5
        w[:max(n // 3, 1)] = rs.rand(max(n // 3, 1))
    S = (Q * w) @ Q.T
    return (S + S.T) / 2, np.sort(w)[::-1]


def _check_top(S, k, w_known=None):
    from msmbuilder_amd.msm.msm import _symmetric_top
    n = S.shape[0]
    vals, V = _symmetric_top(S, k)
    w, U = np.linalg.eigh(S)
    w, U = w[::-1], U[:, ::-1]
    rho, nrm = np.abs(w).max(), np.linalg.norm(S, 2)
    assert vals.shape == (k,) and V.shape == (n, k)
    assert np.all(np.diff(vals) <= 0)
    assert np.abs(vals - w[:k]).max() <= 1e-12 * rho
    if w_known is not None:
        assert np.abs(vals - w_known[:k]).max() <= 1e-12 * rho * 10    # the construction itself rounds Q diag(w) Q^T
    assert np.abs(V.T @ V - np.eye(k)).max() <= 1e-12
    assert np.linalg.norm(S @ V - V * vals, axis=0).max() <= 1e-12 * nrm
    # span agreement inside groups of (nearly) repeated eigenvalues: the projectors of the groups agree
    lo = 0
    while lo < k:
        hi = lo + 1
        while hi < n and abs(w[hi] - w[hi - 1]) <= 1e-9 * rho:
            hi += 1
        if hi <= k:
            Pm = V[:, lo:hi].T @ U[:, lo:hi]
            assert np.abs(Pm @ Pm.T - np.eye(hi - lo)).max() <= 1e-6
        lo = hi


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 300, 1024, 2049])
@pytest.mark.parametrize("kind", ["random", "repeated", "negative"])
def test_syev_top_against_eigh(gpu, n, kind):
    S, w_known = _sym_matrix(kind, n)
    for k in sorted({1, min(2, n), max(n // 2, 1), n}):
        if n == 2049 and k > 64:
            k = 64          # k n stays small at the largest n
        _check_top(S, k, w_known)


@pytest.mark.parametrize("gen,K", [("ring", 65), ("hub", 1025), ("ragged", 1025)])
def test_syev_top_on_mle_outputs(gpu, gen, K):
    C = GEN[gen](K)
    T, pi, S, info = mle(C)
    _check_top(S, 11)
    _check_top(S, K if K <= 65 else 64)
    from msmbuilder_amd.msm.msm import _symmetric_top
    vals, _ = _symmetric_top(S, 3)
    assert abs(vals[0] - 1.0) <= 1e-12
    w = np.sort(np.real(np.linalg.eigvals(T)))[::-1]
    assert np.abs(vals - w[:3]).max() <= 1e-10      # T's own (non-symmetric) eigenvalues


def test_transpose_with_a_state_without_counts(gpu):
    """'transpose' under ergodic_cutoff='off' with a state that has no counts: the fit stands (a NaN row, population 0)
    and the eigensystem is refused with the reference's (scipy's) message -- the golden case 'transpose_zero'."""
    from msmbuilder_amd import MarkovStateModel
    seqs, params, _ = G.cases()['transpose_zero']
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MarkovStateModel(verbose=False, **params).fit(seqs)
    assert np.isnan(m.transmat_[5]).all() and np.isfinite(m.transmat_[:5]).all() and m.populations_[5] == 0.0
    with pytest.raises(ValueError, match=r"^array must not contain infs or NaNs$"):
        m.eigenvalues_
    with pytest.raises(ValueError, match=r"^array must not contain infs or NaNs$"):
        m.timescales_
