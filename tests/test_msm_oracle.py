"""CPU tier of the MLE checkers (oracle/mle_oracle.py): the golden script's float64 stand-in ``mle_numpy`` -- the
solver that wrote msm_golden.npz and the device kernel's algorithmic twin -- against two solvers it shares nothing
with: the reference's own C estimator (Prinz's element-wise updates, oracle/_ref/libref_mle.so) and the long-double
fixed point; the closed form of T in pi; and the reference's return codes.

Measured here (x86-64, 80-bit long double), max relative difference of mle_numpy to mle_longdouble:

    input                    pi        T (pattern)   closed form T(pi) vs T
    ring_links(65, 3, 0)     2.9e-13   2.7e-13       1.7e-14
    hub(130, 0)              4.3e-13   3.3e-13       4.4e-14
    well_counts(60, 2)+0.5   4.9e-13   4.1e-13       8.7e-15
    well_counts(200, 1)      3.3e-10   1.3e-10       2.0e-14
    meta299 counts           2.1e-9    1.8e-10       1.2e-13
    wide_range(200, 0)       5.0e-6    2.6e-7        4.4e-8

The error of a solve stopped at a residual of 1e-14 (relative to the LARGEST population) is that residual over the
spectral gap, per state relative to its own population: 2e-9 on meta299's rarest states, 5e-6 on the rarest of a range
of ten decades -- where T, formed from the last iterate x while pi is g(x), also differs from its closed form in pi.
"""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_msm as G  # noqa: E402
from oracle import mle_oracle as O  # noqa: E402

needs_ref = pytest.mark.skipif(O.ref_mle(np.eye(2)) is None, reason="oracle/_ref/libref_mle.so has not been built")
needs_ld = pytest.mark.skipif(not O.have_extended_precision(), reason="numpy.longdouble is not an extended precision here")


def meta299_counts():
    y = G.cases()['meta299'][0][0]
    C = np.zeros((299, 299))
    np.add.at(C, (y[:-1], y[1:]), 1.0)
    return C


def rel_on_pattern(A, B):
    """max |A - B| / |B| over the nonzero entries of B, and the patterns must agree."""
    nz = B != 0
    assert np.array_equal(np.asarray(A) != 0, nz)
    return float((np.abs(A - B)[nz] / np.abs(B[nz])).max())


def loglik(C, T):
    nz = C > 0
    return float((C[nz] * np.log(T[nz])).sum())


@needs_ref
@pytest.mark.parametrize("name", ["ring65", "ring129", "ring1025", "well60_prior"])
def test_numpy_mle_against_the_reference_solver(name):
    """An independent algorithm reaches the same estimate: mle_numpy is within 4x of the distance between the reference
    at its default tolerance and at 1e-12 (its error decays geometrically: the distance to the limit is about the last
    increment / (1 - rate)), and its likelihood is no lower."""
    C = {"ring65": lambda: G.ring_links(65, 3, 65), "ring129": lambda: G.ring_links(129, 3, 129),
         "ring1025": lambda: G.ring_links(1025, 3, 1025), "well60_prior": lambda: G.well_counts(60, 2) + 0.5}[name]()
    n10, T10, pi10 = O.ref_mle(C, 1e-10)
    n12, T12, pi12 = O.ref_mle(C, 1e-12)
    assert 0 < n10 <= n12 < 10000
    T, pi, _ = G.mle_numpy(C)
    yard_T, yard_pi = rel_on_pattern(T10, T12), float((np.abs(pi10 - pi12) / pi12).max())
    dT, dpi = rel_on_pattern(T, T12), float((np.abs(pi - pi12) / pi12).max())
    print("%s: reference sweeps %d / %d, ref(1e-10) vs ref(1e-12) T %.2e pi %.2e; mle_numpy vs ref(1e-12) T %.2e pi %.2e"
          % (name, n10, n12, yard_T, yard_pi, dT, dpi))
    assert 0 < yard_T < 1e-5 and 0 < yard_pi < 1e-5
    assert dT <= 4 * yard_T and dpi <= 4 * yard_pi
    ll, ll_ref = loglik(C, T), loglik(C, T12)
    assert ll >= ll_ref - 1e-9 * abs(ll_ref)


@needs_ld
@pytest.mark.parametrize("name,bound_pi,bound_T", [
    # bounds: the stopping residual 1e-14 over the spectral gap of the plain iteration, read off the long-double solve's
    # own contraction (well-mixed: gap ~ 0.1; metastable: ~1e-5; ten decades of populations: the rarest state's
    # residual is relative to the largest population)
    ("ring65", 1e-12, 1e-12), ("hub130", 1e-12, 1e-12), ("well60_prior", 1e-12, 1e-12),
    ("well200", 1e-8, 1e-8), ("meta299", 1e-8, 1e-8), ("wide200", 1e-4, 1e-4), ("blocks", 1e-12, 1e-12)])
def test_numpy_mle_against_long_double(name, bound_pi, bound_T):
    C = {"ring65": lambda: G.ring_links(65, 3, 0), "hub130": lambda: G.hub(130, 0),
         "well60_prior": lambda: G.well_counts(60, 2) + 0.5, "well200": lambda: G.well_counts(200, 1),
         "meta299": meta299_counts, "wide200": lambda: G.wide_range(200, 0),
         "blocks": lambda: G.blocks((40, 30, 1), 0)}[name]()
    assert not np.array_equal(C, C.T)
    T, pi, it = G.mle_numpy(C)
    Tl, pil, itl = O.mle_longdouble(C)
    assert Tl.dtype == np.longdouble and O.kkt_longdouble(C, pil) < 1e-17
    if name == "blocks":   # reducible: T is unique, the blocks' weights are not -- compare inside the blocks
        dpi = max(float((np.abs(pi[s] / pi[s].sum() - pil[s] / pil[s].sum()) / (pil[s] / pil[s].sum())).max())
                  for s in (slice(0, 40), slice(40, 70), slice(70, 71)))
    else:
        dpi = float((np.abs(pi - pil) / pil).max())
    dT = rel_on_pattern(T, Tl)
    print("%s: mle_numpy %d its, long double %d its; pi %.2e, T %.2e; decades %.1f"
          % (name, it, itl, dpi, dT, np.log10(pi.max() / pi.min())))
    assert dpi <= bound_pi and dT <= bound_T
    if name == "wide200":
        assert pi.max() / pi.min() >= 1e9
    # the float64 residual evaluated in long double is the float64 one: the certificate is not a rounding artefact
    assert abs(O.kkt_longdouble(C, pi) - G.kkt_residual(C, pi)) <= 1e-15


@needs_ld
def test_closed_form():
    """T is a function of pi alone.  In long double at the converged pi the closed form is the solve's own X / rowsum
    to rounding, is stochastic and in detailed balance; in float64 it reproduces mle_numpy's T to 1e-12."""
    for C in (G.ring_links(65, 3, 0), G.hub(130, 0), G.ragged(300, 1), G.well_counts(60, 2) + 0.5, meta299_counts()):
        Tl, pil, _ = O.mle_longdouble(C)
        assert float(np.abs(Tl.sum(1) - 1).max()) < 1e-16
        flux = pil[:, None] * Tl
        assert float(np.abs(flux - flux.T).max()) < 1e-17 * float(flux.max())
        d = C.astype(np.longdouble).sum(1) / pil
        Cs = C.astype(np.longdouble) + C.T.astype(np.longdouble)
        X = Cs / (d[:, None] + d[None, :])
        assert rel_on_pattern(X / X.sum(1)[:, None], Tl) < 1e-16
        T, pi, _ = G.mle_numpy(C)
        Tc = O.t_from_pi(C, pi)
        assert Tc.dtype == np.float64 and np.array_equal(Tc != 0, (C + C.T) != 0)
        assert rel_on_pattern(T, Tc) <= 1e-12


def test_scaling_by_a_power_of_two_is_exact():
    """Every operation of the solve is homogeneous in C and powers of two are exact: T and pi are bit-identical."""
    for C in (G.ring_links(65, 3, 0), G.hub(130, 0)):
        T, pi, it = G.mle_numpy(C)
        for f in (2.0 ** 20, 2.0 ** -20):
            T2, pi2, it2 = G.mle_numpy(C * f)
            assert it2 == it and np.array_equal(T2, T) and np.array_equal(pi2, pi)


def test_generators():
    for C in (G.ring_links(2, 3, 2), G.ring_links(65, 3, 65), G.hub(65, 0), G.ragged(1025, 0), G.wide_range(200, 0),
              G.blocks((40, 30, 1), 0)):
        assert (C >= 0).all() and (C.sum(1) > 0).all() and not np.array_equal(C, C.T)
    Cs = G.hub(1025, 0)
    L = ((Cs + Cs.T) != 0).sum(1)
    assert L.max() == 1025 and np.median(L) < 12
    Cs = G.ragged(1025, 0)
    L = ((Cs + Cs.T) != 0).sum(1)
    widths = np.array([L[s:s + 64].max() for s in range(0, 1025, 64)])
    assert widths.max() >= 4 * widths.min() and L.min() <= 4 and L.max() >= 100
    # padding inside the slices: the rows of a slice are far from equally long
    assert np.mean([L[s:s + 64].min() / L[s:s + 64].max() for s in range(0, 1024, 64)]) < 0.3
    B = G.blocks((40, 30, 1), 0)
    assert not B[:40, 40:].any() and not B[40:, :40].any() and not B[70, :70].any() and B[70, 70] > 0


def test_numpy_mle_takes_the_singular_fallback_at_three_states():
    """With K = 3 the residuals live in a 2-dimensional space (they sum to zero), so the third difference makes the
    Gram matrix singular: mle_numpy's LinAlgError branch runs, and the solve still converges."""
    st = {}
    C = G.ring_links(3, 1, 0)
    T, pi, it = G.mle_numpy(C, stats=st)
    print(st)
    assert st['singular'] + st['nonpositive'] > 0 and st['accepted'] > 0
    assert G.kkt_residual(C, pi) <= 1e-13


@needs_ref
def test_reference_return_codes():
    """-1 on a zero row; -3 (its 10,000 sweeps used up) on the banded metastable matrix where the fixed point converges;
    -2 on NaN and on infinite entries."""
    assert O.ref_mle(np.array([[0.0, 0.0], [1.0, 1.0]]))[0] == -1
    C = G.well_counts(200, 1)
    assert O.ref_mle(C, 1e-10)[0] == -3
    T, pi, it = G.mle_numpy(C)
    assert it < 100000 and G.kkt_residual(C, pi) <= 1e-13
    for bad in (np.nan, np.inf):
        D = G.ring_links(5, 1, 0)
        D[1, 2] = bad
        assert O.ref_mle(D)[0] == -2
