"""Designed moments for the tICA solve: generalized eigenproblems whose answer is known by construction.

``tICA.from_reference_state`` puts arbitrary accumulators on the device.  With ``lag_time = 1``, ``n_sequences_ = 1``,
``n_observations_ = 2**20 + 1`` (2**20 lagged pairs) and ``shrinkage = 0.0`` the finalisation of the moments
(decomposition/_moments.py, csrc/tica_solve_dev.h) is a division by 2**21, exact in floating point:

    OC = (C + C^T) / 2**21 - mu mu^T,     S = G / 2**21 - mu mu^T,     mu = (s0 + stau) / 2**21

so a test chooses OC and S freely.  ``design`` builds them backwards from the answer:

    W, Q orthogonal (QR of Gaussian matrices);  s log-spaced in [1 / kappa, 1], the spectrum of the covariance
    R = the upper-triangular QR factor of diag(sqrt s) Q^T, diagonal made positive;  S = R^T R
    Cr = W diag(lam) W^T                 the reduced matrix U^-T OC U^-1: the Cholesky factor U of S is unique, so U = R
    OC = R^T Cr R
    V = R^-1 W                           the S-orthonormal eigenvectors: OC v_j = lam_j S v_j,  V^T S V = I

Everything is float64 numpy; the products that build OC and S round, so the designed values are the answer of the
stored pencil only to ~ kappa * eps -- ``host_yardstick`` measures what float64 LAPACK makes of the same stored
matrices, and the GPU tests allow the device a small multiple of that.
"""
import functools

import numpy as np
import scipy.linalg

N_PAIRS = 2 ** 20                 # lagged pairs: n_observations_ - lag_time * n_sequences_
N_OBSERVATIONS = N_PAIRS + 1

# per-vector comparison needs both neighbouring gaps above this (tests/test_gpu_toppairs.py)
GAP_MIN = 1e-4

SPECTRA = ("gap", "double", "edge_tie", "negative", "neg_outlier", "near_one", "wide_cluster", "outside")


def _gap(n, k):
    bulk = np.linspace(0.08, -0.08, n - k) if n > k else np.zeros(0)
    top = np.linspace(0.95, 0.5, k) if k > 1 else np.array([0.95])
    return np.concatenate([top, bulk])


def spectrum(name, n, k):
    """(lam, k, exempt): the n designed eigenvalues in DESCENDING order (lam[:k] are the wanted ones), the number of
    components the spectrum is meant for (``wide_cluster`` fixes it to 16), and the number of the top k vectors that are
    not determined individually -- a property of the construction, asserted by the tests:

    gap           k values in [0.5, 0.95], then a bulk in [-0.08, 0.08]
    double        exact pairs among the top k (k even): every vector is exempt
    edge_tie      lam[k - 1] == lam[k] exactly: the k-th vector is any unit vector of a plane
    negative      everything below 0: the top k in [-0.3, -0.05], the rest in [-0.9, -0.6]
    neg_outlier   gap, with the smallest eigenvalue at -0.97
    near_one      gap, with lam[0] = 1 - 1e-9
    wide_cluster  40 values evenly spaced in [0.90, 0.91], k = 16: more wanted-looking directions than the 32-vector block
                  holds; the spacing 0.01 / 39 is above GAP_MIN, so no vector is exempt
    outside       gap, with lam[0] = 1.7 and lam[-1] = -1.5: moments no data could produce
    """
    if name == "wide_cluster":
        k = 16
        if n < 48:
            raise ValueError("wide_cluster needs n >= 48")
        return np.concatenate([np.linspace(0.91, 0.90, 40), np.linspace(0.08, -0.08, n - 40)]), k, 0
    if not 1 <= k <= n or (k == n and name != "gap"):
        raise ValueError("need 1 <= k < n (gap: k <= n)")
    lam = _gap(n, k)
    exempt = 0
    if name == "gap":
        pass
    elif name == "double":
        if k % 2:
            raise ValueError("double needs an even k")
        lam[:k] = np.repeat(np.linspace(0.95, 0.5, k // 2), 2)
        exempt = k
    elif name == "edge_tie":
        lam[k] = lam[k - 1]
        exempt = 1
    elif name == "negative":
        lam = np.concatenate([np.linspace(-0.05, -0.3, k) if k > 1 else np.array([-0.05]), np.linspace(-0.6, -0.9, n - k)])
    elif name == "neg_outlier":
        lam[-1] = -0.97
    elif name == "near_one":
        lam[0] = 1.0 - 1e-9
    elif name == "outside":
        lam[0] = 1.7
        lam[-1] = -1.5
    else:
        raise ValueError("unknown spectrum %r" % (name,))
    return lam, k, exempt


def spectra(n, k):
    """{name: (lam, k, exempt)} of every named spectrum at n features (``double`` only for even k)."""
    return {name: spectrum(name, n, k) for name in SPECTRA if not (name == "double" and k % 2)}


def exempt_count(lam, k):
    """Number of the top k designed vectors with a neighbouring gap (the one to lam[k] included) of at most GAP_MIN."""
    return int(sum(neighbour_gap(lam, j) <= GAP_MIN for j in range(k)))


def neighbour_gap(lam, j):
    """min(lam[j - 1] - lam[j], lam[j] - lam[j + 1]) of the descending spectrum."""
    lo = lam[j - 1] - lam[j] if j > 0 else np.inf
    hi = lam[j] - lam[j + 1] if j + 1 < len(lam) else np.inf
    return min(lo, hi)


def _orthogonal(rs, n):
    q, r = np.linalg.qr(rs.standard_normal((n, n)))
    return q * np.sign(np.diag(r))          # Haar distributed


def design(n, lam, kappa=1e2, seed=0, mean=None, k=None, n_components=None):
    """The designed problem: a dict with

    state        the mapping ``tICA.from_reference_state`` takes (both Gram halves 2**20 (S + mean mean^T))
    OC, S        the pencil, symmetric bit for bit
    OCf, Sf      what the host formulas of ``_moments`` make of ``state`` (identical to OC, S for a zero mean)
    R, Cr, V, W  the Cholesky factor of S, the reduced matrix, the S-orthonormal eigenvectors and those of Cr, columns in
                 the order of ``lam``
    lam, order   the eigenvalues as given and their indices by descending value; ``top`` = order[:k]
    mean         the designed mean (zeros by default)
    """
    lam = np.asarray(lam, dtype=np.float64)
    if lam.shape != (n,):
        raise ValueError("need %d eigenvalues" % n)
    rs = np.random.RandomState(seed)
    W = _orthogonal(rs, n)
    Q = _orthogonal(rs, n)
    s = np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    R = np.linalg.qr(np.sqrt(s)[:, None] * Q.T, mode="r")
    R = np.triu(R * np.sign(np.diag(R))[:, None])
    S = R.T.dot(R)
    S = 0.5 * (S + S.T)
    Cr = (W * lam).dot(W.T)
    Cr = 0.5 * (Cr + Cr.T)
    OC = R.T.dot(Cr).dot(R)
    OC = 0.5 * (OC + OC.T)
    V = scipy.linalg.solve_triangular(R, W, lower=False)
    mu = np.zeros(n) if mean is None else np.array(np.broadcast_to(mean, (n,)), dtype=np.float64)
    mm = np.outer(mu, mu)
    order = np.argsort(-lam, kind="stable")
    kk = n if k is None else int(k)
    half = N_PAIRS * (S + mm)
    state = dict(n_components=(kk if n_components is None else n_components), lag_time=1, shrinkage=0.0, kinetic_mapping=False,
                 commute_mapping=False, n_features=n, n_observations_=N_OBSERVATIONS, n_sequences_=1,
                 _outer_0_to_T_lagged=N_PAIRS * (OC + mm), _sum_0_to_TminusTau=N_PAIRS * mu, _sum_tau_to_T=N_PAIRS * mu,
                 _outer_0_to_TminusTau=half, _outer_offset_to_T=half.copy())
    OCf, Sf = finalise(state)
    out = dict(state=state, OC=OC, S=S, OCf=OCf, Sf=Sf, R=R, Cr=Cr, V=V, W=W, lam=lam, order=order, top=order[:kk], mean=mu,
               n=n, kappa=float(kappa))
    for v in list(out.values()) + list(state.values()):
        if isinstance(v, np.ndarray):
            v.flags.writeable = False          # shared between tests
    return out


def finalise(state):
    """(OC, S) of a state by the formulas of decomposition/_moments.py (shrinkage 0)."""
    n_pairs = state["n_observations_"] - state["lag_time"] * state["n_sequences_"]
    mu = (state["_sum_0_to_TminusTau"] + state["_sum_tau_to_T"]) / float(2 * n_pairs)
    c = state["_outer_0_to_T_lagged"]
    g = state["_outer_0_to_TminusTau"] + state["_outer_offset_to_T"]
    return (c + c.T) / (2 * n_pairs) - np.outer(mu, mu), g / (2 * n_pairs) - np.outer(mu, mu)


def not_positive_definite(d, p):
    """The state of ``d`` with S[p, p] made negative: the leading minor of order p + 1 is the first that is not positive
    definite (the leading p x p block is a principal submatrix of S)."""
    state = dict(d["state"])
    half = np.array(state["_outer_0_to_TminusTau"])
    half[p, p] = -abs(half[p, p])
    state["_outer_0_to_TminusTau"] = half
    state["_outer_offset_to_T"] = half.copy()
    return state


def host_reduce(OC, S):
    """(U, Cs): S = U^T U and Cs = U^-T OC U^-1 by LAPACK -- dpotrf and two triangular solves, dsygst's arithmetic."""
    U = scipy.linalg.cholesky(S, lower=False)
    X = scipy.linalg.solve_triangular(U, OC, trans="T", lower=False)           # U^-T OC
    Cs = scipy.linalg.solve_triangular(U, X.T, trans="T", lower=False).T       # (U^-T (U^-T OC)^T)^T = U^-T OC U^-1
    return U, Cs


def host_yardstick(d, k=None, back_rows=None):
    """Float64 LAPACK's own error against the designed truth, on the matrices the finalisation hands the solver:

    eig    max |lambda_host - lambda_designed| over the top k (``eigh`` with ``b=``: dsygvd's route)
    Cr     max |Cs_host - Cr|   (``cholesky`` + two ``solve_triangular``)
    back   max |U_host^-1 y - v| over the designed pairs ``back_rows`` (indices into lam; default: the top k)
    vals, vecs, Cs, U   what the host computed
    """
    n = d["n"]
    k = len(d["top"]) if k is None else k
    top = d["order"][:k]
    vals, vecs = scipy.linalg.eigh(d["OCf"], b=d["Sf"], subset_by_index=[n - k, n - 1])
    vals, vecs = vals[::-1], vecs[:, ::-1]
    U, Cs = host_reduce(d["OCf"], d["Sf"])
    return dict(eig=float(np.abs(vals - d["lam"][top]).max()), Cr=float(np.abs(Cs - d["Cr"]).max()),
                back=back_error(d, U, top if back_rows is None else back_rows), vals=vals, vecs=vecs, Cs=Cs, U=U)


def back_error(d, U, rows):
    """max |U^-1 y - v| over the designed pairs ``rows``: one triangular solve against the host's own factor."""
    rows = np.asarray(rows)
    Vh = scipy.linalg.solve_triangular(U, d["W"][:, rows], lower=False)
    return float(np.abs(Vh - d["V"][:, rows]).max())


def case(n, name, k, kappa=1e2, seed=None, mean_scale=0.0):
    """``design`` of the named spectrum plus its yardstick, built once per session and shared (read-only arrays).
    Returns (d, yard, k, exempt)."""
    return _case(int(n), name, int(k), float(kappa), seed, float(mean_scale))


@functools.lru_cache(maxsize=None)
def _case(n, name, k, kappa, seed, mean_scale):
    lam, k, exempt = spectrum(name, n, k)
    seed = (1000 * n + 7 * k + SPECTRA.index(name)) if seed is None else seed
    mean = None
    if mean_scale:
        mean = mean_scale * np.random.RandomState(seed + 1).standard_normal(n)
    d = design(n, lam, kappa=kappa, seed=seed, mean=mean, k=k)
    return d, host_yardstick(d, k), k, exempt


def s_projector_defect(Vdev, S, Vref):
    """max |P P^T - I| with P = Vdev^T S Vref: 0 when the two S-orthonormal sets span the same subspace."""
    P = Vdev.T.dot(S).dot(Vref)
    return float(np.abs(P.dot(P.T) - np.eye(P.shape[0])).max())


def pencil_residual(OC, S, v, lam):
    """(max |OC v - lam S v|, max |S v|) in extended precision: the test's own rounding stays out of the figure."""
    L = np.longdouble
    Sv = S.astype(L).dot(v.astype(L))
    r = OC.astype(L).dot(v.astype(L)) - L(lam) * Sv
    return float(np.abs(r).max()), float(np.abs(Sv).max())
