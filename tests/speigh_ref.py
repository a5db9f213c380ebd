"""Numpy restatement of the sparse generalized eigenpair solver (Sriperumbudur, Torres, Lanckriet 2011, with the ADMM
inner solve and the ellipsoid projection of msmbuilder's ``_speigh``), written from the formulas, and the seeded generator
of the test matrices.  ``dtype`` is float64 or longdouble: the loops run in it, the dense eigensolves are LAPACK's float64.

    speigh      maximise x^T A x - rho_e sum log(|x_j| + eps)  s.t. x^T B x <= 1, rho_e = rho / log1p(1 / eps):
                tau = 0.1 + max(0, -lambda_min(A)); from the top generalized eigenvector, repeat
                    f = x^T A x - rho_e sum log(|x| + eps); stop when |f_old - f| < tol
                    b = A x / tau + x,  w = rho_e / (2 tau (|x| + eps)),  x <- solve_admm(b, w; warm start x)
                then the unconstrained top pair on the rows and columns where x != 0.
    solve_admm  min 1/2 |x - b|^2 + |D(w) x|_1  s.t. x^T B x <= 1 (Boyd et al. 2011, 3.4.1 with the varying penalty
                of eq. 3.13): rho = 16, z = x, u = 0; x <- soft(b + rho (z - u), |w|) / (rho + 1); z <- project(x + u);
                r = x - z, s = rho (z - z_old), u += r; stop when |r|^2 and |s|^2 < N tol^2; rho doubles (u halves) when
                |r|^2 > 100 |s|^2 and rho < 2^10, halves (u doubles) when |s|^2 > 100 |r|^2 and rho > 2^-10.
    project     nearest point of {x : x^T B x <= 1}, B = V diag(w) V^T: c = V^T a; a itself when sum c^2 w < 1, else
                V (c / (mu w + 1)) with mu the root of sum c^2 w / (mu w + 1)^2 = 1 (Newton from 0, <= 100 steps,
                until |delta| < 1e-12).
"""
import numpy as np
import scipy.linalg
from scipy.signal import lfilter

LAG = 5
PHIS = (0.995, 0.965, 0.935)


def project(a, w, V, dtype=np.float64):
    a, w, V = np.asarray(a, dtype), np.asarray(w, dtype), np.asarray(V, dtype)
    c = V.T.dot(a)
    c2w = c * c * w
    if c2w.sum() < 1:
        return a.copy()
    mu = dtype(0)
    for _ in range(100):
        m = mu * w + 1
        G = (c2w / (m * m)).sum() - 1
        Gp = -(2 * c2w * w / (m * m * m)).sum()
        delta = -G / Gp
        mu = mu + delta
        if abs(delta) < 1e-12:
            break
    return V.dot(c / (mu * w + 1))


def solve_admm(b, w, evals, V, x, tol=1e-6, maxiter=100, dtype=np.float64):
    """Returns (x, info): the soft-thresholded iterate and {'iterations', 'doubled', 'halved', 'rho', 'status'}."""
    b, evals, V = np.asarray(b, dtype), np.asarray(evals, dtype), np.asarray(V, dtype)
    absw = np.abs(np.asarray(w, dtype))
    x = np.array(x, dtype)
    N = len(b)
    rho = dtype(16)
    z = x.copy()
    u = np.zeros(N, dtype)
    doubled = halved = 0
    status = 'maxiter'
    it = 0
    bound = N * dtype(tol) * dtype(tol)
    for it in range(1, maxiter + 1):
        z_old = z
        q = b + rho * (z - u)
        x = np.where(q > absw, q - absw, np.where(q < -absw, q + absw, dtype(0))) / (rho + 1)
        z = project(x + u, evals, V, dtype)
        r = x - z
        s = rho * (z - z_old)
        u = u + r
        r2, s2 = r.dot(r), s.dot(s)
        if r2 < bound and s2 < bound:
            status = 'converged'
            break
        if r2 > 100 * s2 and rho < 1024:
            rho = rho * 2
            u = u / 2
            doubled += 1
        if s2 > 100 * r2 and rho > dtype(1) / 1024:
            rho = rho / 2
            u = u * 2
            halved += 1
    return x, {'iterations': it, 'doubled': doubled, 'halved': halved, 'rho': float(rho), 'status': status}


def top_pair(A, B):
    """Largest generalized eigenvalue and its eigenvector (LAPACK, float64)."""
    n = len(A)
    vals, vecs = scipy.linalg.eigh(np.asarray(A, np.float64), np.asarray(B, np.float64), subset_by_index=(n - 1, n - 1))
    return vals[0], vecs[:, 0]


def finish(A, B, x):
    """The pair on the sparsity pattern of x: closed forms for 0 or 1 nonzeros, sum(v) >= 0, no negative zeros."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    N = len(A)
    mask = np.abs(np.asarray(x, np.float64)) > 0
    nnz = int(mask.sum())
    v = np.zeros(N)
    if nnz == 0:
        return 0.0, v, mask
    if nnz == 1:
        i = int(np.flatnonzero(mask)[0])
        v[i] = 1.0 / np.sqrt(B[i, i])
        return A[i, i] / B[i, i], v, mask
    u, vk = top_pair(A[np.ix_(mask, mask)], B[np.ix_(mask, mask)])
    v[mask] = vk
    v = v * np.sign(v.sum())
    v[v == 0] = 0.0
    return float(u), v, mask


def speigh(A, B, rho, eps=1e-6, tol=1e-8, maxiter=100, dtype=np.float64, x0=None, eigh_B=None):
    """Returns (u, v, info): info = {'outer' (ADMM solves), 'admm' (iterations in all), 'x', 'mask', 'objective', 'status',
    'doubled', 'halved'}."""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    Ad = A64.astype(dtype)
    N = len(A64)
    rho_e = dtype(rho) / np.log1p(1 / dtype(eps))
    tau = dtype(0.1) + dtype(max(0.0, -scipy.linalg.eigvalsh(A64).min()))
    x = np.asarray(top_pair(A64, B64)[1] if x0 is None else x0, dtype)
    evals, V = scipy.linalg.eigh(B64) if eigh_B is None else eigh_B
    f = dtype(np.inf)
    outer = admm = doubled = halved = 0
    status = 'maxiter'
    for _ in range(maxiter):
        f_old = f
        Ax = Ad.dot(x)
        f = Ax.dot(x) - (rho_e * np.log(np.abs(x) + dtype(eps))).sum()
        if abs(f_old - f) < tol:
            status = 'converged'
            break
        b = Ax / tau + x
        w = rho_e / (2 * tau * (np.abs(x) + dtype(eps)))
        x, inner = solve_admm(b, w, evals, V, x, tol=tol, maxiter=maxiter, dtype=dtype)
        outer += 1
        admm += inner['iterations']
        doubled += inner['doubled']
        halved += inner['halved']
    u, v, mask = finish(A64, B64, x)
    return u, v, {'outer': outer, 'admm': admm, 'x': x, 'mask': mask, 'objective': float(f), 'status': status,
                  'doubled': doubled, 'halved': halved}


def scdeflate(A, x, dtype=np.float64):
    A, x = np.asarray(A, dtype), np.asarray(x, dtype)
    return A - np.outer(A.dot(x), x.dot(A)) / x.dot(A).dot(x)


# ---- the seeded family of test matrices -------------------------------------------------------------------------------
def rows(F, seed, N=None):
    """N x F Gaussian rows carrying three AR(1) processes (phi = 0.995, 0.965, 0.935; unit variance), each added to six
    random columns with weights geomspace(2, 0.1, 6); per-column scale U(0.5, 2) and offset U(-50, 50)."""
    rs = np.random.RandomState(seed)
    N = 4000 + 10 * F if N is None else N
    X = rs.randn(N, F)
    for phi in PHIS:
        p = lfilter([np.sqrt(1 - phi * phi)], [1.0, -phi], rs.randn(N))
        cols = rs.choice(F, min(6, F), replace=False)
        X[:, cols] += p[:, None] * np.geomspace(2, 0.1, 6)[:len(cols)]
    return X * rs.uniform(0.5, 2.0, F) + rs.uniform(-50.0, 50.0, F)


def moments(X, lag=LAG):
    """A = the symmetrised lagged covariance, B = the mean of the two instantaneous ones (both about the common mean)."""
    X0, X1 = X[:-lag], X[lag:]
    mu = 0.5 * (X0.mean(0) + X1.mean(0))
    X0, X1 = X0 - mu, X1 - mu
    n = len(X0)
    C = X0.T.dot(X1) / n
    return 0.5 * (C + C.T), 0.5 * (X0.T.dot(X0) + X1.T.dot(X1)) / n


def matrices(F, seed):
    return moments(rows(F, seed))


def two_well_rows(seed, N=20000, F=10):
    """A two-well process on feature 0 -- a two-state jump process that keeps its well with probability 0.995 per frame,
    plus Gaussian noise of width 0.2 inside the well -- and F - 1 white-noise features."""
    rs = np.random.RandomState(seed)
    stay = rs.rand(N) < 0.995
    state = np.empty(N)
    s = 1.0
    for t in range(N):
        if not stay[t]:
            s = -s
        state[t] = s
    X = rs.randn(N, F)
    X[:, 0] = state + 0.2 * rs.randn(N)
    return X
