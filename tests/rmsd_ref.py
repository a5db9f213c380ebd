"""tests/rmsd_ref.py -- TEST INFRASTRUCTURE: the rmsd metric restated in numpy, and the rounding bound of the device's.

Written from the published formulas (Theobald, Acta Cryst. A61 (2005) 478; Liu, Agrafiotis & Theobald, J. Comput. Chem. 31
(2010) 1561), not from any implementation's text.  For conformations x, y of A atoms, each minus its centroid,

    M_ab = sum_k x_ka y_kb,   G_x = sum_k |x_k|^2,   msd = (G_x + G_y - 2 lambda_max(K(M))) / A,   rmsd = sqrt(max(msd, 0))

with K the symmetric traceless 4 x 4 key matrix, linear in M (``key_matrix``).

The restatement (``Frames``, ``cdist`` ...) shares only the INPUT rounding with the library: the centroid is the float64
sum over the atoms in order divided by A, and coordinates minus centroid are formed in float64 and rounded once to
float32 (include/msmhip.h, msm_rmsd_prepare).  From those float32 values on it goes its own way: M and G in longdouble,
K rounded to float64, lambda_max by ``numpy.linalg.eigvalsh`` -- deliberately not Newton on the quartic.

The bound (``pair_bound``) -- derived, not fitted.  Write u32 = 2^-24, u64 = 2^-53, lam0 = (G_x + G_y) / 2 >= lambda_max
(msd >= 0), lam_1 >= lam_2 >= lam_3 >= lam_4 the eigenvalues of K(M), g_i = lam_1 - lam_i.

 1. chain    The library's M^ is a float32 fma chain of A steps (an MFMA or fmaf each: one rounding per step), so
             |M^_ab - M_ab| <= gamma_A sum_k |x_ka||y_kb|, gamma_A = A u32 / (1 - A u32), hence by Cauchy-Schwarz
             ||M^ - M||_F <= gamma_A sqrt(G_x G_y).  K is linear in M with ||K(D)||_F = 2 ||D||_F, and Weyl's inequality
             moves every eigenvalue by at most ||K(D)||_2 <= ||K(D)||_F:        e_chain = 2 gamma_A sqrt(G_x G_y).
 2. stop     For a real-rooted quartic P and x above its largest root r, the Newton step s = P/P' = 1 / sum_i 1/(x - r_i)
             lies in [(x - r)/4, x - r]: the iterates fall monotonically to r, each step removes at least a quarter of the
             error.  The loop ends on |s| < tol |x| -- then the error left is at most 3 |s| < 3 tol lam0 -- or after 50
             steps -- then at most (3/4)^50 of the starting error lam0 - lam_1 (a repeated largest root converges only
             linearly, which this covers):                           e_stop = 3 tol lam0 + (3/4)^50 (lam0 - lam_1).
 3. floor    The coefficients and Horner's rule are float64.  With |M_ab| <= ||M||_F <= sqrt(G_x G_y) <= lam0 every entry of
             K is at most sqrt(3) lam0, and counting roundings -- det K as 24 products of four entries (<= 9 lam0^4 each, <=
             12 roundings: 2592 u64 lam0^4) summed (1296), C1 lam (288), C2 lam^2 (22), Horner's four operations (~10) --
             the evaluated P differs from the exact quartic of K(M^) by at most delta = 4400 u64 lam0^4.  Newton cannot
             tell x from the root once P(x) <= delta; allowing a factor 4 for the same noise in the step's quotient, and
             with P(r + e) = e prod_{i>1} (e + g_i), the iteration stalls within e_floor of the root, the solution of
             e prod (e + g^_i) = 4 delta.  The gaps are those of K(M^): g^_i = max(g_i - 2 e_chain, 0).  At a simple
             root this is ~ delta / prod g_i; at a double root (collinear conformations, A = 2) its square root.
 4. branch   M^'s largest root can exceed lam0 by up to e_chain, so the start can lie just BELOW it.  From between the two
             largest roots Newton still lands on one of them; the lower one only if the local minimum between them is
             within e_chain of the top, i.e. g^_2 <~ 2 e_chain -- then the answer is off by the gap as well:
                                                    e_branch = g_2 + 2 e_chain   if g_2 <= 4 e_chain, else 0.
 5. ref      eigvalsh on the float64 K (backward stable) and K's own rounding: e_ref = 16 u64 lam0.

    |lambda^ - lam_1| <= e_chain + e_stop + e_floor + e_branch + e_ref =: e_lam
    |msd^ - msd|      <= 2 e_lam / A + (3 A + 8) u64 (G_x + G_y) / A          (G^ is a float64 sum of 3 A squares)
    |d^ - d|          <= min(sqrt(e_msd), e_msd / d) + 4 u64 d                 (|sqrt a - sqrt b| <= both; sqrt's rounding)

Not covered: a Newton iterate that lands, by the noise of item 3, within that noise of a stationary point of P (the
quotient is then arbitrary).  The hand cases include the double roots where this could show.

Also here: the loops of ``assign_nearest`` (libdistance.pyx:343-355) and k-centers (kcenters.py:79-102) over the
restated distances with their decision margins, an emulation of the library's arithmetic order in numpy, and the
inputs the tests share, from seeds.
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
NEWTON_TOL = 1e-11
NEWTON_MAX = 50
NOISE_ROUNDINGS = 4400.0
# (frames, conformations = centres, atoms, seed) of the planted inputs the decision tests use
DECISION_CASES = [(80, 5, 33, 1), (129, 33, 5, 2), (200, 8, 257, 3), (300, 65, 4, 4)]
FLT_MAX = float(np.finfo(np.float32).max)


# ---- the restatement -----------------------------------------------------------------------------------------------
def centre(xyz):
    """Frames minus their centroids as the library stores them: float64 centroid (atoms added in order), float64
    difference, one rounding to float32."""
    xyz = np.asarray(xyz)
    assert xyz.ndim == 3 and xyz.shape[2] == 3 and xyz.dtype == np.float32
    x64 = xyz.astype(np.float64)
    if xyz.shape[1] == 0:
        return xyz.copy()
    centroid = np.add.accumulate(x64, axis=1)[:, -1, :] / float(xyz.shape[1])   # accumulate is sequential by definition
    with np.errstate(invalid='ignore'):   # inf - inf of a frame that is not finite
        return (x64 - centroid[:, None, :]).astype(np.float32)


class Frames(object):
    """Centred float32 coordinates ``c`` (n, A, 3) and the exact sums of squares ``G`` (longdouble)."""

    def __init__(self, xyz):
        self.c = centre(xyz)
        self.n, self.A = self.c.shape[:2]
        cl = self.c.astype(np.longdouble)
        self.G = (cl * cl).sum(axis=(1, 2))


def key_matrix(M):
    """K(M) for M of shape (..., 3, 3): the 4 x 4 matrix whose largest eigenvalue is the maximum of sum_k x_k . R y_k."""
    Sxx, Sxy, Sxz = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    Syx, Syy, Syz = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    Szx, Szy, Szz = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    K = np.empty(M.shape[:-2] + (4, 4), dtype=M.dtype)
    K[..., 0, 0] = Sxx + Syy + Szz
    K[..., 1, 1] = Sxx - Syy - Szz
    K[..., 2, 2] = -Sxx + Syy - Szz
    K[..., 3, 3] = -Sxx - Syy + Szz
    K[..., 0, 1] = K[..., 1, 0] = Syz - Szy
    K[..., 0, 2] = K[..., 2, 0] = Szx - Sxz
    K[..., 0, 3] = K[..., 3, 0] = Sxy - Syx
    K[..., 1, 2] = K[..., 2, 1] = Sxy + Syx
    K[..., 1, 3] = K[..., 3, 1] = Szx + Sxz
    K[..., 2, 3] = K[..., 3, 2] = Syz + Szy
    return K


def solve_floor(rhs, gaps):
    """The e >= 0 with e * prod(e + gaps) = rhs, per element (gaps: (..., 3) >= 0), by bisection on a monotone function;
    returned from above."""
    rhs = np.asarray(rhs, dtype=np.float64)
    hi = np.maximum(rhs, 0.0) ** 0.25 + 1e-300   # e^4 <= e prod(e + g): the root is at most rhs^(1/4)
    lo = np.zeros_like(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        val = mid * np.prod(mid[..., None] + gaps, axis=-1)
        up = val >= rhs
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return hi


def pair_bound(A, Gx, Gy, eig, d):
    """The bound of the module docstring for pairs with sums of squares Gx, Gy, eigenvalues ``eig`` (..., 4) ascending,
    restated distance d.  NaN where the pair is not finite."""
    Gx, Gy, d = np.asarray(Gx, np.float64), np.asarray(Gy, np.float64), np.asarray(d, np.float64)
    gamma = A * U32 / (1.0 - A * U32)
    lam0 = 0.5 * (Gx + Gy)
    lam1 = eig[..., 3]
    gaps = lam1[..., None] - eig[..., 2::-1]   # g_2, g_3, g_4
    e_chain = 2.0 * gamma * np.sqrt(Gx * Gy)
    e_stop = 3.0 * NEWTON_TOL * lam0 + 0.75 ** NEWTON_MAX * np.maximum(lam0 - lam1, 0.0)
    delta = NOISE_ROUNDINGS * U64 * lam0 ** 4
    e_floor = solve_floor(4.0 * delta, np.maximum(gaps - 2.0 * e_chain[..., None], 0.0))
    e_branch = np.where(gaps[..., 0] <= 4.0 * e_chain, gaps[..., 0] + 2.0 * e_chain, 0.0)
    e_ref = 16.0 * U64 * lam0
    e_lam = e_chain + e_stop + e_floor + e_branch + e_ref
    e_msd = 2.0 * e_lam / A + (3.0 * A + 8.0) * U64 * (Gx + Gy) / A
    with np.errstate(divide='ignore', invalid='ignore'):
        e_d = np.minimum(np.sqrt(e_msd), np.where(d > 0, e_msd / d, np.inf)) + 4.0 * U64 * d
    return e_d


def cdist(fx, fy, with_bound=True):
    """(D, B): restated float64 distances between every frame of ``fx`` and of ``fy`` (``Frames``) and their bounds.
    A frame with a non-finite coordinate gives NaN distances (and NaN bounds)."""
    assert fx.A == fy.A
    A = fx.A
    D = np.full((fx.n, fy.n), np.nan)
    B = np.full((fx.n, fy.n), np.nan)
    okx = np.isfinite(fx.c).all(axis=(1, 2))
    oky = np.isfinite(fy.c).all(axis=(1, 2))
    if not (okx.any() and oky.any()):
        return (D, B) if with_bound else D
    x = fx.c[okx].astype(np.longdouble)
    y = fy.c[oky].astype(np.longdouble)
    M = np.einsum('ika,jkb->ijab', x, y)
    K = key_matrix(M).astype(np.float64)
    eig = np.linalg.eigvalsh(K)
    Gx, Gy = fx.G[okx][:, None], fy.G[oky][None, :]
    msd = (Gx + Gy - 2.0 * eig[..., 3].astype(np.longdouble)) / A
    d = np.sqrt(np.maximum(msd, 0)).astype(np.float64)
    D[np.ix_(okx, oky)] = d
    if with_bound:
        B[np.ix_(okx, oky)] = pair_bound(A, Gx.astype(np.float64) + 0 * d, Gy.astype(np.float64) + 0 * d, eig, d)
        return D, B
    return D


def condensed(S):
    """The strict upper triangle of a square array in pdist order."""
    return S[np.triu_indices(len(S), 1)]


# ---- the reference's loops over given distances ------------------------------------------------------------------------
def assign_loop(D):
    """libdistance.pyx:343-355 on a distance matrix (frames x centres): labels, the minimum distances (FLT_MAX where none
    is below it: a NaN never wins), the inertia added in row order, and each row's margin = second-smallest minus
    smallest distance (inf with one centre, 0 when nothing won)."""
    n, K = D.shape
    labels = np.zeros(n, dtype=np.intp)
    mind = np.full(n, FLT_MAX)
    for j in range(K):
        better = D[:, j] < mind
        labels[better] = j
        mind[better] = D[better, j]
    filled = np.where(np.isnan(D), np.inf, D)
    part = np.sort(filled, axis=1)
    with np.errstate(invalid='ignore'):
        margin = part[:, 1] - part[:, 0] if K > 1 else np.full(n, np.inf)
    margin = np.where(np.isfinite(part[:, 0]), margin, 0.0)
    return labels, mind, float(np.add.accumulate(mind)[-1]) if n else 0.0, margin


def kcenters_loop(column, n, K, seed, follow=None):
    """kcenters.py:79-102 with ``column(i)`` = (distances of every frame to frame i, their bounds).  ``follow``: centre ids
    to take instead of the loop's own argmax from the second on (the library's, when a check walks beside it).
    Returns dict(ids, labels, distances, steps) -- steps[k] for the choice made AFTER pass k: (own argmax, its value, the
    gap to the largest value at any other row, the largest bound of that pass)."""
    labels = np.zeros(n, dtype=np.intp)
    distances = np.full(n, np.inf)
    ids, steps, centre_cols, centre_bounds = [], [], [], []
    nxt = int(seed)
    for k in range(K):
        d, b = column(nxt)
        mask = d < distances
        distances[mask] = d[mask]
        labels[mask] = k
        ids.append(nxt)
        centre_cols.append(d)
        centre_bounds.append(b)
        own = int(np.argmax(distances))
        rest = np.delete(distances, own)
        gap = distances[own] - (rest.max() if len(rest) else -np.inf)
        steps.append((own, distances[own], gap, np.nanmax(np.stack(centre_bounds)) if n else 0.0))
        nxt = own if follow is None or k + 1 >= len(follow) else int(follow[k + 1])
    D = np.stack(centre_cols, axis=1)
    return dict(ids=ids, labels=labels, distances=distances, steps=steps, D=D, B=np.stack(centre_bounds, axis=1))


# ---- the library's arithmetic order, emulated ---------------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum rounds to float64 and then to float32 (a double
    rounding can differ from the fused result in the last float32 bit on rare ties -- the emulation is held to the bound,
    not to the library's bits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def device_order(fx, fy):
    """Distances by the library's definition: float32 fma chain over the atoms from atom 0, float64 coefficients of the
    quartic, Newton from (G_x + G_y) / 2.  Returns (D, the largest number of Newton steps taken)."""
    A = fx.A
    Gx = np.add.accumulate((fx.c.astype(np.float64) ** 2).reshape(fx.n, -1), axis=1)[:, -1] if A else np.zeros(fx.n)
    Gy = np.add.accumulate((fy.c.astype(np.float64) ** 2).reshape(fy.n, -1), axis=1)[:, -1] if A else np.zeros(fy.n)
    M = np.zeros((fx.n, fy.n, 3, 3), dtype=np.float32)
    for k in range(A):
        M = fmaf(np.broadcast_to(fx.c[:, None, k, :, None], M.shape), np.broadcast_to(fy.c[None, :, k, None, :], M.shape), M)
    S = M.astype(np.float64)
    C2 = -2.0 * (S ** 2).sum(axis=(2, 3))
    C1 = -8.0 * np.linalg.det(S)
    C0 = np.linalg.det(key_matrix(S))
    Gs = Gx[:, None] + Gy[None, :]
    lam = Gs / 2.0
    live = np.ones(lam.shape, dtype=bool)
    most = 0
    with np.errstate(all='ignore'):
        for it in range(NEWTON_MAX):
            l2 = lam * lam
            b = (l2 + C2) * lam
            a = b + C1
            P = a * lam + C0
            dP = 2.0 * l2 * lam + b + a
            live &= dP != 0.0
            if not live.any():
                break
            most = it + 1
            step = np.where(live, P / np.where(dP == 0.0, 1.0, dP), 0.0)
            lam = lam - step
            live &= ~(np.abs(step) < NEWTON_TOL * np.abs(lam))
        msd = (Gs - 2.0 * lam) / A
        return np.sqrt(np.where(msd < 0.0, 0.0, msd)), most


# ---- shared inputs, from seeds ---------------------------------------------------------------------------------------------
def random_rotation(rs):
    """A proper rotation matrix (QR of a Gaussian matrix, determinant fixed to +1)."""
    Q, R = np.linalg.qr(rs.randn(3, 3))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def gaussian_frames(n, A, seed, offset=0.0, spread=1.0):
    rs = np.random.RandomState(seed)
    return (offset + spread * rs.randn(n, A, 3)).astype(np.float32)


def planted(n, K, A, seed, noise=1e-2):
    """(frames, the K conformations, each frame's conformation): every frame is one of K random conformations plus
    ``noise``, under a random proper rotation and a translation."""
    rs = np.random.RandomState(seed)
    shapes = rs.randn(K, A, 3)
    which = rs.randint(0, K, size=n)
    which[:min(n, K)] = np.arange(min(n, K))   # every conformation occurs when n >= K
    out = np.empty((n, A, 3), dtype=np.float32)
    for i in range(n):
        out[i] = ((shapes[which[i]] + noise * rs.randn(A, 3)) @ random_rotation(rs).T + 3.0 * rs.randn(3)).astype(np.float32)
    return out, shapes.astype(np.float32), which


def degenerate_frames():
    """Named hand cases, (x, y) single conformations, with what the distance must be: 'zero' (within the bound of 0),
    'positive', or None."""
    rs = np.random.RandomState(7)
    base = rs.randn(12, 3)
    Rm = random_rotation(rs)
    line = np.outer(np.linspace(-2.0, 3.0, 9), [1.0, 2.0, -0.5])
    plane = np.c_[rs.randn(10, 2), np.zeros(10)]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)[None]
    return {
        'identical': (f(base), f(base), 'zero'),
        'rotated_translated': (f(base), f(base @ Rm.T + [5.0, -3.0, 2.0]), 'zero'),
        'mirror': (f(base), f(base * [1.0, 1.0, -1.0]), 'positive'),
        'collinear_same': (f(line), f(line @ Rm.T), 'zero'),
        'collinear_other': (f(line), f(np.outer(np.linspace(-2.0, 3.0, 9) ** 2, [0.3, -1.0, 1.0])), 'positive'),
        'planar_same': (f(plane), f(plane @ Rm.T - 1.0), 'zero'),
        'planar_other': (f(plane), f(np.c_[rs.randn(10, 2), np.zeros(10)]), 'positive'),
        'one_atom': (f(rs.randn(1, 3)), f(rs.randn(1, 3)), 'zero'),
        'two_atoms_same': (f(base[:2]), f(base[:2] @ Rm.T + 1.0), 'zero'),
        'two_atoms_other': (f(base[:2]), f(1.5 * base[2:4]), 'positive'),
    }
