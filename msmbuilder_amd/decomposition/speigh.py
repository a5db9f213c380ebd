"""Sparse approximate generalized eigenpairs on the device (``decomposition/_speigh.pyx`` of msmbuilder).

``speigh`` approximates  max x^T A x - rho |x|_0  s.t.  x^T B x <= 1  by the majorisation-minimisation of Sriperumbudur,
Torres and Lanckriet (2011): each outer step is an ADMM solve, each ADMM iteration a soft threshold and a projection onto
the ellipsoid.  Outer and inner loops run in one persistent launch (``csrc/speigh_dev.h``); there is no host
implementation behind it.  Arguments are numpy arrays or torch tensors on the device; results follow the inputs.

Switches (read per call): ``MSM_SPEIGH_BUDGET`` ADMM iterations per launch, ``MSM_SPEIGH_GRID`` workgroups.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._lib import Arr, check, empty_like_placement

__all__ = ['speigh', 'scdeflate', 'project', 'solve_admm']

STATUS = {0: 'converged', 1: 'maxiter', 2: 'barrier timeout'}
MAX_FEATURES = 2048


def _run(rc):
    if rc == _lib.MSM_ERR_INVALID and "positive definite" in _lib.last_error():
        raise np.linalg.LinAlgError(_lib.last_error())
    check(rc)


def _square(M, name):
    a = Arr(M, np.float64)
    if len(a.shape) != 2 or a.shape[0] != a.shape[1]:
        raise ValueError('%s must be a square matrix' % name)
    return a


def _transposed(V):
    """Eigenvectors in columns (the reference's and LAPACK's layout) -> one eigenvector per row, contiguous."""
    if _lib.is_device_array(V):
        return V.t().contiguous()
    return np.ascontiguousarray(np.asarray(V, dtype=np.float64).T)


def _vp(a):
    return None if a is None else a.vp


def scdeflate(A, x):
    """Schur complement deflation ``A - outer(A x, x A) / (x A x)`` (Mackey 2008)."""
    a = _square(A, 'A')
    v = Arr(x, np.float64)
    n = a.shape[0]
    if v.shape != (n,) or v.on_device != a.on_device:
        raise ValueError('x must be a vector of %d entries placed like A' % n)
    out = empty_like_placement(a, (n, n), np.float64)
    o = Arr(out)
    check(_lib.lib().msm_scdeflate(a.vp, v.vp, n, o.vp, a.on_device))
    return out


def project(a, w, V, out=None):
    """Projection of ``a`` onto ``{x : x^T B x <= 1}``, ``(w, V)`` the eigenvalues and eigenvectors (columns) of ``B``.
    Written into ``out`` when given (the reference's calling convention) and returned."""
    va, vw, vE = Arr(a, np.float64), Arr(w, np.float64), Arr(_transposed(V), np.float64)
    n = va.shape[0] if len(va.shape) == 1 else -1
    if n < 0 or vw.shape != (n,) or vE.shape != (n, n):
        raise ValueError('Incompatible matrix dimensions')
    if not (va.on_device == vw.on_device == vE.on_device):
        raise ValueError('a, w and V must all be on the host or all on the device')
    res = empty_like_placement(va, (n,), np.float64)
    check(_lib.lib().msm_speigh_project(va.vp, vw.vp, vE.vp, n, Arr(res).vp, va.on_device))
    if out is not None:
        out[:] = res
        return out
    return res


def solve_admm(b, w, B_eigvals, B_eigvecs, x, tol=1e-6, maxiter=100, verbose=0, return_info=False):
    """Minimise ``1/2 |x - b|^2 + |D(w) x|_1`` subject to ``x^T B x <= 1`` by ADMM, warm-started at ``x``, which is
    overwritten with the soft-thresholded iterate.  Returns the objective (and the ``info`` dictionary on request)."""
    vb, vw, ve, vE = Arr(b, np.float64), Arr(w, np.float64), Arr(B_eigvals, np.float64), Arr(_transposed(B_eigvecs), np.float64)
    vx = Arr(x, np.float64)
    n = vb.shape[0] if len(vb.shape) == 1 else -1
    if n < 0 or not (vw.shape == ve.shape == vx.shape == (n,)) or vE.shape != (n, n):
        raise ValueError('Incompatible matrix dimensions')
    if not (vb.on_device == vw.on_device == ve.on_device == vE.on_device == vx.on_device):
        raise ValueError('all arrays must be on the host or all on the device')
    info = np.zeros(4)
    check(_lib.lib().msm_speigh_admm(vb.vp, vw.vp, ve.vp, vE.vp, vx.vp, n, float(tol), int(maxiter),
                                     info.ctypes.data_as(C.POINTER(C.c_double)), vb.on_device))
    if vx.keep is not x:
        x[:] = vx.keep      # (a converted copy was solved: hand the result back in place)
    if vb.on_device:
        xs, bs, ws = vx.keep, vb.keep, vw.keep
        fun = float(0.5 * (xs @ xs) - xs @ bs + 0.5 * (bs @ bs) + (ws * xs).abs().sum())
    else:
        xs, bs, ws = vx.keep, vb.keep, vw.keep
        fun = float(0.5 * np.dot(xs, xs) - np.dot(xs, bs) + 0.5 * np.dot(bs, bs) + np.sum(np.abs(ws * xs)))
    if return_info:
        return fun, {'iterations': int(info[0]), 'launches': int(info[1]), 'status': STATUS[int(info[2])], 'rho': float(info[3])}
    return fun


def speigh(A, B, rho, eps=1e-6, tol=1e-8, maxiter=100, verbose=False, method=1, x0=None, eigh_B=None, return_info=False):
    """A sparse approximate generalized eigenpair ``(u, v)`` of ``(A, B)``; larger ``rho`` gives sparser ``v``.

    ``x0`` (a start vector) and ``eigh_B = (eigenvalues, eigenvectors in columns)`` are taken from the device solves when
    not given.  With ``return_info`` a third value holds the counters of the solve and the iterate ``x`` itself."""
    if method != 1:
        raise ValueError('method=%r is not supported: only method=1 (the ADMM solver) is built; method=2 needs cvxpy' % (method,))
    if not (rho >= 0 and eps > 0 and tol > 0 and int(maxiter) >= 1):
        raise ValueError('speigh needs rho >= 0, eps > 0, tol > 0 and maxiter >= 1')
    a, b = _square(A, 'A'), _square(B, 'B')
    n = a.shape[0]
    if b.shape != a.shape:
        raise ValueError('Wrong B dimensions (%d, %d) should be (%d, %d)' % (b.shape + a.shape))
    if a.on_device != b.on_device:
        raise ValueError('A and B must both be on the host or both on the device')
    vx0 = None if x0 is None else Arr(x0, np.float64)
    ve = vE = None
    if eigh_B is not None:
        ve, vE = Arr(eigh_B[0], np.float64), Arr(_transposed(eigh_B[1]), np.float64)
        if ve.shape != (n,) or vE.shape != (n, n):
            raise ValueError('Incompatible matrix dimensions')
    for extra in (vx0, ve, vE):
        if extra is not None and extra.on_device != a.on_device:
            raise ValueError('x0 and eigh_B must be placed like A')
    if vx0 is not None and vx0.shape != (n,):
        raise ValueError('Incompatible matrix dimensions')
    u = C.c_double(0.0)
    v = empty_like_placement(a, (n,), np.float64)
    xit = empty_like_placement(a, (n,), np.float64)
    info = np.zeros(8)
    _run(_lib.lib().msm_speigh(a.vp, b.vp, n, float(rho), float(eps), float(tol), int(maxiter), _vp(vx0), _vp(ve), _vp(vE),
                               C.byref(u), Arr(v).vp, Arr(xit).vp, info.ctypes.data_as(C.POINTER(C.c_double)), a.on_device))
    if verbose:
        print("speigh: %d outer steps, %d ADMM iterations, objective=%.5f, %d/%d active" % (info[0], info[1], info[3], info[4], n))
    if return_info:
        return u.value, v, {'outer': int(info[0]), 'admm': int(info[1]), 'launches': int(info[2]), 'objective': float(info[3]),
                            'nnz': int(info[4]), 'status': STATUS[int(info[5])], 'workgroups': int(info[6]), 'tau': float(info[7]),
                            'x': xit}
    return u.value, v
