#!/usr/bin/env python
"""Measurements of the sparse eigenpair solver (csrc/speigh_dev.h) on one GPU -> profiles/speigh_probe.txt.

    python scripts/speigh_probe.py [--out profiles/speigh_probe.txt] [--widths 64,128,512,1024,2048]

1. Time per ADMM iteration: msm_speigh_admm with a tolerance that is never met, the slope between two iteration counts
   (launch and copies cancel), per layout: the single-workgroup layout where E fits in LDS, the row-owning layout at
   several grids.  The barrier share is bounded from below where both layouts run: the single-workgroup layout does all of
   the arithmetic of the row-owning one and more, without a grid barrier.
2. A SparseTICA(n_components=10, rho=1e-3) solve split into its parts (each timed on its own through the C ABI).
3. The float64 numpy restatement (tests/speigh_ref.py) on this host in the same run.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speigh_ref as R  # noqa: E402

EPS, TOL, MAXITER = 1e-6, 1e-6, 10000
BUDGET = 2048          # SPG_BUDGET_DEFAULT of csrc/speigh.hip


def wall(fn, repeat=3):
    best = np.inf
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speigh_probe.txt"))
    ap.add_argument("--widths", default="64,128,512,1024,2048")
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    import scipy.linalg
    import torch
    from msmbuilder_amd import SparseTICA, _lib
    from msmbuilder_amd.decomposition import speigh as S
    _lib.ensure_device(0)
    L = _lib.lib()
    name = ctypes_name(L)
    lines = ["speigh probe: %s, %s" % (name, time.strftime("%Y-%m-%d")),
             "budget per launch (SPG_BUDGET_DEFAULT): %d ADMM iterations" % BUDGET, ""]
    say = lambda s: (print(s, flush=True), lines.append(s))  # noqa: E731

    say("1. time per ADMM iteration (us; slope between 500 and 2500 iterations at a tolerance that is never met)")
    say("   %-6s %-28s %10s" % ("F", "layout", "us/iter"))
    per_iter = {}
    cache = {}
    for F in widths:
        A, B = R.matrices(F, F)
        cache[F] = (A, B)
        w, V = scipy.linalg.eigh(B)
        x0 = R.top_pair(A, B)[1]
        tau = 0.1 + max(0.0, -scipy.linalg.eigvalsh(A).min())
        rho_e = 1e-3 / np.log1p(1 / EPS)
        dev = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (A.dot(x0) / tau + x0, rho_e / (2 * tau * (np.abs(x0) + EPS)), w, V)]
        grids = (["1"] if F <= 128 else []) + [g for g in ("2", "8", "64", "256") if int(g) <= F]
        single = None
        for g in grids:
            os.environ["MSM_SPEIGH_GRID"] = g
            os.environ["MSM_SPEIGH_BUDGET"] = "1000000"
            t = {}
            for iters in (500, 2500):
                def go():
                    x = torch.as_tensor(x0).cuda()
                    S.solve_admm(dev[0], dev[1], dev[2], dev[3], x, tol=1e-300, maxiter=iters)
                go()
                t[iters] = wall(go)
            us = (t[2500] - t[500]) / 2000 * 1e6
            layout = "one workgroup, E in LDS" if (g == "1" and F <= 128) else "row-owning, %s workgroups" % g
            per_iter[(F, g)] = us
            if g == "1" and F <= 128:
                single = us
            extra = ""
            if single is not None and g != "1":
                extra = "   barrier share >= %.2f" % max(0.0, 1 - single / us)
            say("   %-6d %-28s %10.2f%s" % (F, layout, us, extra))
        os.environ.pop("MSM_SPEIGH_GRID")
        os.environ.pop("MSM_SPEIGH_BUDGET")
    widest = max(widths)
    rule = per_iter[(widest, str(max(int(g) for (F, g) in per_iter if F == widest)))]      # the grid the rule picks: every CU
    say("   a launch of %d iterations (the default budget) at F = %d on the grid the rule picks: %.3f s" % (BUDGET, widest, BUDGET * rule * 1e-6))
    say("   barrier share above 128 features: not measured (no layout without the barrier runs there)")
    say("")

    say("2. SparseTICA(n_components=10, rho=1e-3), solve only (ms)")
    for F in (512, 2048):
        if F not in cache:
            continue
        X = R.rows(F, F)
        m = SparseTICA(n_components=10, lag_time=R.LAG, rho=1e-3).fit([X])
        m._is_dirty = True
        t0 = time.perf_counter()
        m._solve()
        total = time.perf_counter() - t0
        info = m.solve_info_
        A, B = m.offset_correlation_, m.covariance_
        dA, dB = torch.as_tensor(A).cuda(), torch.as_tensor(B).cuda()
        ev, E, vals, x = (torch.empty(F, dtype=torch.float64, device="cuda"), torch.empty(F, F, dtype=torch.float64, device="cuda"),
                          torch.empty(F, dtype=torch.float64, device="cuda"), torch.empty(F, dtype=torch.float64, device="cuda"))
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        t_eighB = wall(lambda: L.msm_syev_top(p(dB), F, F, p(ev), p(E), 1))
        t_lmin = wall(lambda: L.msm_syev_top(p(dA), F, F, p(vals), p(E), 1))
        t_start = wall(lambda: L.msm_sygv_top(p(dA), p(dB), F, 1, p(vals), p(x), 1))
        nnz = max(2, int(np.median([i["nnz"] for i in info])))
        Ak, Bk = np.ascontiguousarray(A[:nnz, :nnz]), np.ascontiguousarray(B[:nnz, :nnz])
        uu, vv = np.zeros(1), np.zeros(nnz)
        t_sub = wall(lambda: L.msm_sygv_top(Ak.ctypes.data, Bk.ctypes.data, nnz, 1, uu.ctypes.data, vv.ctypes.data, 0))
        admm = sum(i["admm"] for i in info)
        parts = t_eighB + 10 * (t_lmin + t_start + t_sub)
        say("   F=%-5d total %9.1f | eigh(B) once %8.1f | per component: lambda_min(A) %7.1f, start pair %7.1f, masked sub-problem "
            "(median %d nonzeros) %6.2f | persistent loop and copies, by difference %9.1f for %d ADMM iterations in %d outer steps"
            % (F, total * 1e3, t_eighB * 1e3, t_lmin * 1e3, t_start * 1e3, nnz, t_sub * 1e3, (total - parts) * 1e3, admm,
               sum(i["outer"] for i in info)))
    say("")

    say("3. comparators")
    for F in (512, 1024, 2048):
        if F not in cache:
            continue
        A, B = cache[F]
        t0 = time.perf_counter()
        u, v, info = R.speigh(A, B, 1e-3, EPS, TOL, MAXITER)
        t_host = time.perf_counter() - t0
        t_dev = wall(lambda: S.speigh(A, B, 1e-3, eps=EPS, tol=TOL, maxiter=MAXITER), repeat=2)
        ud, vd, idev = S.speigh(A, B, 1e-3, eps=EPS, tol=TOL, maxiter=MAXITER, return_info=True)
        say("   F=%-5d one component at rho=1e-3: float64 numpy restatement on this host %8.3f s (%d ADMM iterations, %d nonzeros); "
            "device, host arrays in and out %8.3f s (%d iterations, %d nonzeros, same mask: %s)"
            % (F, t_host, info["admm"], info["mask"].sum(), t_dev, idev["admm"], idev["nnz"], np.array_equal(info["mask"], np.abs(vd) > 0)))
    say("   the reference's compiled extension, one component at rho=1e-3, measured on a CPU-only machine and quoted as such: "
        "0.13 s at F = 512, 0.47 s at F = 1,024; F = 2,048: not measured")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def ctypes_name(L):
    buf = C.create_string_buffer(256)
    cus, mem = C.c_int(0), C.c_int64(0)
    try:
        L.msm_device_info(buf, 256, C.byref(cus), C.byref(mem))
        return "%s (%d CUs)" % (buf.value.decode(), cus.value)
    except Exception:
        return "unknown device"


if __name__ == "__main__":
    main()
