"""The tICA accumulation dispatch, restated in Python from the host code as it stood before it had a plan (one function,
tica_accumulate_device, that derived a dozen path flags inline, and msm_tica_create): what the library's tica_plan
(csrc/tica_plan.h, asked through msm_tica_plan / msm_tica_last_plan) is held to.  Nothing here is derived from tica_plan.h.

geometry() restates msm_tica_create for given resident slots; plan() restates a launch of whole trajectories (or of segments) and returns
the fields of msm_tica_plan's out array, in order."""
import ctypes

import numpy as np

F32, F64, BF16, BF16X2 = 0, 1, 2, 3
TM, BK32, BK64, KCMAX, KFLUSH_SYM = 128, 32, 16, 4096, 4096
PATHS = ("none", "cg64", "cg32", "sym", "symw", "symw64", "img_ring", "img_fused")          # MSM_TICA_PATH_*
FL_EDGE, FL_ALIGNED, FL_FOLD, FL_REM, FL_VEC, FL_X2 = 1, 2, 4, 8, 16, 32                    # MSM_TICA_FL_*
GEOM_FIELDS = ("F", "lag", "mode", "T", "ntiles", "S32", "S64", "sym", "ntiles_sym", "sym_cohorts", "sym_grid", "S_sym", "symw",
               "symw_var", "symw_KS", "symw_S", "symw64", "symw_S64", "img_on", "T2", "ntile2", "S_img", "img_grid", "have_fold",
               "shift_on")
PLAN_FIELDS = ("path", "flavour", "bk", "S", "G", "symrem", "kc", "rem_R", "rem_rounds", "pairsem", "shifted", "fold", "kflush",
               "pace", "single", "total", "nvalid")
# whole-matrix variants by width: (widest F, variant id, frames per K-step)
SYMW_CHAIN = ((16, 0, 64), (32, 1, 32), (64, 2, 64), (96, 6, 32), (128, 3, 32), (160, 7, 16), (192, 4, 16), (256, 5, 16))
BALANCE_SIZES = (4096, 3072, 2560, 2048, 1536, 1024)


def cdiv(a, b):
    return -(-a // b)


def geometry(F, lag, mode, slots, cus=256, sym_env=None, symw_env=None, symw64_env=None, shift_on=1):
    """msm_tica_create with `slots` resident workgroups of every kernel flavour on `cus` compute units."""
    g = dict.fromkeys(GEOM_FIELDS, 0)
    T = cdiv(F, TM)
    g.update(F=F, lag=lag, mode=mode, T=T, ntiles=T * T + T * (T + 1) // 2, shift_on=shift_on)
    g["S32"] = max(1, slots // g["ntiles"])
    g["S64"] = max(1, slots // g["ntiles"])
    sym_off, symw_off = sym_env == 0, symw_env == 0
    if mode == F32 and not (sym_off or symw_off) and F <= 256:
        _, g["symw_var"], g["symw_KS"] = next(c for c in SYMW_CHAIN if F <= c[0])
        g.update(symw=1, sym=1, symw_S=slots)
        if F <= 128 and symw64_env != 0:
            g.update(symw64=1, symw_S64=slots)
    if not g["symw"]:
        nts = g["ntiles_sym"] = T * (T + 1) // 2
        if mode == F32 and not sym_off and 2 <= T <= 64 and F % 4 == 0:
            g["sym_cohorts"] = slots // nts
            g["sym"] = int(g["sym_cohorts"] >= 1)
            R = slots - g["sym_cohorts"] * nts
            rem = bool(g["sym"]) and R * 16 >= slots and 3 * R >= nts
            g["sym_grid"] = slots if rem else g["sym_cohorts"] * nts
            g["S_sym"] = g["sym_cohorts"] + int(rem)
    g["T2"] = cdiv(F, 256)
    g["ntile2"] = g["T2"] * (g["T2"] + 1)
    if mode in (BF16, BF16X2) and g["ntile2"] <= cus:
        g["img_on"] = 1
        g["img_grid"] = max(cus, g["ntile2"])
        g["S_img"] = g["img_grid"] // g["ntile2"]
        g.update(sym=1, S_sym=g["S_img"] + 1, sym_cohorts=g["S_img"])
    g["have_fold"] = g["sym"]                      # the fold storage is allocated with `sym`
    return g


def _balance(n_rows, lag, S, bk):
    best, best_kc = -1, KCMAX
    for cand in BALANCE_SIZES:
        sizes = []
        for own in n_rows:
            if own <= lag:
                continue
            piece = cdiv(cdiv(own, cdiv(own, cand)), bk) * bk
            k = cdiv(own, piece)
            sizes.append(np.full(k, piece + 16, dtype=np.int64))
            sizes[-1][-1] = own - (k - 1) * piece + 16
        sizes = np.concatenate(sizes)
        load = np.zeros(S, dtype=np.int64)
        np.add.at(load, np.arange(len(sizes)) % S, sizes)
        worst = int(load.max())
        if best < 0 or worst < best:
            best, best_kc = worst, cand
    return best_kc


def plan(g, dtype_bytes, ld, n_rows, ptr16=True, dims4=None, fold_env=None, fused_env=None, ptr16_all=None, segs=None):
    """A launch of whole trajectories, or -- segs: a list of (len, own_begin, own_end) -- of segments.  ptr16: every
    trajectory longer than the lag starts on a 16-byte boundary; ptr16_all: the skipped ones do too (default: as ptr16)."""
    F, lag, mode = g["F"], g["lag"], g["mode"]
    if dims4 is None:
        dims4 = F % 4 == 0 and ld % 4 == 0
    if ptr16_all is None:
        ptr16_all = ptr16
    if segs is not None:
        owned = [oe - ob for n, ob, oe in segs if n > lag and oe > ob]      # the frames a launch owns of each valid segment
    else:
        owned = [n for n in n_rows if n > lag]
    total, nvalid = sum(owned), len(owned)
    out = dict.fromkeys(PLAN_FIELDS, 0)
    out.update(total=total, nvalid=nvalid)
    if nvalid == 0:
        return tuple(out[k] for k in PLAN_FIELDS)
    aligned = dims4 and ptr16
    slabs_sym = bool(g["sym"]) and not g["symw"]          # the sum/difference slabs are allocated for these handles
    bfmode = mode in (BF16, BF16X2)
    useimg = bfmode and bool(g["img_on"]) and dtype_bytes in (2, 4)
    usefused = False
    if useimg and dtype_bytes == 2 and F % 256 == 0 and ld % 8 == 0:
        usefused = (fused_env == 1) if fused_env is not None else F <= 512
        usefused = usefused and ptr16_all         # (every pointer of the table, skipped trajectories included)
    use32 = dtype_bytes == 4 and (mode == F32 or (bfmode and not useimg))
    symw64 = dtype_bytes == 8 and mode == F32 and bool(g["symw64"])
    usesymw = (use32 and mode == F32 and bool(g["symw"])) or symw64
    bk = g["symw_KS"] if usesymw else BK32 if (use32 or useimg) else BK64
    usesym = (not usesymw) and ((use32 and mode == F32 and bool(g["sym"]) and slabs_sym and aligned) or useimg)
    pairsem = usesym or usesymw
    if symw64:
        S = min(g["symw_S"], g["symw_S64"])
    elif usesymw:
        S = g["symw_S"]
    elif useimg:
        S = g["S_img"]
    elif usesym:
        S = g["sym_cohorts"]
    else:
        S = g["S32"] if use32 else g["S64"]
    symrem = usesym and not useimg and g["sym_grid"] > S * g["ntiles_sym"]
    G = S if usesymw else g["sym_grid"] if symrem else S * (g["ntiles_sym"] if usesym else g["ntiles"])
    kc = cdiv(cdiv(total, S), bk) * bk
    kc = min(kc, KCMAX)
    if useimg and kc > 1024:
        kc = 1024
    kc = max(kc, bk)
    if usesymw:
        kmin = min(KCMAX, max(256, 4 * bk))
        kc = cdiv(cdiv(total, 8 * S), bk) * bk
        kc = min(KCMAX, max(kc, kmin))
    if kc == KCMAX and total < 16 * KCMAX * S and not useimg and not usesymw:
        kc = _balance(owned, lag if segs is None else 0, S, bk)
    single = nvalid == 1 and len(n_rows) == 1 and segs is None and not useimg
    kflush = 2 * KFLUSH_SYM if g["shift_on"] else KFLUSH_SYM
    pace = usesym and not useimg
    rem_R = rem_rounds = 0
    if symrem:
        rem_R = G - S * g["ntiles_sym"]
        rem_rounds = cdiv(g["ntiles_sym"], rem_R)
    fold = False
    if usesym and segs is None and g["have_fold"] and not usefused and (useimg or F % TM == 0):
        fmode = 1 if fold_env is None else fold_env
        fold = fmode != 0 and (fmode == 2 or total * F >= 67108864)
        if any(lag < n < 2 * lag for n in n_rows):
            fold = False
        if 2 * lag * nvalid > total // 4:
            fold = False
    shifted = bool(g["shift_on"]) and (use32 or useimg or symw64)
    x2 = mode == BF16X2
    if usefused or useimg:
        path = "img_fused" if usefused else "img_ring"
        flavour = (FL_X2 if x2 else 0) | (FL_FOLD if fold else 0)
    elif usesymw:
        path = "symw64" if symw64 else "symw"
        flavour = FL_VEC if F >= (2 if symw64 else 4) else 0
    elif usesym:
        path = "sym"
        flavour = (FL_REM if symrem else 0) | (FL_FOLD if fold else 0 if F % TM == 0 else FL_EDGE)
    elif use32:
        path = "cg32"
        flavour = (FL_ALIGNED if F % TM == 0 else FL_ALIGNED | FL_EDGE) if aligned else FL_EDGE
    else:
        path, flavour = "cg64", 0
    out.update(path=PATHS.index(path), flavour=flavour, bk=bk, S=S, G=G, symrem=int(symrem), kc=kc, rem_R=rem_R, rem_rounds=rem_rounds,
               pairsem=int(pairsem), shifted=int(shifted), fold=int(fold), kflush=kflush, pace=int(pace), single=int(single))
    return tuple(out[k] for k in PLAN_FIELDS)


def n_main(p, nchunks):
    """Chunks of the whole cohorts when the launch has a remainder cohort (p: a plan as a dict)."""
    if not p["symrem"]:
        return nchunks
    d = p["S"] * p["rem_rounds"] + 1
    return nchunks - (nchunks + d // 2) // d


def library_plan(g, dtype_bytes, ld, n_rows, ptr16=True, dims4=None, fold_env=None, fused_env=None, ptr16_all=None):
    """The same launch as the library's tica_plan decides it (msm_tica_plan: needs no device)."""
    from msmbuilder_amd import _lib
    if dims4 is None:
        dims4 = g["F"] % 4 == 0 and ld % 4 == 0
    geom = (ctypes.c_int * len(GEOM_FIELDS))(*[int(g[k]) for k in GEOM_FIELDS])
    rows = (ctypes.c_int64 * max(1, len(n_rows)))(*n_rows)
    out = (ctypes.c_longlong * len(PLAN_FIELDS))()
    ptr16_all = ptr16 if ptr16_all is None else ptr16_all
    _lib.check(_lib.lib().msm_tica_plan(geom, dtype_bytes, ld, rows, len(n_rows), int(ptr16) | 2 * int(ptr16_all), int(dims4),
                                        -1 if fold_env is None else fold_env, -1 if fused_env is None else fused_env, out))
    return tuple(out)


def last_plan(handle):
    """(geometry dict, plan tuple, chunks, super-chunks) of a handle's most recent accumulate."""
    from msmbuilder_amd import _lib
    out = (ctypes.c_longlong * (len(GEOM_FIELDS) + len(PLAN_FIELDS) + 2))()
    _lib.check(_lib.lib().msm_tica_last_plan(handle, out))
    v = list(out)
    ng, npl = len(GEOM_FIELDS), len(PLAN_FIELDS)
    return dict(zip(GEOM_FIELDS, v[:ng])), tuple(v[ng:ng + npl]), v[ng + npl], v[ng + npl + 1]
