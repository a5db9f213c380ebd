"""K-centers pass chains at the sizes where their grids differ (csrc/kcenters.hip kcenters_impl).

Every pass of a fit writes one KcPartial (best distance, row) per workgroup into one of two arrays of the partials
buffer, and the next pass reads all of them to choose its centre.  The passes run on grids of different sizes (DT = 256
rows per tile, C = the device's compute units, read from torch, not assumed):

- plain pass: nblk0 = min(ceil(n / DT), KC_MAXBLK = 1024); rows that take the wide streaming kernel (wide_ok: 16-byte
  aligned, row length a multiple of 16 bytes, more than 32 float32 / 16 float64 features) cut it to nblk = min(nblk0, 2 C);
- wide screened pass, one centre per pass: gpass = min(ceil(n / (kr DT)), nblk0), kr = 8 / 4 / 2 rows per thread
  (kr = 4 up to 64 features, 2 beyond; the row count of the byte copy decides, whatever the type);
- wide batched pass: gp2, the same formula.

The sizes below sit on both sides of each relation between those grids:

- T1: ceil(n / DT) against 2 C, where the wide grid fills (131,072 rows at C = 256): "T1-" 2 C DT - 2,000 and "T1+"
  2 C DT + 5,000;
- T2: ceil(n / DT) against KC_MAXBLK, where nblk0 reaches its cap (262,144 rows): "T2-" and "T2+" (-3,000 / +9,000);
- T3: gpass / gp2 against nblk.  For kr = 2 it coincides with T2 at C = 256 (T2+ has gpass = 530 > nblk = 512);
  for kr = 4, "T3k4-" / "T3k4+" = 2 C 4 DT -/+ 3,000 (524,288 at C = 256).  "T3k2=" (524,088 rows) and "T3k4="
  (1,048,376 rows) have gpass = gp2 = nblk0 = 1024 -- twice the plain grid.

Paths (each case asserts through msm_kcenters_last_stats / msm_kcenters_last_batch_fallbacks that it ran the path meant):
wide one centre per screened pass (default for rows over 1 KiB; MSM_KC_WBATCH=0 below that), wide batched with the
selector on several workgroups (default up to 1 KiB) and on one (MSM_KC_WSELECT=1), plain passes on the cut grid
(cityblock / chebyshev on wide_ok rows), the same sizes with wide_ok false (rows at an address offset by one element:
grids uncut; rows of m % 4 != 0 do NOT give that -- the fit pads them to an aligned copy), and the narrow float64 screen
(one centre per pass and batched against each other).

Every case is checked three ways: against another path on the same rows (the plain passes, MSM_KC_WSCREEN=0, whose
arrays always hold the same count; the plain metrics against the uncut grid; the narrow screen's two modes), bit for bit;
against an fp64 recomputation in torch from the fit's ids (distances_ within 1e-12 of the running minimum, labels_ the
argmin with the lowest index on ties, each centre the farthest row of the centres before it, within 1e-12 -- the
difference u - v of float32 rows is rounded to float32 before it is widened, as the reference's kernels do); and, up to
5e8 row x feature x centre terms, against the C oracle bit for bit.

The 512- and 1,280-feature default cases place 9 far outliers (far from the bulk and from each other) in rows 0-255.
Those rows are tile 0, which block 0 of the plain passes handles (distance_wide_dev.h), so the first centres are
outliers and the argmax the first screened pass reads lies in prev[0] -- the slot a workgroup b = nblk of that pass
overwrote when the two partial arrays were nblk apart for the plain passes and the pass wrote gpass > nblk entries:
a workgroup that started after it chose another centre.  (Fixed: both arrays are nblk0 apart for every pass.)  Whether
a late workgroup starts after workgroup nblk has finished depends on the order in which workgroups finish, so these
cases make a wrong result certain when that happens, not the happening itself.
"""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 256
KC_MAXBLK = 1024
KNOBS = ("MSM_KC_WBATCH", "MSM_KC_WSCREEN", "MSM_KC_WSELECT", "MSM_KC_BATCH")
ORACLE_TERMS = 500_000_000
OUTLIER_ROWS = [7 + 27 * j for j in range(9)]   # all in tile 0 (rows 0-255)


def _n(size):
    import torch
    c2 = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    return {"T1-": c2 * DT - 2_000, "T1+": c2 * DT + 5_000,
            "T2-": KC_MAXBLK * DT - 3_000, "T2+": KC_MAXBLK * DT + 9_000,
            "T3k4-": c2 * 4 * DT - 3_000, "T3k4+": c2 * 4 * DT + 3_000,
            "T3k2=": KC_MAXBLK * 2 * DT - 200, "T3k4=": KC_MAXBLK * 4 * DT - 200}[size]


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _rows(n, m, dtype, seed, outliers=False, offset=False):
    """n x m rows around 12 hubs, generated on the device in slices (no full-size temporaries); `offset`: the rows start
    one element past a 16-byte boundary (wide_ok false, nothing padded)."""
    import torch
    td = torch.float32 if dtype == np.float32 else torch.float64
    g = torch.Generator(device="cuda").manual_seed(seed)
    if offset:
        X = torch.empty(n * m + 1, dtype=td, device="cuda")[1:].view(n, m)
        assert X.data_ptr() % 16 != 0
    else:
        X = torch.empty(n, m, dtype=td, device="cuda")
    hubs = torch.randn(12, m, generator=g, device="cuda") * 2.0
    for s in range(0, n, 65_536):
        e = min(n, s + 65_536)
        X[s:e] = hubs[torch.randint(0, 12, (e - s,), generator=g, device="cuda")] + torch.randn(e - s, m, generator=g, device="cuda")
    if outliers:
        for r in OUTLIER_ROWS:
            X[r] = torch.randn(m, generator=g, device="cuda") * 30.0
    return X


def _fit(monkeypatch, X, k, metric="euclidean", env=None):
    from msmbuilder_amd import KCenters, _lib
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    kc = KCenters(n_clusters=k, metric=metric, random_state=3).fit([X])
    st = (C.c_int64 * 5)()
    fb = (C.c_int64 * 1)()
    _lib.check(_lib.lib().msm_kcenters_last_stats(st))
    _lib.check(_lib.lib().msm_kcenters_last_batch_fallbacks(fb))
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    return dict(kc=kc, ids=list(kc.cluster_ids_), labels=kc.labels_[0], dist=kc.distances_[0], inertia=kc.inertia_,
                st=list(st), fb=int(fb[0]))


def _assert_path(r, path, k):
    """The pass counts of msm_kcenters_last_stats: st[1] plain passes, st[2] screened passes (rounds when batched)."""
    st, fb = r["st"], r["fb"]
    if path == "wide1":     # four plain passes, then one centre per screened pass
        assert st[1] == 4 and st[2] == k - 4 and fb == 0, (st, fb)
    elif path == "wbatch":  # four plain passes, then rounds of several centres (fewer rounds than centres)
        assert st[1] == 4 and 0 < st[2] < k - 4 and fb < st[2], (st, fb)
    elif path == "plain":
        assert st[1] == k and st[2] == 0, (st, fb)
    elif path == "narrow1":
        assert st[1] == 4 and st[2] == k - 4 and fb == 0, (st, fb)
    elif path == "nbatch":  # two plain passes, then rounds of several centres
        assert st[1] == 2 and 0 < st[2] < k - 2 and fb < st[2], (st, fb)
    else:
        raise AssertionError(path)


def _assert_same(a, b, same_grid=True):
    """Bit-equal fits.  inertia_ is the device's tree sum over the plain grid's blocks: on grids of different sizes
    only its value, not its rounding, is the same."""
    assert a["ids"] == b["ids"]
    assert np.array_equal(a["labels"].cpu().numpy(), b["labels"].cpu().numpy())
    assert np.array_equal(a["dist"].cpu().numpy(), b["dist"].cpu().numpy(), equal_nan=True)
    if same_grid:
        assert a["inertia"] == b["inertia"] or (np.isnan(a["inertia"]) and np.isnan(b["inertia"]))
    else:
        tot = float(np.sum(a["dist"].cpu().numpy()))
        assert abs(a["inertia"] - tot) <= 1e-12 * tot and abs(b["inertia"] - tot) <= 1e-12 * tot


def _metric_rows(xb, c, metric):
    """fp64 distances of the rows xb to the row c; the elementwise difference in the rows' own type (float32 rows:
    rounded to float32, then widened -- the reference's arithmetic), everything after it in float64."""
    import torch
    d = xb - c
    if metric == "euclidean":
        return d.double().square_().sum(1).sqrt_()
    if metric == "cityblock":
        return d.abs_().double().sum(1)
    if metric == "chebyshev":
        return d.abs_().amax(1).double()
    raise AssertionError(metric)


def _assert_fp64_reference(X, r, metric="euclidean"):
    """Recompute every row's distance to every centre of the fit's ids in float64 (row slices of at most 2^25
    elements: < 1 GB of scratch) and check distances_, labels_ and the greedy choice of every centre."""
    import torch
    n, m = X.shape
    ids, k = r["ids"], len(r["ids"])
    assert len(set(ids)) == k
    exact = metric == "chebyshev"   # (a maximum of widened float32 values: no rounding anywhere)
    tol = 0.0 if exact else 1e-12
    labels, dist = r["labels"], r["dist"]
    cen = X[torch.tensor(ids, device=X.device)]
    dev = X.device
    far = torch.zeros(k, dtype=torch.float64, device=dev)               # max_i d_{k-1}[i]
    at_id = torch.full((k,), -1.0, dtype=torch.float64, device=dev)     # d_{k-1}[ids[k]]
    bad_dist = torch.zeros((), dtype=torch.int64, device=dev)
    bad_lab = torch.zeros((), dtype=torch.int64, device=dev)
    near_ties = torch.zeros((), dtype=torch.int64, device=dev)
    rows = max(1, (1 << 25) // m)
    for s in range(0, n, rows):
        e = min(n, s + rows)
        xb = X[s:e]
        run = torch.full((e - s,), float("inf"), dtype=torch.float64, device=dev)
        second = run.clone()
        arg = torch.zeros(e - s, dtype=torch.int64, device=dev)
        for j in range(k):
            if j >= 1:
                far[j] = torch.maximum(far[j], run.max())
                if s <= ids[j] < e:
                    at_id[j] = run[ids[j] - s]
            d = _metric_rows(xb, cen[j], metric)
            lt = d < run                                            # strict: the lowest centre index wins a tie
            second = torch.where(lt, run, torch.minimum(second, d))
            arg = torch.where(lt, j, arg)
            run = torch.where(lt, d, run)
        bad_dist += ((dist[s:e] - run).abs() > tol * run).sum()
        tie = (second - run) <= 1e-12 * run if not exact else torch.zeros_like(lt)
        near_ties += tie.sum()
        bad_lab += ((labels[s:e] != arg) & ~tie).sum()
    assert int(bad_dist) == 0, "distances_ off the fp64 running minimum in %d rows" % int(bad_dist)
    assert int(bad_lab) == 0, "labels_ not the argmin in %d rows" % int(bad_lab)
    assert int(near_ties) <= 16, int(near_ties)
    far, at_id = far.cpu().numpy(), at_id.cpu().numpy()
    short = [j for j in range(1, k) if not at_id[j] >= far[j] * (1.0 - tol)]
    assert not short, "centres %s are not the farthest row (d %s < max %s)" % (short, at_id[short], far[short])


def _assert_oracle(X, r, k, metric="euclidean"):
    from oracle.libdistance_oracle import Oracle
    n, m = X.shape
    assert n * m * k <= ORACLE_TERMS
    ids, labels, dist = Oracle().kcenters_fit(X.cpu().numpy(), k, metric, r["ids"][0])
    assert r["ids"] == list(ids)
    assert np.array_equal(r["labels"].cpu().numpy(), labels)
    assert np.array_equal(r["dist"].cpu().numpy(), dist)


_F32, _F64 = np.float32, np.float64
# (path, knobs, dtype, features, size, K, flags): o = outliers in tile 0, x = rows offset by one element (wide_ok false),
# c = the C oracle too
CASES = [
    # one centre per screened pass, default (rows over 1 KiB)
    ("wide1", {}, _F32, 260, "T1-", 24, ""),
    ("wide1", {}, _F32, 260, "T2+", 24, ""),
    ("wide1", {}, _F32, 512, "T3k2=", 30, "o"),
    ("wide1", {}, _F32, 512, "T3k2=", 30, "ox"),
    ("wide1", {}, _F32, 1280, "T1+", 24, ""),
    ("wide1", {}, _F32, 1280, "T3k2=", 30, "o"),
    ("wide1", {}, _F64, 130, "T2-", 24, ""),
    ("wide1", {}, _F64, 130, "T2+", 24, ""),
    ("wide1", {}, _F64, 200, "T3k2=", 24, ""),
    # one centre per screened pass, forced
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F32, 36, "T1+", 24, "c"),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F32, 36, "T3k4=", 24, ""),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F32, 64, "T3k4-", 24, ""),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F32, 64, "T3k4+", 24, ""),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F32, 100, "T3k2=", 24, ""),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F64, 18, "T3k4=", 24, ""),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F64, 40, "T2+", 24, "c"),
    ("wide1", {"MSM_KC_WBATCH": "0"}, _F64, 40, "T2+", 24, "xc"),
    # batched, selector on several workgroups (default up to 1 KiB)
    ("wbatch", {}, _F32, 36, "T3k4=", 24, ""),
    ("wbatch", {}, _F32, 36, "T3k4=", 24, "x"),
    ("wbatch", {}, _F32, 128, "T1-", 24, ""),
    ("wbatch", {}, _F32, 128, "T2+", 24, ""),
    ("wbatch", {}, _F32, 256, "T3k2=", 24, ""),
    ("wbatch", {}, _F64, 18, "T1+", 24, "c"),
    ("wbatch", {}, _F64, 100, "T2+", 24, ""),
    # batched, selector on one workgroup
    ("wbatch", {"MSM_KC_WSELECT": "1"}, _F32, 64, "T3k4+", 24, ""),
    ("wbatch", {"MSM_KC_WSELECT": "1"}, _F64, 40, "T2+", 24, "c"),
]


def _case_id(c):
    path, env, dtype, m, size, k, flags = c
    knob = "".join("-%s=%s" % (key[7:].lower(), v) for key, v in env.items())
    return "%s%s-%s-%d-%s%s" % (path, knob, np.dtype(dtype).name, m, size, ("-" + flags) if flags else "")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_wide_paths_at_grid_sizes(gpu, monkeypatch, case):
    """A wide screened path at one size of the grid relations: bit-equal to the plain passes on the same rows, the fp64
    recomputation, and (flag c) the C oracle."""
    path, env, dtype, m, size, k, flags = case
    n = _n(size)
    X = _rows(n, m, dtype, seed=m * 7 + k, outliers="o" in flags, offset="x" in flags)
    a = _fit(monkeypatch, X, k, env=env)
    _assert_path(a, path, k)
    b = _fit(monkeypatch, X, k, env={"MSM_KC_WSCREEN": "0"})
    _assert_path(b, "plain", k)
    _assert_same(a, b)
    if "o" in flags:
        assert set(OUTLIER_ROWS) <= set(a["ids"][:len(OUTLIER_ROWS) + 1])   # the data does what the docstring says
    _assert_fp64_reference(X, a)
    if "c" in flags:
        _assert_oracle(X, a, k)


@pytest.mark.parametrize("metric", ["cityblock", "chebyshev"])
def test_plain_passes_on_the_cut_grid(gpu, monkeypatch, metric):
    """Plain passes only (no screen for these metrics) on wide_ok rows past T2: nblk = 2 C of nblk0 = 1024 partial
    slots; the same values at an offset address run the uncut grid of the other kernel."""
    n, m, k = _n("T2+"), 64, 20
    X = _rows(n, m, _F32, seed=11)
    a = _fit(monkeypatch, X, k, metric)
    _assert_path(a, "plain", k)
    Xo = _rows(n, m, _F32, seed=11, offset=True)
    assert bool((Xo == X).all())
    b = _fit(monkeypatch, Xo, k, metric)
    _assert_path(b, "plain", k)
    _assert_same(a, b, same_grid=False)
    _assert_fp64_reference(X, a, metric)
    _assert_oracle(X, a, k, metric)


def test_narrow_float64_screen_past_t2(gpu, monkeypatch):
    """The register-resident float64 screen (10 features: no wide path) just past T2: one centre per pass
    (MSM_KC_BATCH=0) and batched give the same fit, the fp64 recomputation's and the oracle's."""
    n, m, k = _n("T2+"), 10, 30
    X = _rows(n, m, _F64, seed=5)
    a = _fit(monkeypatch, X, k, env={"MSM_KC_BATCH": "0"})
    _assert_path(a, "narrow1", k)
    b = _fit(monkeypatch, X, k)
    _assert_path(b, "nbatch", k)
    _assert_same(a, b)
    _assert_fp64_reference(X, a)
    _assert_oracle(X, a, k)


@pytest.mark.parametrize("size,m,oracle", [("T1+", 1280, False), ("T2+", 64, True)])
def test_predict_on_the_fit_rows(gpu, monkeypatch, size, m, oracle):
    """KCenters.predict on the rows of the fit gives labels_; past T2 libdistance.assign_nearest also gives the oracle's
    labels and, within 1e-13, its inertia."""
    from msmbuilder_amd import libdistance
    n, k = _n(size), 24
    X = _rows(n, m, _F32, seed=m + 1)
    a = _fit(monkeypatch, X, k)
    _assert_path(a, "wide1" if m * 4 > 1024 else "wbatch", k)
    lab = a["kc"].predict([X])[0]
    assert np.array_equal(np.asarray(lab.cpu().numpy() if hasattr(lab, "cpu") else lab), a["labels"].cpu().numpy())
    if oracle:
        from oracle.libdistance_oracle import Oracle
        cen = a["kc"].cluster_centers_
        lab_g, inertia_g = libdistance.assign_nearest(X, cen, "euclidean")
        lab_o, inertia_o = Oracle().assign_nearest(X.cpu().numpy(), cen, "euclidean")
        assert np.array_equal(lab_g.cpu().numpy(), lab_o)
        assert abs(inertia_g - inertia_o) <= 1e-13 * abs(inertia_o)
