"""Butterworth, EWMA and DoubleEWMA on the device (msm_ts_filter) against the long-double restatement of
tests/timeseries_ref.py, under the tolerances that module derives and test_timeseries_ref.py measures on the CPU:

* Butterworth: MARGIN x scipy's own error on the same input + ULPS ulp of the output's type, at the output's scale;
* EWMA: ((2 / alpha + 1) + 2 seams) eps max|x| per element.

MSM_TS_SEGMENT=64 puts seams into trajectories of a few hundred frames: lengths of width, 63, 64, 65, 129 and 3 * 64 + 1
frames (1 for the EWMA kinds) in ragged lists; the 20,000-frame inputs run at the library's own segment.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeseries_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = R.LENGTHS


@pytest.fixture(scope="module")
def TS(gpu):
    from msmbuilder_amd import preprocessing, timeseries
    assert preprocessing.Butterworth is timeseries.Butterworth and preprocessing.DoubleEWMA is timeseries.DoubleEWMA
    return timeseries


def place(X, how):
    import torch
    if how == "host":
        return X
    if how == "device":
        return torch.tensor(X, device="cuda")
    buf = torch.full((X.shape[0], X.shape[1] + 5), float("nan"), dtype=torch.tensor(X[:0]).dtype, device="cuda")
    buf[:, :X.shape[1]] = torch.tensor(X, device="cuda")
    view = buf[:, :X.shape[1]]
    assert X.shape[0] < 2 or not view.is_contiguous()
    return view


def host(y):
    return y if isinstance(y, np.ndarray) else y.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def bw_reference(name, n, F, width, order, dt):
    """(input, long-double reference, scipy's own relative error) of one trajectory; computed once, never written to."""
    X = R.case_input(name, n, F, np.dtype(dt))
    ref = R.butterworth(X.astype(np.float64), width, order)
    e_s = R.relerr(R.scipy_butterworth(X, width, order), ref)
    for a in (X, ref):
        a.setflags(write=False)
    return X, ref, e_s


def assert_butterworth(out, X, ref, e_s, what):
    out = host(out)
    assert out.dtype == X.dtype and out.shape == X.shape
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(out.astype(np.longdouble) - ref)))
    tol = R.butterworth_bound(e_s, scale, out.dtype)
    print("%s: error %.3e of scale, scipy %.3e, bound %.3e" % (what, err / scale, e_s, tol / scale))
    assert err <= tol, what


# ---- Butterworth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("case", [c for c in R.BW_CASES if c[4] == 64], ids=lambda c: c[0])
def test_butterworth_seams_in_ragged_lists(TS, monkeypatch, case, dt):
    name, width, order, n_max, seg = case
    lengths = R.bw_case_lengths(case)
    refs = [bw_reference(name, n, 3, width, order, dt) for n in lengths]
    est = TS.Butterworth(width=width, order=order)
    seqs = [place(r[0], "device") for r in refs]
    monkeypatch.setenv("MSM_TS_SEGMENT", "64")
    outs = est.transform(seqs)
    for n, o, (X, ref, e_s) in zip(lengths, outs, refs):
        assert_butterworth(o, X, ref, e_s, "%s %s n=%d segment 64" % (name, dt, n))
    assert all(same_bits(a, b) for a, b in zip(outs, est.fit_transform(seqs)))                     # run to run
    assert all(same_bits(a, est.partial_transform(s)) for a, s in zip(outs, seqs))                # list == one by one
    monkeypatch.setenv("MSM_TS_SEGMENT", "0")
    ones = est.transform(seqs)
    for n, o1, o, (X, ref, e_s) in zip(lengths, ones, outs, refs):
        assert_butterworth(o1, X, ref, e_s, "%s %s n=%d one segment" % (name, dt, n))
        gap = float(np.max(np.abs(host(o1).astype(np.float64) - host(o).astype(np.float64))))
        assert gap <= 2 * R.butterworth_bound(e_s, float(np.max(np.abs(ref))), X.dtype)


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("case", [c for c in R.BW_CASES if c[4] is None], ids=lambda c: c[0])
def test_butterworth_at_the_library_segment(TS, monkeypatch, case, dt):
    name, width, order, n, seg = case
    monkeypatch.delenv("MSM_TS_SEGMENT", raising=False)
    X, ref, e_s = bw_reference(name, n, 3, width, order, dt)
    est = TS.Butterworth(width=width, order=order)
    S = TS._segment_for(est._denom, n + 2 * (est.width - 1) + 6 * (order + 1))
    assert (S == 0) == name.endswith("_single")
    out = est.partial_transform(place(X, "device"))
    assert_butterworth(out, X, ref, e_s, "%s %s segment %d" % (name, dt, S))
    assert same_bits(out, est.partial_transform(place(X, "device")))
    monkeypatch.setenv("MSM_TS_SEGMENT", "0")
    assert_butterworth(est.partial_transform(X), X, ref, e_s, "%s %s one segment, host rows" % (name, dt))


@pytest.mark.parametrize("how,dt", [("host", "float32"), ("device", "float64"), ("pitched", "float32"), ("pitched", "float64")])
@pytest.mark.parametrize("F", [1, 3, 4, 33, 257, 1100])
def test_every_width_of_rows_and_every_placement(TS, monkeypatch, F, how, dt):
    monkeypatch.setenv("MSM_TS_SEGMENT", "64")
    refs = [bw_reference("rows", n, F, 5, 3, dt) for n in (5, 65, 193)]
    seqs = [place(r[0], how) for r in refs]
    outs = TS.Butterworth(width=5, order=3).transform(seqs)
    for s, o, (X, ref, e_s) in zip(seqs, outs, refs):
        assert isinstance(o, np.ndarray) == (how == "host") and (how == "host" or o.is_cuda)
        assert_butterworth(o, X, ref, e_s, "F=%d %s %s n=%d" % (F, how, dt, len(X)))
    alpha = R.ewm_alpha(span=20)
    for cls, fn in ((TS.EWMA, R.ewma), (TS.DoubleEWMA, R.double_ewma)):
        outs = cls(span=20, min_periods=3).transform(seqs)
        for o, (X, _, _) in zip(outs, refs):
            assert isinstance(o, np.ndarray) == (how == "host")
            assert_ewma(o, np.asarray(fn(X.astype(np.float64), alpha, True, 3)), X, alpha, 64, "F=%d %s %s %s" % (F, how, dt, cls.__name__))
    if how == "pitched":   # nothing was written between the rows
        assert all(bool(s._base[:, F:].isnan().all()) for s in seqs)


def test_butterworth_nan_or_inf_column_comes_out_all_nan(TS, monkeypatch):
    X, ref, e_s = bw_reference("nan", 193, 4, 5, 3, "float64")
    est = TS.Butterworth(width=5, order=3)
    for seg in ("64", "0"):
        monkeypatch.setenv("MSM_TS_SEGMENT", seg)
        clean = host(est.partial_transform(place(X, "device")))
        for v, row in ((np.nan, 0), (np.nan, 100), (np.inf, 192), (-np.inf, 64)):
            bad = X.copy()
            bad[row, 2] = v
            out = host(est.partial_transform(place(bad, "device")))
            assert np.isnan(out[:, 2]).all()
            assert same_bits(out[:, [0, 1, 3]], clean[:, [0, 1, 3]])


# ---- EWMA -------------------------------------------------------------------------------------------------------------------
def assert_ewma(out, ref, X, alpha, S, what):
    out = host(out)
    assert out.dtype == np.float64 and out.shape == X.shape
    live = ~np.isnan(ref.astype(np.float64))
    assert np.array_equal(~np.isnan(out), live), what
    seams = -(-len(X) // S) - 1 if S else 0
    xmax = np.abs(X).max(0).astype(np.float64)
    err = np.where(live, np.abs(out.astype(np.longdouble) - ref), 0).max(0, initial=0.0).astype(np.float64) if len(X) else np.zeros(X.shape[1])
    tol = R.ewma_bound(alpha, seams, xmax)
    print("%s: largest error / bound %.3f (%d seams)" % (what, float(np.max(err / tol, initial=0.0)), seams))
    assert (err <= tol).all(), what


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("double", [False, True], ids=["EWMA", "DoubleEWMA"])
@pytest.mark.parametrize("case", R.EW_CASES, ids=lambda c: c[0])
def test_ewma(TS, monkeypatch, case, double, dt):
    name, kw, adjust, mp, n_max, seg = case
    alpha = R.ewm_alpha(**kw)
    est = (TS.DoubleEWMA if double else TS.EWMA)(min_periods=mp, adjust=adjust, **kw)
    fn = R.double_ewma if double else R.ewma
    if seg is None:
        monkeypatch.delenv("MSM_TS_SEGMENT", raising=False)
        lengths = [n_max]
        S = TS._segment_for([1.0, -(1.0 - alpha)], n_max)
        assert S and n_max // S >= 2
    else:
        monkeypatch.setenv("MSM_TS_SEGMENT", str(seg))
        lengths, S = [1] + list(LENGTHS), seg
    Xs = [R.case_input(name, n, 3, np.dtype(dt)) for n in lengths]
    refs = [np.asarray(fn(X.astype(np.float64), alpha, adjust, mp)) for X in Xs]
    seqs = [place(X, "device") for X in Xs]
    outs = est.transform(seqs)
    for X, o, ref in zip(Xs, outs, refs):
        assert_ewma(o, ref, X, alpha, S, "%s %s n=%d" % (name, dt, len(X)))
    assert all(same_bits(a, b) for a, b in zip(outs, est.transform(seqs)))
    assert all(same_bits(a, est.partial_transform(s)) for a, s in zip(outs, seqs))
    monkeypatch.setenv("MSM_TS_SEGMENT", "0")
    for X, o, ref in zip(Xs, est.transform([X for X in Xs]), refs):
        assert_ewma(o, ref, X, alpha, 0, "%s %s n=%d one segment, host rows" % (name, dt, len(X)))


def test_double_ewma_does_not_reverse_its_backward_half(TS, monkeypatch):
    monkeypatch.setenv("MSM_TS_SEGMENT", "64")
    X = R.case_input("unreversed", 193, 3)
    fwd = host(TS.EWMA(com=3).partial_transform(place(X, "device")))
    bwd = host(TS.EWMA(com=3).partial_transform(place(np.ascontiguousarray(X[::-1]), "device")))
    both = host(TS.DoubleEWMA(com=3).partial_transform(place(X, "device")))
    assert np.array_equal(both, (fwd + bwd) / 2.)                # exactly the reference's recipe, bit for bit
    assert np.max(np.abs(both - (fwd + bwd[::-1]) / 2.)) > 1e-3   # and not the symmetric smoother


# ---- goldens: the reference's own outputs ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "timeseries_golden.npz"))


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_goldens(TS, monkeypatch, golden, dn, how):
    X = R.golden_input(np.float32 if dn == "f32" else np.float64)
    for seg in (None, "64"):
        if seg is None:
            monkeypatch.delenv("MSM_TS_SEGMENT", raising=False)
        else:
            monkeypatch.setenv("MSM_TS_SEGMENT", seg)
        for width, order in R.GOLDEN_BUTTERWORTH:
            if seg == "64" and width == 101 and order > 3:
                continue
            g = golden["bw_w%d_o%d_%s" % (width, order, dn)]
            _, ref, e_s = bw_reference_of(X, width, order)
            out = TS.Butterworth(width=width, order=order).partial_transform(place(X, how))
            assert_butterworth(out, X, ref, e_s, "golden w%d o%d %s %s" % (width, order, dn, how))
            scale = float(np.max(np.abs(ref)))
            # the golden is itself scipy's result (float32 rows: with the extension formed in float32 and the result
            # rounded to float32): its own distance to the restatement is added to the device's bound
            e_g = R.relerr(g, ref)
            assert g.dtype == host(out).dtype
            assert np.max(np.abs(host(out).astype(np.float64) - g.astype(np.float64))) <= R.butterworth_bound(e_s, scale, g.dtype) + e_g * scale
        for tag, kw, adjust, mp in R.GOLDEN_EWMA:
            alpha = R.ewm_alpha(**kw)
            S = int(seg) if seg else 0
            seams = -(-len(X) // S) - 1 if S else 0
            tol = R.ewma_bound(alpha, seams, np.abs(X).max(0).astype(np.float64)) + R.ewma_bound(alpha, 0, np.abs(X).max(0).astype(np.float64))
            for cls, key in ((TS.EWMA, "ewma_"), (TS.DoubleEWMA, "dewma_")):
                g = golden[key + tag + "_" + dn]
                out = host(cls(min_periods=mp, adjust=adjust, **kw).partial_transform(place(X, how)))
                assert out.dtype == np.float64 and np.array_equal(np.isnan(out), np.isnan(g))
                live = ~np.isnan(g)
                assert (np.where(live, np.abs(out - g), 0).max(0) <= tol).all(), (key, tag, dn, how, seg)


@functools.lru_cache(maxsize=None)
def _bw_golden_ref(dn, width, order):
    X = R.golden_input(np.float32 if dn == "f32" else np.float64)
    ref = R.butterworth(X.astype(np.float64), width, order)
    return X, ref, R.relerr(R.scipy_butterworth(X, width, order), ref)


def bw_reference_of(X, width, order):
    return _bw_golden_ref("f32" if X.dtype == np.float32 else "f64", width, order)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_estimator_refusals(TS, monkeypatch):
    monkeypatch.delenv("MSM_TS_SEGMENT", raising=False)
    X = R.case_input("refuse", 40, 3)
    with pytest.raises(ValueError, match="shorter"):
        TS.Butterworth(width=5).partial_transform(X[:4])
    with pytest.raises(ValueError, match="shorter"):
        TS.Butterworth(width=101).transform([place(X, "device")])
    with pytest.raises(ValueError, match="padlen"):
        TS.Butterworth(width=3, order=3).partial_transform(X[:3])
    with pytest.raises(ValueError):
        TS.Butterworth().transform([X, X[:, :2]])
    with pytest.raises(ValueError):
        TS.Butterworth().partial_transform(X[:, 0])
    with pytest.raises(ValueError):
        TS.Butterworth(width=1)
    for kw in (dict(), dict(com=1, span=3), dict(com=-1), dict(span=0.5), dict(halflife=0), dict(com=1, freq="D"),
               dict(com=1, min_periods=-1)):
        for cls in (TS.EWMA, TS.DoubleEWMA):
            with pytest.raises(ValueError):
                cls(**kw).partial_transform(X)
    for v in (np.nan, np.inf):
        for row in (0, 39):
            bad = X.copy()
            bad[row, 1] = v
            for cls in (TS.EWMA, TS.DoubleEWMA):
                for how in ("host", "device"):
                    with pytest.raises(ValueError, match="NaN, infinity"):
                        cls(com=1).partial_transform(place(bad, how))
    monkeypatch.setenv("MSM_TS_SEGMENT", "-4")
    with pytest.raises(ValueError):
        TS.EWMA(com=1).partial_transform(X)


def test_c_abi_refusals(gpu):
    L = gpu.lib()
    X = R.case_input("abi", 40, 3)
    out = np.empty_like(X)
    w, b, a, zi = R.butter_design(5, 3)

    def call(rows=40, dtype_bytes=8, F=3, ld=3, ld_out=3, kind=0, order=3, b=b, a=a, zi=zi, width=5, alpha=0.5, adjust=1,
             min_periods=0, segment=0, x=X, o=out, n_seq=1):
        ptr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64).ctypes.data
        keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (b, a, zi)]
        xp = (C.c_void_p * 1)(None if x is None else x.ctypes.data)
        op = (C.c_void_p * 1)(None if o is None else o.ctypes.data)
        nr = (C.c_int64 * 1)(rows)
        return L.msm_ts_filter(xp, op, nr, n_seq, dtype_bytes, F, ld, ld_out, 0, kind, order, *[None if k is None else k.ctypes.data for k in keep],
                               width, alpha, adjust, min_periods, segment)

    assert call() == gpu.MSM_OK and call(kind=1) == gpu.MSM_OK and call(kind=2, segment=16) == gpu.MSM_OK
    invalid = [dict(dtype_bytes=2), dict(F=0), dict(ld=2), dict(ld_out=2), dict(kind=3), dict(kind=-1), dict(order=0), dict(order=9),
               dict(b=None), dict(a=None), dict(zi=None), dict(width=4), dict(width=1), dict(a=2 * a), dict(b=b * np.nan),
               dict(segment=-1), dict(rows=4), dict(rows=-1), dict(x=None), dict(o=None), dict(rows=3, width=3),
               dict(kind=1, alpha=0.0), dict(kind=1, alpha=1.5), dict(kind=2, alpha=float("nan")), dict(kind=1, alpha=-0.5)]
    for kw in invalid:
        assert call(**kw) == gpu.MSM_ERR_INVALID, kw
        assert gpu.last_error()
    bad = X.copy()
    bad[17, 0] = np.nan
    for kind in (1, 2):
        assert call(kind=kind, x=bad) == gpu.MSM_ERR_NONFINITE
        assert "NaN, infinity" in gpu.last_error()
    assert call(n_seq=0) == gpu.MSM_OK and call(rows=0, kind=1) == gpu.MSM_OK
