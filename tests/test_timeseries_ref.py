"""The restatement of the time-series smoothers (tests/timeseries_ref.py) against scipy and pandas, and the tolerance the
device is held to, measured here and never taken from the device's own output (CPU only).

``measure()`` computes, for every shared test input, scipy's (pandas') own error against the long-double loop and the
error of the float64 emulation of the device's segment order; ``python tests/test_timeseries_ref.py`` writes them to
profiles/timeseries_bounds.txt with the date.  The tests assert what that file states: the emulation stays within
``butterworth_bound`` / ``ewma_bound`` of the restatement, the margin over scipy's error is at most ``MARGIN`` <= 4, and
every Butterworth input lies where scipy's own error is below 1e-9 of scale.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (run as a script: the package)
import timeseries_ref as R  # noqa: E402

from msmbuilder_amd import timeseries as TS  # noqa: E402

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "timeseries_bounds.txt")
# (width, order) where scipy's own error on a 2,000-frame un-centred walk is below 1e-9 of scale: all orders at small
# widths, the low orders at large ones.  Order 5 at width 1001 (scipy: 1e-5) and its neighbours are outside.
DOMAIN = ([(w, o) for w in (2, 3, 5) for o in range(1, 9)] + [(21, o) for o in range(1, 7)] +
          [(101, o) for o in range(1, 6)] + [(301, o) for o in (1, 2, 3)] + [(1001, o) for o in (1, 2, 3)])


def resolved_segment(a, segment, elements):
    """The segment the library runs a pass of ``elements`` at: the forced one, or the rule's."""
    if segment is not None:
        return segment
    os.environ.pop("MSM_TS_SEGMENT", None)
    return TS._segment_for(a, elements)


@functools.lru_cache(maxsize=None)
def measure():
    """{case: dict(e_ref=scipy's or pandas' error, e_emu=the emulation's, S=segment, seams, bound)}; Butterworth errors are
    relative to max |y|, EWMA errors absolute with the bound beside them."""
    pd = pytest.importorskip("pandas")
    pytest.importorskip("scipy.signal")
    out = {}
    for case in R.BW_CASES:
        name, width, order, n_max, seg = case
        w, b, a, zi = R.butter_design(width, order)
        worst = None
        for n in R.bw_case_lengths(case):   # the very trajectories the GPU test runs; the line kept is the worst ratio's
            X = R.case_input(name, n)
            elements = n + 2 * (w - 1) + 6 * (order + 1)
            S = resolved_segment(a, seg, elements)
            ref = R.butterworth(X, width, order)
            e_s = R.relerr(R.scipy_butterworth(X, width, order), ref)
            e_m = R.relerr(R.butterworth_segmented(X, width, order, S), ref)
            e_1 = R.relerr(R.butterworth_segmented(X, width, order, 0), ref)
            v = dict(kind="bw", width=w, order=order, n=n, S=S, seams=(-(-elements // S) - 1 if S else 0), e_ref=e_s, e_emu=e_m,
                     e_one=e_1, ratio=max(e_m, e_1) / max(e_s, R.ULPS * R.EPS64), e_ref_max=e_s)
            if worst is not None:
                v["e_ref_max"] = max(e_s, worst["e_ref_max"])
            worst = v if worst is None or v["ratio"] >= worst["ratio"] else dict(worst, e_ref_max=v["e_ref_max"])
        out[name] = worst
    for name, kw, adjust, mp, n, seg in R.EW_CASES:
        X = R.case_input(name, n)
        alpha = R.ewm_alpha(**kw)
        S = resolved_segment([1.0, -(1.0 - alpha)], seg, n)
        seams = -(-n // S) - 1 if S else 0
        ref = np.asarray(R.ewma(X, alpha, adjust, mp))
        live = ~np.isnan(ref.astype(np.float64))
        pdv = pd.DataFrame(X).ewm(adjust=adjust, min_periods=mp, **kw).mean().values
        assert np.array_equal(np.isnan(pdv), ~live)
        emu = R.ewma_segmented(X, alpha, adjust, mp, S)
        assert np.array_equal(np.isnan(emu), ~live)
        err = lambda y: float(np.max(np.abs(y - ref)[live], initial=0.0))
        out[name] = dict(kind="ew", alpha=alpha, n=n, S=S, seams=seams, e_ref=err(pdv), e_emu=err(emu),
                         bound_seq=R.ewma_bound(alpha, 0, np.abs(X).max()), bound=R.ewma_bound(alpha, seams, np.abs(X).max()))
    return out


def write_profile(path=PROFILE):
    import datetime
    m = measure()
    lines = ["Tolerances of the time-series smoothers at the test inputs (tests/timeseries_ref.py), written by",
             "`python tests/test_timeseries_ref.py` on %s; numpy float64 against a long-double sequential loop, CPU."
             % datetime.date.today().isoformat(),
             "Butterworth: errors relative to max |y|.  scipy = filtfilt's own error (the yardstick); emulation = the device's",
             "segment order in float64 at segment S (0: one segment); one = the same with one segment; ratio = max(emulation,",
             "one) / max(scipy, %g eps), and of the trajectories a case runs (lengths around the seams) the line is the one" % R.ULPS,
             "with the largest ratio.  Device bound = MARGIN x scipy + %g ulp of the output type, MARGIN = %g (largest ratio"
             % (R.ULPS, R.MARGIN),
             "measured below: %.2f; the cap is 4)." % max(v["ratio"] for v in m.values() if v["kind"] == "bw"),
             "%-18s %6s %5s %7s %6s %6s %10s %10s %10s %6s" % ("case", "width", "order", "frames", "S", "seams", "scipy",
                                                              "emulation", "one", "ratio")]
    for k, v in m.items():
        if v["kind"] == "bw":
            lines.append("%-18s %6d %5d %7d %6d %6d %10.3e %10.3e %10.3e %6.2f" % (k, v["width"], v["order"], v["n"], v["S"], v["seams"],
                                                                                v["e_ref"], v["e_emu"], v["e_one"], v["ratio"]))
    lines += ["EWMA: absolute errors on columns of |mean| = 100, std 1.  bound = ((2 / alpha + 1) + 2 seams) eps max|x|;",
              "pandas is held to the bound without seams.",
              "%-18s %9s %7s %6s %6s %10s %10s %10s %10s" % ("case", "alpha", "frames", "S", "seams", "pandas", "bound(0)", "emulation",
                                                         "bound")]
    for k, v in m.items():
        if v["kind"] == "ew":
            lines.append("%-18s %9.6f %7d %6d %6d %10.3e %10.3e %10.3e %10.3e" % (k, v["alpha"], v["n"], v["S"], v["seams"], v["e_ref"],
                                                                              v["bound_seq"], v["e_emu"], v["bound"]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


# ---- the restatement is scipy's and pandas' arithmetic ---------------------------------------------------------------------
@pytest.mark.parametrize("width,order", DOMAIN)
def test_restatement_is_filtfilt_on_the_reflect_padded_signal(width, order):
    pytest.importorskip("scipy.signal")
    X = R.walk(2000, 2, seed=width * 10 + order, offset=100.0)
    e = R.relerr(R.scipy_butterworth(X, width, order), R.butterworth(X, width, order))
    print("width %d order %d: scipy against the long-double loop %.3e" % (width, order, e))
    assert e < 1e-9                      # the domain
    if width <= 5 and order <= 4:
        assert e < 64 * R.EPS64          # and where the filter is well conditioned (low order, short memory) the two are one computation


def test_width_rule_and_short_trajectories():
    pytest.importorskip("scipy.signal")
    assert [R.butter_design(w, 1)[0] for w in (2, 3, 4, 5, 100, 101)] == [3, 3, 5, 5, 101, 101]
    X = R.walk(50, 2, seed=0)
    with pytest.raises(ValueError, match="shorter"):
        R.butterworth(X[:4], 5, 3)
    with pytest.raises(ValueError, match="padlen"):
        R.butterworth(X[:3], 3, 3)       # 3 + 2 * 2 = 7 padded frames, padlen 12
    R.butterworth(X[:5], 5, 3)
    bad = X.copy()
    bad[7, 1] = np.nan
    out = np.asarray(R.butterworth(bad, 5, 3), dtype=np.float64)
    assert np.isnan(out[:, 1]).all() and np.isfinite(out[:, 0]).all()


@pytest.mark.parametrize("kw", [dict(com=0), dict(com=0.5), dict(com=100), dict(span=1), dict(span=20), dict(halflife=0.3),
                                dict(halflife=7.5)])
@pytest.mark.parametrize("adjust", [True, False])
def test_restatement_is_pandas_ewm(kw, adjust):
    pd = pytest.importorskip("pandas")
    X = R.walk(700, 3, seed=5, offset=100.0)
    alpha = R.ewm_alpha(**kw)
    for mp in (0, 1, 5, 701):
        ref = np.asarray(R.ewma(X, alpha, adjust, mp))
        pdv = pd.DataFrame(X).ewm(adjust=adjust, min_periods=mp, **kw).mean().values
        live = ~np.isnan(pdv)
        assert np.array_equal(live, ~np.isnan(ref.astype(np.float64))) and live[:max(mp - 1, 0)].sum() == 0 and live[max(mp - 1, 0):].all()
        err = float(np.max(np.abs(pdv - ref)[live], initial=0.0))
        print(kw, adjust, mp, "pandas against the long-double loop %.3e, bound %.3e" % (err, R.ewma_bound(alpha, 0, np.abs(X).max())))
        assert err <= R.ewma_bound(alpha, 0, np.abs(X).max())
    fwd = pd.DataFrame(X).ewm(adjust=adjust, **kw).mean().values
    bwd = pd.DataFrame(X[::-1]).ewm(adjust=adjust, **kw).mean().values
    d = np.asarray(R.double_ewma(X, alpha, adjust))
    assert np.max(np.abs((fwd + bwd) / 2. - d)) <= R.ewma_bound(alpha, 0, np.abs(X).max())
    # the backward half is NOT reversed back: reversing it is a different (symmetric) smoother
    assert np.max(np.abs((fwd + bwd[::-1]) / 2. - d)) > 1e-3 or alpha == 1.0


def test_ewma_refuses_non_finite_rows():
    X = R.walk(20, 2, seed=1)
    for v in (np.nan, np.inf):
        bad = X.copy()
        bad[3, 0] = v
        with pytest.raises(ValueError):
            R.ewma(bad, 0.5)
        with pytest.raises(ValueError):
            R.ewma_segmented(bad, 0.5, S=8)


def test_estimator_refusals_need_no_device():
    pytest.importorskip("scipy.signal")
    for w in (1, 0, -3, 2.0, 5.5, "5", None, True):
        with pytest.raises((ValueError, TypeError)):
            TS.Butterworth(width=w)
    for o in (0, 9, 2.0, "3"):
        with pytest.raises((ValueError, TypeError)):
            TS.Butterworth(order=o)
    assert TS.Butterworth(width=2).width == 3 and TS.Butterworth(width=100).width == 101 and TS.Butterworth().order == 3
    for kw in (dict(), dict(com=1, span=3), dict(com=1, halflife=2), dict(span=3, halflife=2), dict(com=-0.1), dict(span=0.5),
               dict(halflife=0), dict(halflife=-1), dict(com=1, freq="D"), dict(com=1, min_periods=-1), dict(com=1, min_periods=1.5)):
        for cls in (TS.EWMA, TS.DoubleEWMA):
            with pytest.raises(ValueError):
                cls(**kw)._alpha()
    assert TS.EWMA(span=20)._alpha() == R.ewm_alpha(span=20) and TS.EWMA(halflife=7.5)._alpha() == R.ewm_alpha(halflife=7.5)
    assert TS.EWMA(com=3).fit([np.zeros((2, 2))]).com == 3


# ---- the segment rule -------------------------------------------------------------------------------------------------------
def test_segment_rule():
    pytest.importorskip("scipy.signal")
    for width, order in DOMAIN:
        a = R.butter_design(width, order)[2]
        S = TS.segment_length(a)
        assert S >= TS.SEGMENT_MIN and np.abs(R.state_power(a, S)).max() <= TS.SEGMENT_DECAY, (width, order, S)
    # the float64 coefficients of a wide order-5 or order-8 design do not forget: one segment per trajectory
    assert TS.segment_length(R.butter_design(1001, 5)[2]) == 0 and TS.segment_length(R.butter_design(101, 8)[2]) == 0
    assert TS.segment_length([1.0, -0.5]) == TS.SEGMENT_MIN
    a = [1.0, -(1 - R.ewm_alpha(com=100))]
    S = TS.segment_length(a)
    assert (1 - R.ewm_alpha(com=100)) ** S <= TS.SEGMENT_DECAY and S <= 1024
    os.environ.pop("MSM_TS_SEGMENT", None)
    assert TS._segment_for(a, 2 * S) == S and TS._segment_for(a, 2 * S - 1) == 0


# ---- the device's order of operations, held against the restatement ----------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.BW_CASES])
def test_butterworth_emulation_within_the_device_bound(name):
    v = measure()[name]
    print(name, v)
    assert v["e_ref_max"] < 1e-9
    assert v["e_emu"] <= R.MARGIN * v["e_ref"] + R.ULPS * R.EPS64 and v["e_one"] <= R.MARGIN * v["e_ref"] + R.ULPS * R.EPS64
    assert v["ratio"] <= R.MARGIN <= 4.0
    if name.endswith("_single"):
        assert v["S"] == 0
    if name.endswith("_long"):
        assert v["seams"] >= 2


@pytest.mark.parametrize("name", [c[0] for c in R.EW_CASES])
def test_ewma_emulation_and_pandas_within_the_bound(name):
    v = measure()[name]
    print(name, v)
    assert v["e_ref"] <= v["bound_seq"] and v["e_emu"] <= v["bound"]
    assert v["seams"] >= 1


def test_bounds_profile_lists_every_case():
    with open(PROFILE) as fh:
        text = fh.read()
    listed = {line.split()[0] for line in text.split("\n") if line and line.split()[0] in measure()}
    assert listed == set(measure())


if __name__ == "__main__":
    write_profile()
    print(open(PROFILE).read())
