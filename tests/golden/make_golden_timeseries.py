#!/usr/bin/env python
"""tests/golden/make_golden_timeseries.py -- generate timeseries_golden.npz.

Runs ONLY where the reference tree is present (like make_golden.py, whose loader it uses): the reference's own
preprocessing/timeseries.py is imported *by file path* -- nothing of the reference is copied into this repository -- and its
outputs are stored next to this script.  The inputs are regenerated from seeds (tests/timeseries_ref.py: ``golden_input``)
by this script and by the tests alike, so the file holds outputs only.

* Butterworth: ``Butterworth(width, order).partial_transform(X)`` of the reference itself, float32 and float64 rows.
* EWMA / DoubleEWMA: ``DataFrame.ewm(...).mean()`` called directly, with the reference's ``(fwd + bwd) / 2`` recipe
  (``bwd`` over ``X[::-1]``, not reversed back) on top.  Why not the reference's classes: they pass ``freq=`` to ``ewm``,
  which the pandas of this decade does not take (``TypeError``), so the reference's own call does not run; every other
  argument is handed on as the reference hands it on.

Usage:  python tests/golden/make_golden_timeseries.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (the loader recipe)
import timeseries_ref as R  # noqa: E402


def load_reference_timeseries():
    make_golden.load_reference()
    if "msmbuilder.preprocessing" not in sys.modules:
        pkg = types.ModuleType("msmbuilder.preprocessing")
        pkg.__path__ = [os.path.join(make_golden.REF, "preprocessing")]
        sys.modules["msmbuilder.preprocessing"] = pkg
    if "msmbuilder.preprocessing.base" not in sys.modules:
        # the mixin only maps transform over a list; partial_transform, which is all that is called here, is the class's own
        base = types.ModuleType("msmbuilder.preprocessing.base")
        base.MultiSequencePreprocessingMixin = type("MultiSequencePreprocessingMixin", (object,), {})
        sys.modules["msmbuilder.preprocessing.base"] = base
    return make_golden._load("msmbuilder.preprocessing.timeseries",
                             os.path.join(make_golden.REF, "preprocessing", "timeseries.py"), "msmbuilder.preprocessing")


def main():
    import pandas
    import scipy
    warnings.simplefilter("ignore")
    mod = load_reference_timeseries()
    g = {"scipy_version": np.array(scipy.__version__), "pandas_version": np.array(pandas.__version__)}
    for dn, dt in (("f32", np.float32), ("f64", np.float64)):
        X = R.golden_input(dt)
        for width, order in R.GOLDEN_BUTTERWORTH:
            out = mod.Butterworth(width=width, order=order).partial_transform(X)
            assert out.dtype == dt and out.shape == X.shape
            g["bw_w%d_o%d_%s" % (width, order, dn)] = out
        for tag, kw, adjust, mp in R.GOLDEN_EWMA:
            ewm = lambda Z: pandas.DataFrame(Z).ewm(com=kw.get("com"), span=kw.get("span"), halflife=kw.get("halflife"),
                                                    min_periods=mp, adjust=adjust).mean().values
            fwd, bwd = ewm(X), ewm(X[::-1, :])
            assert fwd.dtype == np.float64
            g["ewma_%s_%s" % (tag, dn)] = fwd
            g["dewma_%s_%s" % (tag, dn)] = (fwd + bwd) / 2.
    try:
        mod.EWMA(com=1.0).partial_transform(R.golden_input(np.float64))
        raise SystemExit("the reference's EWMA runs under this pandas: take the goldens from it")
    except TypeError as e:
        print("reference EWMA under pandas %s: TypeError: %s" % (pandas.__version__, e))
    np.savez_compressed(os.path.join(HERE, "timeseries_golden.npz"), **g)
    print("timeseries_golden.npz:", len(g), "arrays,", os.path.getsize(os.path.join(HERE, "timeseries_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
