"""GPU tests of BACE lumping: the estimator against the reference's stored runs (tests/golden/bace_golden.npz) and the
restatement of tests/bace_ref.py, ``msm_bace_pairs`` against the longdouble restatement within the derived bound
(bace_ref.pair_d, profiles/bace_bounds.txt) at every seam of the two kernels, exact ties, repeated runs and the refusals.

Seams.  Tile kernel: 32 x 32 pairs per workgroup, 32 columns per LDS chunk -> n = 31, 32, 33, and 65 (three tiles a side,
more than one workgroup's rows).  Row kernel: 16 pairs per workgroup -> n = 15, 16, 17; 128 columns per pass -> n = 127, 128,
129.  Merge loop: 256 states per workgroup of the update kernel, 256 threads across a row of the maxima -> n = 257.

Bayes factors.  A recorded factor is fl32(1 / fl32(1 / fl32(d))).  d on the device and in the reference differ by parts in
10^13 (the bound), each of the three roundings is at most half a float32 ulp on either side, so two factors differ by at
most 3 float32 ulps <= 3 * 2^-23 relatively."""
import ctypes as C
import os

import numpy as np
import pytest

import bace_ref as R

pytestmark = pytest.mark.gpu

SEAMS = [15, 16, 17, 31, 32, 33, 65, 127, 128, 129, 257]
FACTOR_RTOL = 3 * 2.0 ** -23


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bace_golden.npz")))


@pytest.fixture(scope="module")
def B(gpu):
    from msmbuilder_amd.lumping import bace
    return bace


def fitted_msm(counts, **params):
    from msmbuilder_amd import MarkovStateModel
    n = len(counts)
    msm = MarkovStateModel(verbose=False, **params)
    msm.transmat_, msm.populations_, msm.countsmat_ = None, np.full(n, 1.0 / n), counts
    msm.mapping_, msm.n_states_ = dict(zip(range(n), range(n))), n
    return msm


def assert_run(model, maps, bayes_keys, bayes, n_macrostates, what):
    left = sorted(model.map_dict, reverse=True)
    assert len(left) == len(maps), what
    for k, want in zip(left, maps):
        assert np.array_equal(model.map_dict[k], want), (what, k)
    assert model.microstate_mapping_.dtype == np.int32
    if len(maps):
        assert np.array_equal(model.microstate_mapping_, model.map_dict[n_macrostates]), what
    keys = sorted(model.bayesFactors, reverse=True)
    assert keys == list(bayes_keys), what
    got = np.array([model.bayesFactors[k] for k in keys], dtype=np.float32)
    want = np.asarray(bayes, dtype=np.float32)
    assert all(isinstance(model.bayesFactors[k], np.float32) for k in keys)
    assert np.array_equal(np.isinf(got), np.isinf(want)), what
    fin = np.isfinite(want)
    with np.errstate(all='ignore'):   # (a factor of exactly 0 -- an inf was stored -- has to be met exactly)
        off = np.where(got[fin] == want[fin], 0.0, np.abs(got[fin].astype(np.float64) - want[fin]) / np.abs(want[fin]))
    print(what, "largest factor difference %.3g of %.3g allowed" % (off.max() if off.size else 0.0, FACTOR_RTOL))
    assert np.all(off <= FACTOR_RTOL), (what, off.max())


# ---- the estimator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GOLDEN))
def test_from_msm_against_reference(B, golden, name):
    from msmbuilder_amd import BACE
    spec = R.GOLDEN[name]
    msm = fitted_msm(R.golden_counts(spec), lag_time=spec.get('lag_time', 1), sliding_window=spec.get('sliding_window', True))
    before = msm.countsmat_.copy()
    m = BACE.from_msm(msm, spec['n_macrostates'], filter=spec['filter'])
    assert np.array_equal(msm.countsmat_, before) and m.countsmat_ is msm.countsmat_ and m.mapping_ is msm.mapping_
    assert_run(m, golden[name + "_maps"], golden[name + "_bayes_keys"], golden[name + "_bayes"], spec['n_macrostates'], name)
    if golden[name + "_mapping"].min() >= 0:
        assert np.array_equal(m.microstate_mapping_, golden[name + "_mapping"])
    assert np.array_equal(m.microstate_mapping_, golden[name + "_maps"][-1])   # (a), also where the reference sets nothing
    # the merge record itself, a second run bit for bit, and a merge into a state that merges again
    c, w, unm, alive, keep = R.state_after(msm.countsmat_ * (spec.get('lag_time', 1)), 0, spec['filter'])
    merges, values = B.bace_merges(c, w, alive, spec['n_macrostates'])
    again = B.bace_merges(c, w, alive, spec['n_macrostates'])
    assert np.array_equal(merges[:-1], golden[name + "_merges"])
    assert np.array_equal(merges, again[0]) and np.array_equal(values.view(np.int32), again[1].view(np.int32))
    if len(merges) > 4:
        first = merges[:-1, 0].tolist()
        assert len(set(first)) < len(first)


def test_fit_on_label_sequences(B):
    from msmbuilder_amd import BACE
    seqs = R.label_sequences(20, 2, 0)
    m = BACE(n_macrostates=2, filter=0, lag_time=1, verbose=False).fit(seqs)
    assert m.n_states_ == 20
    r = R.bace(m.countsmat_, 2, filt=0, lag_time=1, sliding_window=True)
    assert min(r['gaps']) >= 64 * R.F32_ULP
    keys = sorted(r['bayes'], reverse=True)
    assert_run(m, [r['maps'][k] for k in sorted(r['maps'], reverse=True)], keys, [r['bayes'][k] for k in keys], 2, "fit")
    inverse = [m.mapping_[s] for s in range(20)]
    assert sorted(np.bincount(m.microstate_mapping_).tolist()) == [10, 10]
    assert len(set(m.microstate_mapping_[inverse][np.arange(20) % 2 == 0])) == 1
    out = m.transform([seqs[0][:50]])
    assert np.array_equal(np.concatenate(out[0]) if isinstance(out[0], list) else out[0], m.microstate_mapping_[[m.mapping_[s] for s in seqs[0][:50]]])
    filled = m.partial_transform(np.array([0, 99, 3]), mode='fill')
    assert np.isnan(filled[1]) and filled[0] == m.microstate_mapping_[m.mapping_[0]]
    with pytest.raises(RuntimeError, match="n_macrostates must not be None to fit"):
        BACE(None, verbose=False).fit(seqs)
    again = BACE(n_macrostates=3, filter=0, lag_time=1, verbose=False).fit(seqs).fit(seqs)   # (b)
    assert sorted(again.map_dict) == list(range(3, 20)) and sorted(again.bayesFactors) == list(range(2, 20))


def test_no_merge_and_no_candidate(B):
    from msmbuilder_amd import BACE
    C0 = R.block_counts(12, 2, 0)
    for nm in (12, 40):
        m = BACE.from_msm(fitted_msm(C0), nm, filter=0)
        assert m.map_dict == {} and np.array_equal(m.microstate_mapping_, np.arange(12)) and sorted(m.bayesFactors) == [11]
    two = R.disconnected_counts()
    ok = BACE.from_msm(fitted_msm(two), 2, filter=0)
    assert ok.microstate_mapping_.tolist() == [0, 0, 1, 1] and np.isinf(ok.bayesFactors[1])
    with pytest.raises(ValueError, match="at 2 states"):
        BACE.from_msm(fitted_msm(two), 1, filter=0)
    heavy = BACE.from_msm(fitted_msm(R.self_heavy_counts()), 2, filter=1.1)
    want = R.bace(R.self_heavy_counts(), 2, filt=1.1)
    assert np.array_equal(heavy.microstate_mapping_, want['mapping']) and heavy.microstate_mapping_.min() == 0


# ---- msm_bace_pairs --------------------------------------------------------------------------------------------------
def check_pairs(B, c, w, unm, alive, keep, rows, what, device=False):
    """Tile kernel and row kernel (for ``rows``) against the longdouble restatement within its bound; stored values are the
    two correctly rounded float32 roundings of d; both kernels give the same bits."""
    n = len(c)
    counts = c
    if device:
        import torch
        counts = torch.as_tensor(c, device='cuda')
    host = (lambda t: t.cpu().numpy()) if device else (lambda t: t)
    tile, tile_d = [host(t) for t in B.bace_pairs(counts, w, unm, alive, return_d=True)]
    want_rows = sorted(set(rows) | ({int(keep[0]), int(keep[-1])} if n <= 65 else set()))
    full = n <= 65
    worst = 0.0
    for x in (keep if full else want_rows):
        J = np.flatnonzero((c[x, :] > 1) & (alive > 0) & (np.arange(n) > x))
        mask = np.zeros(n, dtype=bool)
        mask[J] = True
        assert not tile[x, ~mask].any() and not tile_d[x, ~mask].any(), (what, x)
        if len(J):
            d, bound = R.pair_d(c, w, unm, keep, x, J, wide=True)
            err = np.abs(tile_d[x, J].astype(np.longdouble) - d)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (what, x, float((err / bound).max()))
            assert np.array_equal(tile[x, J].view(np.int32), R.stored(tile_d[x, J]).view(np.int32)), (what, x)
    assert not tile[alive == 0].any() and not tile[:, alive == 0].any(), what
    for x in want_rows:
        row, row_d = [host(t) for t in B.bace_pairs(counts, w, unm, alive, row=x, return_d=True)]
        J = np.flatnonzero((c[x, :] > 1) & (alive > 0) & (np.arange(n) != x))
        mask = np.zeros((n, n), dtype=bool)
        mask[x, J] = True
        assert not row[~mask].any() and not row_d[~mask].any(), (what, x)
        if len(J):
            d, bound = R.pair_d(c, w, unm, keep, x, J, wide=True)
            err = np.abs(row_d[x, J].astype(np.longdouble) - d)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (what, x, float((err / bound).max()))
            assert np.array_equal(row[x, J].view(np.int32), R.stored(row_d[x, J]).view(np.int32)), (what, x)
            # the same pair from the tile kernel, where it is a candidate there too (c[lo, hi] > 1): bit for bit
            lo, hi = np.minimum(x, J), np.maximum(x, J)
            both = c[lo, hi] > 1
            assert np.array_equal(row_d[x, J][both].view(np.int64), tile_d[lo, hi][both].view(np.int64)), (what, x)
            assert np.array_equal(row[x, J][both].view(np.int32), tile[lo, hi][both].view(np.int32)), (what, x)
    print(what, "largest error %.3f of the bound" % worst)


@pytest.mark.parametrize("n", SEAMS)
def test_pairs_at_the_seams(B, n):
    k = 2 if n < 30 else 3
    c, w, unm, alive, keep = R.state_after(R.block_counts(n, k, 10 + n), 0)
    check_pairs(B, c, w, unm, alive, keep, [0, n // 2, n - 1], "fresh n=%d" % n)
    # the middle of a run: merged states (no pseudo-count), merged-away states (skipped), sparse counts
    c, w, unm, alive, keep = R.state_after(R.block_counts(n, k, 20 + n, zeros=0.3), min(5, n // 3))
    assert (unm[keep] == 0).any() and (alive == 0).any()
    check_pairs(B, c, w, unm, alive, keep, [int(keep[np.flatnonzero(unm[keep] == 0)[0]]), int(keep[len(keep) // 2])], "mid-run n=%d" % n,
                device=(n in (33, 129)))


def test_pairs_with_pruned_states(B):
    c, w, unm, alive, keep = R.state_after(R.golden_counts(R.GOLDEN['weak48']), 2, filt=1.1)
    assert len(keep) < 46
    check_pairs(B, c, w, unm, alive, keep, [int(keep[3])], "pruned n=48", device=True)


# ---- exact ties ------------------------------------------------------------------------------------------------------
def test_ties_take_the_first_maximum(B):
    from msmbuilder_amd import BACE
    for what, counts in (("tied", R.tied_counts()), ("duplicated", R.duplicated_counts(20, 2, 0))):
        r = R.bace(counts, 2, filt=0)
        assert r['gaps'][0] == 0.0 and min(g for g in r['gaps'] if g > 0) >= 64 * R.F32_ULP
        c, w, unm, alive, keep = R.state_after(counts, 0)
        stored = B.bace_pairs(c, w, unm, alive)
        best = stored.max()
        assert (stored == best).sum() >= 2                                       # equal stored values on the device
        assert np.unravel_index(np.argmax(stored), stored.shape) == r['merges'][0]
        merges, values = B.bace_merges(c, w, alive, 2)
        assert [tuple(m) for m in merges[:-1]] == r['merges'], what
        m = BACE.from_msm(fitted_msm(counts), 2, filter=0)
        keys = sorted(r['bayes'], reverse=True)
        assert_run(m, [r['maps'][k] for k in sorted(r['maps'], reverse=True)], keys, [r['bayes'][k] for k in keys], 2, what)
    assert np.isinf(values[0]) and m.bayesFactors[19] == 0.0 and tuple(merges[0]) == (1, 4)   # d == 0: inf stored, merged first


def test_rows_refreshed_after_a_merge(B):
    """n = 3 is the first n with a row beside the merged pair, whose cached maximum may point at a merged column."""
    C3 = np.array([[40.0, 3.0, 30.0], [5.0, 50.0, 4.0], [28.0, 2.0, 45.0]])
    r = R.bace(C3, 1, filt=0)
    c, w, unm, alive, keep = R.state_after(C3, 0)
    merges, values = B.bace_merges(c, w, alive, 1)
    assert [tuple(m) for m in merges[:-1]] == r['merges'] and tuple(merges[-1]) == (-1, -1) and values[-1] == 0
    assert np.array_equal(values, np.array(r['values'], dtype=np.float32)) or np.allclose(values, r['values'], rtol=FACTOR_RTOL)
    import torch
    on_device = B.bace_merges(torch.as_tensor(c, device='cuda'), w, alive, 1)
    assert np.array_equal(on_device[0], merges) and np.array_equal(on_device[1].view(np.int32), values.view(np.int32))


# ---- the grid-stride loops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_strides_change_nothing(B, monkeypatch, cap):
    """The tile, row and row-maximum kernels walk their work in grid strides, which at the sizes above they never need: the
    caps (2^20, 2^16 and 2,048 workgroups) are far away.  MSM_BACE_MAX_GRID caps the grids -- at 1 a single workgroup does
    everything, at 3 the strides leave a remainder -- and every result is the uncapped one, which the tests above hold to
    the reference and the restatement, bit for bit."""
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    for n, k, merged in ((65, 3, 0), (257, 3, 5)):
        c, w, unm, alive, keep = R.state_after(R.block_counts(n, k, 20 + n, zeros=0.3), merged)
        x = int(keep[len(keep) // 2])
        monkeypatch.delenv("MSM_BACE_MAX_GRID", raising=False)
        assert libc.getenv(b"MSM_BACE_MAX_GRID") is None
        plain = B.bace_pairs(c, w, unm, alive, return_d=True) + B.bace_pairs(c, w, unm, alive, row=x, return_d=True)
        fresh = R.state_after(R.block_counts(n, k, 20 + n, zeros=0.3), 0)
        record = B.bace_merges(fresh[0], fresh[1], fresh[3], k)
        monkeypatch.setenv("MSM_BACE_MAX_GRID", str(cap))
        assert libc.getenv(b"MSM_BACE_MAX_GRID") == str(cap).encode()      # (the library reads the C environment)
        capped = B.bace_pairs(c, w, unm, alive, return_d=True) + B.bace_pairs(c, w, unm, alive, row=x, return_d=True)
        for a, b in zip(plain, capped):
            assert a.any() and np.array_equal(a.view(np.int32), b.view(np.int32)), (n, cap)
        again = B.bace_merges(fresh[0], fresh[1], fresh[3], k)
        assert len(record[0]) == n - k + 1 and record[0].min() >= 0
        assert np.array_equal(record[0], again[0]) and np.array_equal(record[1].view(np.int32), again[1].view(np.int32)), (n, cap)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(B):
    import torch
    from msmbuilder_amd import BACE, _lib
    C0 = R.block_counts(12, 2, 0)
    with pytest.raises(ValueError, match="n_macrostates"):
        BACE.from_msm(fitted_msm(C0), 0, filter=0)
    for bad in (-1.0, np.nan, np.inf):
        X = C0.copy()
        X[3, 4] = bad
        with pytest.raises(ValueError, match="non-negative and finite"):
            BACE.from_msm(fitted_msm(X), 2, filter=0)
        w, flags = X.sum(1) + 1, np.ones(12, dtype=np.int32)
        for counts in (X, torch.as_tensor(X, device='cuda')):
            with pytest.raises(ValueError, match="non-negative and finite"):
                B.bace_merges(counts, np.abs(np.nan_to_num(w, posinf=1.0)) + 1, flags, 2)
            with pytest.raises(ValueError, match="non-negative and finite"):
                B.bace_pairs(counts, np.abs(np.nan_to_num(w, posinf=1.0)) + 1, flags, flags)
    with pytest.raises(ValueError, match="at most 16384 states"):
        BACE.from_msm(fitted_msm(np.broadcast_to(np.ones(1), (16385, 16385))), 2, filter=0)
    with pytest.raises(ValueError, match="at least 2 states"):
        BACE.from_msm(fitted_msm(np.ones((1, 1))), 1, filter=0)
    with pytest.raises(RuntimeError, match="n_macrostates must not be None to transform"):
        BACE(None).partial_transform([0, 1])
    # the C ABI: status and msm_last_error()
    L = _lib.lib()
    w, flags = C0.sum(1) + 1, np.ones(12, dtype=np.int32)
    merges, values, count = np.zeros((12, 2), dtype=np.int32), np.zeros(12, dtype=np.float32), C.c_int64(0)
    out = np.zeros((12, 12), dtype=np.float32)
    some, none = flags.copy(), np.zeros(12, dtype=np.int32)
    some[3] = 0
    p = lambda a: a.ctypes.data   # noqa: E731

    def fit(counts=p(C0), w_=p(w), keep=p(flags), n=12, nm=2, mg=p(merges), vl=p(values), cap=12, cnt=C.byref(count)):
        return L.msm_bace_fit(counts, w_, keep, n, nm, mg, vl, cap, cnt, None, 0)

    def pairs(counts=p(C0), w_=p(w), unm=p(flags), alive=p(flags), n=12, row=-1, o=p(out)):
        return L.msm_bace_pairs(counts, w_, unm, alive, n, row, o, None, 0)

    assert fit() == _lib.MSM_OK and count.value == 11 and pairs() == _lib.MSM_OK
    for call, text in ((lambda: fit(counts=None), "null pointer"), (lambda: fit(w_=None), "null pointer"),
                       (lambda: fit(keep=None), "null pointer"), (lambda: fit(mg=None), "null pointer"),
                       (lambda: fit(vl=None), "null pointer"), (lambda: fit(cnt=None), "null pointer"),
                       (lambda: fit(n=1), "at least 2 states"), (lambda: fit(n=16385), "at most 16384 states"),
                       (lambda: fit(nm=0), "n_macrostates must be at least 1"), (lambda: fit(cap=3), "record holds"),
                       (lambda: pairs(counts=None), "null pointer"), (lambda: pairs(o=None), "null pointer"),
                       (lambda: pairs(unm=None), "null pointer"), (lambda: pairs(n=1), "at least 2 states"),
                       (lambda: pairs(n=16385), "at most 16384 states"), (lambda: pairs(row=12), "not a kept state"),
                       (lambda: pairs(alive=None), "null pointer"), (lambda: pairs(w_=None), "null pointer"),
                       (lambda: pairs(alive=p(some), unm=p(some), row=3), "row 3 is not a kept state"),
                       (lambda: fit(keep=p(none)), "no state is kept")):
        assert call() == _lib.MSM_ERR_INVALID and text in _lib.last_error(), text
    assert pairs(alive=p(some), unm=p(some), row=4) == _lib.MSM_OK and not out[3].any() and not out[:, 3].any() and out[4].any()
    for bad in (0.0, -2.0, np.nan, np.inf):
        bad_w = w.copy()
        bad_w[5] = bad
        assert fit(w_=p(bad_w)) == _lib.MSM_ERR_INVALID and "weight of kept state 5" in _lib.last_error()
        assert pairs(w_=p(bad_w)) == _lib.MSM_ERR_INVALID and "weight of kept state 5" in _lib.last_error()
    bad_w[3] = 0.0                                               # (the weight of a state that is not kept is not looked at)
    bad_w[5] = w[5]
    assert pairs(w_=p(bad_w), alive=p(some), unm=p(some)) == _lib.MSM_OK
    for bad in (-1.0, np.nan, np.inf):
        X = C0.copy()
        X[11, 11] = bad
        assert fit(counts=p(X)) == _lib.MSM_ERR_NONFINITE and "non-negative and finite" in _lib.last_error()
        assert pairs(counts=p(X)) == _lib.MSM_ERR_NONFINITE
    plan = (C.c_int64 * 6)()
    assert L.msm_bace_plan(plan) == _lib.MSM_OK and list(plan) == [32, 32, 16, 128, 256, 16384]
    assert L.msm_bace_plan(None) == _lib.MSM_ERR_INVALID
