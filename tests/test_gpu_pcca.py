"""GPU tests of PCCA and PCCA+ lumping: ``msm_pcca_*`` against the exact replay on lattice systems at every seam of the
kernels, against the longdouble restatement within the derived bounds on planted models (tests/pcca_ref.py,
profiles/pcca_bounds.txt), the -inf cases, repeated runs and the reuse switch, the estimators against the reference's stored
runs (tests/golden/pcca_golden.npz), the optimised fit, and the refusals.

Seams (all read from ``msm_pcca_plan``): ``rows`` rows of T per workgroup, ``cols`` columns per pass of a wave (a row of T is
read in 16-byte pairs: for odd n every second row starts 8 bytes off and is read in 8-byte loads), the 64 lanes of a wave
(n = 63, 64, 65) and the 256 threads of the block sums (n = 257, 1,025).  The kernels over V put the next power of two >= m
columns side by side: m = 2, 3, 8, 9, 16, 17, 64."""
import ctypes as C
import os

import numpy as np
import pytest

import pcca_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "pcca_golden.npz")))


@pytest.fixture(scope="module")
def PP(gpu):
    from msmbuilder_amd.lumping import pcca_plus
    return pcca_plus


@pytest.fixture(scope="module")
def plan(PP):
    return PP.pcca_plan()


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def handle_of(PP, s, device=False):
    if device:
        import torch
        return PP.PccaHandle(*[torch.as_tensor(np.ascontiguousarray(s[k]), device='cuda') for k in ('T', 'pi', 'V')])
    return PP.PccaHandle(s['T'], s['pi'], s['V'])


def everything(handle, s, mappings):
    """Every output of the handle on a lattice system, as one list of arrays."""
    out = list(handle.moments())
    for mp in mappings:
        out += list(handle.crisp(mp))
    A = R.to_square(s['alpha'], s['m']).astype(np.float64)
    out += list(handle.chi(A))
    for kind in range(3):
        value, info = handle.objective(kind, s['alpha'])
        out += [np.array([value]), info[:2]]
    return out


M_LIST = [2, 3, 8, 9, 16, 17, 64]
N_SPECS = ['2', '3', '63', '64', '65', 'rows-1', 'rows+1', 'cols-1', 'cols+1', '2*cols+1', '1025']


def lattice_sizes(plan, spec):
    """The (n, m) of one entry of N_SPECS: that n with two of the m (its largest one up to n = 2 cols + 1); 'every m': all of
    M_LIST on an odd n past one wave."""
    if spec == 'every m':
        return [(129, m) for m in M_LIST]
    n = eval(spec, {}, {'rows': plan['rows'], 'cols': plan['cols']})
    fits = [m for m in M_LIST if m <= n and (n <= 2 * plan['cols'] + 1 or m <= 17)]
    return sorted(set([(n, fits[N_SPECS.index(spec) % len(fits)]), (n, fits[-1])]))


# ---- lattice systems: exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", N_SPECS + ['every m'])
def test_lattice_systems_are_exact(PP, plan, monkeypatch, spec):
    """Every sum of the device is exact on these systems, so every output equals the replay bit for bit: the moments, the
    block sums of the home mapping, of one that leaves a macrostate empty and of one with a macrostate of one state, A, chi,
    the mapping and the three objectives.  The same bits come from device pointers and under MSM_PCCA_MAX_GRID = 1 and 3."""
    assert (plan['max_n'], plan['max_m']) == (16384, 64) and plan['rows'] >= 2 and plan['cols'] >= 64 and plan['threads'] % 64 == 0
    monkeypatch.delenv("MSM_PCCA_MAX_GRID", raising=False)
    for n, m in lattice_sizes(plan, spec):
        s = R.lattice(n, m, 0, zero_population=(n >= 3 * m and n % 2 == 1))
        home = (np.arange(n) % m).astype(np.int32)
        empty = np.where(home == m - 1, 0, home).astype(np.int32)         # the last macrostate receives nothing
        single = np.where(home == 1, 0, home).astype(np.int32)            # macrostate 1 keeps one state
        single[1] = 1
        with handle_of(PP, s) as h:
            got = everything(h, s, (home, empty, single))
            monkeypatch.setenv("MSM_PCCA_MAX_GRID", "1")
            one = everything(h, s, (home, empty, single))
            monkeypatch.setenv("MSM_PCCA_MAX_GRID", "3")
            three = everything(h, s, (home, empty, single))
            monkeypatch.delenv("MSM_PCCA_MAX_GRID")
        want = [x.astype(np.float64) for x in R.moments(s['T'], s['pi'], s['V'])]
        for mp in (home, empty, single):
            want += [x.astype(np.float64) for x in R.block_sums(s['T'], s['pi'], mp, m)]
        replays = [R.replay(kind, s) for kind in range(3)]
        want += [replays[0][1], replays[0][2], replays[0][3].astype(np.int32)]
        for kind in range(3):
            want += [np.array([replays[kind][0]]), np.array([1, m], dtype=np.int32)]
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and (np.array_equal(a, b) if a.dtype.kind == 'i' else same_bits(a, b)), (n, m, i)
        assert not got[4][m - 1] and not got[5][m - 1] and np.array_equal(replays[2][3], home), (n, m)
        assert np.all(np.isfinite([r[0] for r in replays]) | (s['pi'].min() == 0)), (n, m)
        for other in (one, three):
            assert all(same_bits(a, b) if a.dtype.kind == 'f' else np.array_equal(a, b) for a, b in zip(got, other)), (n, m)
        if n in (65, 2 * plan['cols'] + 1):
            with handle_of(PP, s, device=True) as h:
                dev = everything(h, s, (home, empty, single))
            assert all(same_bits(a, b) if a.dtype.kind == 'f' else np.array_equal(a, b) for a, b in zip(got, dev)), (n, m)


def test_exact_tie_goes_to_the_first_column(PP):
    """m = 2 with the last state at (max v + min v) / 2: both memberships are exactly 1/2 and macrostate 0 wins, as numpy's
    argmax has it."""
    for n in (9, 130):
        s = R.lattice(n, 2, 1, tie=True)
        with handle_of(PP, s) as h:
            A, chi, mapping = h.chi(R.to_square(s['alpha'], 2).astype(np.float64))
            value, info = h.objective(2, s['alpha'])
        want = R.replay(2, s)
        assert chi[n - 1].tolist() == [0.5, 0.5] and mapping[n - 1] == 0
        assert same_bits(chi, want[2]) and np.array_equal(mapping, want[3]) and same_bits(value, want[0]) and np.isfinite(value)


# ---- planted models: within the derived bound ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(33, 3), (33, 6), (257, 3), (257, 6), (1025, 3), (1025, 6)])
def test_planted_models_within_the_bound(PP, n, m):
    """Every kind at 20 seeded alphas around the initial A against the longdouble restatement in its direct form (T chi),
    within pcca_ref.device_bounds; chi within its bound, the mapping equal (every margin is far above the bound)."""
    s = R.planted_system(n, m, 0)
    T_ld = np.asarray(s['T'], dtype=LD)
    worst = np.zeros(3)
    with handle_of(PP, s) as h:
        G, w = h.moments()
        Gr, wr = R.moments(T_ld, s['pi'], s['V'])
        assert np.abs(G - Gr.astype(np.float64)).max() <= 4 * n * R.U * (np.abs(s['V']) * s['pi'][:, None]).T.dot(np.abs(s['T']).dot(np.abs(s['V']))).max()
        assert np.abs(w - wr.astype(np.float64)).max() <= 2 * n * R.U * np.abs(s['V'] * s['pi'][:, None]).sum(axis=0).max()
        for i, alpha in enumerate(R.alphas_around(s['V'], 20, 100 + n + m)):
            bound = R.device_bounds(s, alpha)
            info = None
            for kind in range(3):
                want, info = R.objective(kind, alpha, T_ld, s['pi'], s['V'])
                value, flags = h.objective(kind, alpha)
                assert np.isfinite(want) and flags[0] == 1 and flags[1] == m, (i, kind)
                err = abs(float(LD(value) - want))
                worst[kind] = max(worst[kind], err / bound['value'][kind])
                assert err <= bound['value'][kind], (i, kind, value, float(want), err, bound['value'][kind])
            assert np.all(R.argmax_margin(info['chi']) >= 1000 * bound['chi'].max(axis=1)), i
            A, chi, mapping = h.chi(R.to_square(alpha, m).astype(np.float64))
            assert np.array_equal(mapping, info['mapping']) and np.all(np.abs(chi - info['chi'].astype(np.float64)) <= bound['chi']), i
    print("n=%d m=%d largest fraction of the bound: crispness %.3g, metastability %.3g, crisp_metastability %.3g" % ((n, m) + tuple(worst)))


# ---- -inf ---------------------------------------------------------------------------------------------------------------------
def test_infeasible_points_are_minus_infinity(PP):
    for n, m in ((33, 3), (65, 6)):
        s = R.planted_system(n, m, 0)
        a0 = R.alphas_around(s['V'], 1, 0)[0]
        sq = a0.reshape(m - 1, m - 1).copy()
        sq[:, 1] = sq[:, 0]                       # two equal columns of A: the second macrostate never wins
        bad = [sq.ravel(), np.zeros_like(a0)]
        for poison in (np.nan, np.inf, -np.inf):
            x = a0.copy()
            x[len(x) // 2] = poison
            bad += [x, np.full_like(a0, poison)]
        with handle_of(PP, s) as h:
            for kind in range(3):
                assert np.isfinite(h.objective(kind, a0)[0])
                for i, alpha in enumerate(bad):
                    value, info = h.objective(kind, alpha)
                    want, winfo = R.objective(kind, alpha, s['T'], s['pi'], s['V'])
                    assert np.isneginf(value) and np.isneginf(want) and info[3] == 0, (n, m, kind, i, value)
                    assert not (info[0] == 1 and info[1] == m), (n, m, kind, i)
            value, info = h.objective(2, sq.ravel())
            assert info[0] == 1 and info[1] == m - 1     # feasible, but a macrostate is empty


# ---- repeats and the reuse switch --------------------------------------------------------------------------------------------
def test_repeats_and_the_reuse_switch(PP, monkeypatch):
    """The same alpha twice: the second evaluation meets the first one's mapping (info[2] = 1) and, for kind 2, forms its value
    from the remembered block sums (info[3] = 0).  MSM_PCCA_REUSE=0 forces the pass (info[3] = 1); the bits are the same."""
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    monkeypatch.delenv("MSM_PCCA_REUSE", raising=False)
    s = R.lattice(257, 3, 0)
    a0, a1 = s['alpha'], 2.0 * s['alpha']            # (a scaled alpha fills to the same A)
    far = a0.copy()
    far[1] = 0.5 * a0[0]                             # A[1, 2] > 0 moves states of macrostate 1 with a share of 2 over to 2
    base, same, other = [R.objective(2, x, s['T'], s['pi'], s['V']) for x in (a0, a1, far)]
    assert np.isfinite(other[0]) and np.count_nonzero(other[1]['mapping'] != base[1]['mapping']) >= 10
    assert np.array_equal(same[1]['mapping'], base[1]['mapping'])
    with handle_of(PP, s) as h:
        first, flags = {}, {}
        for kind in range(3):
            first[kind], info = h.objective(kind, a0)
            flags[kind] = info.tolist()
        # kind 2 meets kind 1's mapping, but no block sums are remembered yet: it passes over T
        assert flags == {0: [1, 3, 0, 0], 1: [1, 3, 1, 0], 2: [1, 3, 1, 1]}
        v, info = h.objective(2, a0)
        assert same_bits(v, first[2]) and info.tolist() == [1, 3, 1, 0]
        v, info = h.objective(2, a1)                 # another A, the same mapping: no pass either
        assert info.tolist() == [1, 3, 1, 0] and same_bits(v, first[2])
        v_far, info = h.objective(2, far)
        assert info.tolist() == [1, 3, 0, 1] and np.isfinite(v_far) and not same_bits(v_far, first[2])
        v, info = h.objective(2, a0)
        assert info.tolist() == [1, 3, 0, 1] and same_bits(v, first[2])
        for kind in (0, 1):                          # kinds 0 and 1 never pass over T and leave the remembered sums valid
            v, info = h.objective(kind, a0)
            assert info.tolist() == [1, 3, 1, 0] and same_bits(v, first[kind])
        v, info = h.objective(2, a0)
        assert info.tolist() == [1, 3, 1, 0] and same_bits(v, first[2])
        monkeypatch.setenv("MSM_PCCA_REUSE", "0")
        assert libc.getenv(b"MSM_PCCA_REUSE") == b"0"
        for _ in range(3):
            v, info = h.objective(2, a0)
            assert info.tolist() == [1, 3, 1, 1] and same_bits(v, first[2])
        monkeypatch.delenv("MSM_PCCA_REUSE")
        v, info = h.objective(2, a0)
        assert info.tolist() == [1, 3, 1, 0] and same_bits(v, first[2])
        assert (h.evaluations, h.passes, h.reused) == (14, 6, 11)
    with handle_of(PP, s) as h2:                      # a fresh handle: the first evaluation has no mapping to meet
        v, info = h2.objective(2, a0)
        assert info.tolist() == [1, 3, 0, 1] and same_bits(v, first[2])


# ---- the estimators against the reference's stored runs -------------------------------------------------------------------
def golden_system(golden, name):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_pcca import GOLDEN
    n, m, seed = GOLDEN[name]
    T, pi, labels = R.planted(n, m, seed)
    return dict(T=T, pi=pi, V=golden[name + '_V'], labels=labels, n=n, m=m)


def row_signs(A):
    """Rows 1.. of A are fixed up to the sign of their eigenvector: make each row's largest entry positive."""
    A = np.array(A, dtype=np.float64)
    for k in range(1, len(A)):
        A[k] *= np.sign(A[k, np.argmax(np.abs(A[k]))])
    return A


@pytest.mark.parametrize("name", ['p8_2', 'p33_3', 'p65_4', 'p100_9', 'p129_3', 'p257_6'])
def test_estimators_against_the_reference(PP, golden, name):
    from msmbuilder_amd import PCCA, PCCAPlus
    s = golden_system(golden, name)
    m = s['m']
    # the handle on the reference's own eigenvectors: A and chi to 1e-10 of their scale, the integers equal
    with handle_of(PP, s) as h:
        A, chi, mapping = h.chi(golden[name + '_A0'])
        assert np.array_equal(mapping, golden[name + '_map0'])
        assert np.abs(A - golden[name + '_A0']).max() <= 1e-10 * np.abs(golden[name + '_A0']).max()
        assert np.abs(chi - golden[name + '_chi0']).max() <= 1e-10 * np.abs(golden[name + '_chi0']).max()
        for alpha, values in zip(golden[name + '_alphas'], golden[name + '_values']):
            for kind in range(3):
                got = h.objective(kind, alpha)[0]
                assert got == values[kind] if np.isinf(values[kind]) else abs(got - values[kind]) <= 1e-10 * abs(values[kind])
    # from_msm: the eigenvectors are the device's own (their signs are free)
    msm = R.fitted_msm(s['T'], s['pi'])
    plus = PCCAPlus.from_msm(msm, m, do_minimization=False)
    assert np.array_equal(plus.microstate_mapping_, golden[name + '_map0']) and plus.microstate_mapping_.dtype == int
    assert np.abs(row_signs(plus.A_) - row_signs(golden[name + '_A0'])).max() <= 1e-10 * np.abs(golden[name + '_A0']).max()
    assert np.abs(plus.chi_ - golden[name + '_chi0']).max() <= 1e-10 * np.abs(golden[name + '_chi0']).max()
    assert plus.optimize_info_ == {'evaluations': 0, 'passes': 0, 'reused': 0}
    coarse = PCCA.from_msm(msm, m)
    assert R.same_partition(coarse.microstate_mapping_, golden[name + '_pcca'])
    flipped = np.where(np.sum(golden[name + '_V'] * np.asarray(coarse.right_eigenvectors_)[:, :m], axis=0) < 0)[0]
    if not len(flipped):                             # the same signs: the same labels, not only the same partition
        assert np.array_equal(coarse.microstate_mapping_, golden[name + '_pcca'])


def test_fit_on_label_sequences(PP):
    """``fit`` on labels, host and device, gives what ``from_msm`` gives on the fitted model, and the restatement's mapping on
    the model's own eigenvectors."""
    import torch
    from msmbuilder_amd import MarkovStateModel, PCCA, PCCAPlus
    seq = R.block_labels(24, 3, 0)
    pieces = [seq[:15000], seq[15000:]]
    msm = MarkovStateModel(lag_time=2, verbose=False).fit(pieces)
    for cls, kw in ((PCCA, {}), (PCCAPlus, {'do_minimization': False})):
        a = cls(3, lag_time=2, verbose=False, **kw).fit(pieces)
        b = cls(3, lag_time=2, verbose=False, **kw).fit([torch.as_tensor(p, device='cuda') for p in pieces])
        c = cls.from_msm(msm, 3, **kw)
        assert np.array_equal(a.microstate_mapping_, b.microstate_mapping_) and np.array_equal(a.microstate_mapping_, c.microstate_mapping_)
        assert R.same_partition(a.microstate_mapping_, np.arange(24) % 3)
        V = np.asarray(a.right_eigenvectors_)[:, :3]
        if cls is PCCA:
            assert np.array_equal(a.microstate_mapping_, R.pcca_split(V[:, 1:], 3))
        else:
            A0 = R.initial_A(V)[0]
            assert np.array_equal(a.microstate_mapping_, R.chi_of(A0, V)[1])
            assert np.abs(a.A_ - A0.astype(np.float64)).max() <= 1e-10 * np.abs(a.A_).max()
        out = a.transform([np.array([0, 1, 2, 99, 4])])
        assert [x.tolist() for x in out] == [a.microstate_mapping_[[0, 1, 2]].tolist(), a.microstate_mapping_[[4]].tolist()]
        coarse = cls(3, lag_time=2, verbose=False, **kw).fit_transform(pieces)
        assert len(coarse) == 2 and set(np.concatenate(coarse).tolist()) == {0, 1, 2}


# ---- the optimised fit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['p33_3', 'p129_3'])
@pytest.mark.parametrize("kind", R.KINDS)
def test_optimised_fit(PP, golden, name, kind):
    """On the planted models on which the goldens show the reference recovers the planted partition: so does the search on the
    device objective, and it does not lose against the initial A in the restatement's objective.  For the default objective
    a second fit with the same ``random_state`` gives the same A_ bit for bit."""
    from msmbuilder_amd import PCCAPlus
    s = golden_system(golden, name)
    assert R.same_partition(golden[name + '_opt_map'][R.KINDS.index(kind)], s['labels'])
    msm = R.fitted_msm(s['T'], s['pi'])
    fit = PCCAPlus.from_msm(msm, 3, objective_function=kind, random_state=0)
    assert R.same_partition(fit.microstate_mapping_, s['labels'])
    V = np.asarray(fit.right_eigenvectors_)[:, :3]
    start = R.objective(kind, R.alphas_around(V, 1, 0)[0], s['T'], s['pi'], V)[0]
    final = R.objective(kind, fit.A_[1:, 1:].ravel(), s['T'], s['pi'], V)[0]
    info = fit.optimize_info_
    print(name, kind, "evaluations %d, passes over T %d, reused %d; %.12g -> %.12g (reference: %.12g)"
          % (info['evaluations'], info['passes'], info['reused'], float(start), float(final), golden[name + '_opt_value'][R.KINDS.index(kind)]))
    assert np.isfinite(final) and final >= start and info['evaluations'] > 100 and info['passes'] <= info['evaluations']
    if kind == 'crisp_metastability':
        assert info['passes'] < info['evaluations']
        again = PCCAPlus.from_msm(msm, 3, objective_function=kind, random_state=0)
        assert same_bits(again.A_, fit.A_) and again.optimize_info_ == info


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(PP):
    from msmbuilder_amd import _lib
    L = _lib.lib()
    s = R.lattice(12, 3, 0)
    p = lambda a: a.ctypes.data   # noqa: E731
    handle = C.c_void_p(None)
    big = np.zeros(1)

    def create(T=p(s['T']), pi=p(s['pi']), V=p(s['V']), n=12, m=3, out=C.byref(handle)):
        return L.msm_pcca_create(T, pi, V, n, m, 0, out)

    for call, text in ((lambda: create(T=None), "null pointer"), (lambda: create(pi=None), "null pointer"),
                       (lambda: create(V=None), "null pointer"), (lambda: create(out=None), "null pointer"),
                       (lambda: create(m=1), "2 to 64 macrostates"), (lambda: create(m=65, n=100), "2 to 64 macrostates"),
                       (lambda: create(n=2), "cannot form"), (lambda: create(T=p(big), pi=p(big), V=p(big), n=16385), "at most 16384 states")):
        assert call() == _lib.MSM_ERR_INVALID and text in _lib.last_error(), text
        assert not handle.value
    assert create() == _lib.MSM_OK and handle.value
    value, info = C.c_double(0.0), np.zeros(4, dtype=np.int32)
    num, den, mapping = np.zeros(3), np.zeros(3), np.zeros(12, dtype=np.int32)
    A, chi = np.zeros((3, 3)), np.zeros((12, 3))
    alpha = np.ascontiguousarray(s['alpha'])
    assert L.msm_pcca_objective(handle, 2, p(alpha), C.byref(value), p(info)) == _lib.MSM_OK and np.isfinite(value.value)
    for kind in (-1, 3):
        assert L.msm_pcca_objective(handle, kind, p(alpha), C.byref(value), p(info)) == _lib.MSM_ERR_INVALID
        assert "kind must be 0, 1 or 2" in _lib.last_error()
    for call in (lambda: L.msm_pcca_objective(None, 2, p(alpha), C.byref(value), p(info)),
                 lambda: L.msm_pcca_objective(handle, 2, None, C.byref(value), p(info)),
                 lambda: L.msm_pcca_objective(handle, 2, p(alpha), None, p(info)),
                 lambda: L.msm_pcca_objective(handle, 2, p(alpha), C.byref(value), None),
                 lambda: L.msm_pcca_crisp(None, p(mapping), p(num), p(den)), lambda: L.msm_pcca_crisp(handle, None, p(num), p(den)),
                 lambda: L.msm_pcca_crisp(handle, p(mapping), None, p(den)), lambda: L.msm_pcca_crisp(handle, p(mapping), p(num), None),
                 lambda: L.msm_pcca_chi(None, p(A), p(A), p(chi), p(mapping)), lambda: L.msm_pcca_chi(handle, None, p(A), p(chi), p(mapping)),
                 lambda: L.msm_pcca_chi(handle, p(A), None, p(chi), p(mapping)), lambda: L.msm_pcca_chi(handle, p(A), p(A), p(chi), None),
                 lambda: L.msm_pcca_moments(None, p(A), p(num)), lambda: L.msm_pcca_moments(handle, None, p(num)),
                 lambda: L.msm_pcca_moments(handle, p(A), None), lambda: L.msm_pcca_plan(None)):
        assert call() == _lib.MSM_ERR_INVALID and "null pointer" in _lib.last_error()
    assert L.msm_pcca_chi(handle, p(np.diag([0.0, 1.0, 2.0])), p(A), None, p(mapping)) == _lib.MSM_OK     # chi_out may be null
    for bad in (-1, 3):
        mapping[7] = bad
        assert L.msm_pcca_crisp(handle, p(mapping), p(num), p(den)) == _lib.MSM_ERR_INVALID and "mapping[7]" in _lib.last_error()
    mapping[7] = 2
    assert L.msm_pcca_crisp(handle, p(mapping), p(num), p(den)) == _lib.MSM_OK
    assert L.msm_pcca_destroy(handle) == _lib.MSM_OK and L.msm_pcca_destroy(None) == _lib.MSM_OK
    with pytest.raises(ValueError, match="alpha must have 4 entries"):
        with handle_of(PP, s) as h:
            h.objective(2, np.zeros(3))
