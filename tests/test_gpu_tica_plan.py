"""GPU tier of the tICA launch plan: one case per kernel path and template flavour of tica_accumulate_device, through the C ABI.
Each case asserts that msm_tica_last_plan names the path and flavour the case is there for, that this plan is
msm_tica_plan's (and the restated dispatch's, tests/tica_plan_ref.py) for the handle's own geometry and the same inputs,
and that the accumulators meet a float64 oracle at the tolerances tests/test_gpu_tica.py states for the mode.
(msm_tica_plan plans whole trajectories: the segment cases hold their plan to the restated dispatch alone.)

Inputs: three ragged trajectories of 650 to 1,400 frames (_ar1 of test_gpu_tica.py) unless the case says otherwise.
The flavours expected at 2,048 features (remainder cohort) are those of 512 resident sum/difference workgroups."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_plan_ref as R  # noqa: E402
from test_gpu_tica import ATOL_SCALE, _ar1  # noqa: E402

pytestmark = pytest.mark.gpu

LAG = 10
LENS = (650, 1400, 1000)
MODES = {"f32": R.F32, "f64": R.F64, "bf16": R.BF16, "bf16x2": R.BF16X2}
SWITCHES = ("MSM_TICA_SYM", "MSM_TICA_SYMW", "MSM_TICA_SYMW64", "MSM_TICA_SHIFT", "MSM_TICA_FOLD", "MSM_TICA_IMG_FUSED",
            "MSM_TICA_IMG_CARRY", "MSM_TICA_IMG_RING_MB")


def case(name, F, want, mode="f32", rows="f32", lens=LENS, env=None, layout="plain"):
    return dict(name=name, F=F, want=want, mode=mode, rows=rows, lens=tuple(lens), env=env or {}, layout=layout)


CASES = [
    # whole-matrix kernel, float rows: element-wise at F = 3, then four of its variants
    case("symw-3", 3, ("symw", 0)), case("symw-12", 12, ("symw", R.FL_VEC)), case("symw-100", 100, ("symw", R.FL_VEC)),
    case("symw-171", 171, ("symw", R.FL_VEC)), case("symw-256", 256, ("symw", R.FL_VEC)),
    # ... double rows
    case("symw64-1", 1, ("symw64", 0), rows="f64"), case("symw64-64", 64, ("symw64", R.FL_VEC), rows="f64"),
    case("symw64-128", 128, ("symw64", R.FL_VEC), rows="f64"),
    case("f64rows-129", 129, ("cg64", 0), rows="f64"),
    # sum/difference kernel
    case("sym-260-edge", 260, ("sym", R.FL_EDGE)), case("sym-512-full", 512, ("sym", 0)),
    case("sym-2048-rem", 2048, ("sym", R.FL_REM)),
    case("sym-2048-search", 2048, ("sym", R.FL_REM), lens=(12500,)),
    case("sym-512-fold", 512, ("sym", R.FL_FOLD), env={"MSM_TICA_FOLD": "2"}),
    case("sym-2048-fold-rem", 2048, ("sym", R.FL_FOLD | R.FL_REM), env={"MSM_TICA_FOLD": "2"}),
    # C/G fp32 kernel
    case("cg32-512-full", 512, ("cg32", R.FL_ALIGNED), env={"MSM_TICA_SYM": "0"}),
    case("cg32-260-edge", 260, ("cg32", R.FL_ALIGNED | R.FL_EDGE), env={"MSM_TICA_SYM": "0"}),
    case("cg32-258", 258, ("cg32", R.FL_EDGE)),
    case("cg32-512-misaligned", 512, ("cg32", R.FL_EDGE), layout="one float in"),
    # f64 mode
    case("f64mode-f32rows", 130, ("cg64", 0), mode="f64"), case("f64mode-f64rows", 130, ("cg64", 0), mode="f64", rows="f64"),
    # bf16 image paths
    case("img-bf16-300", 300, ("img_ring", 0), mode="bf16"), case("img-bf16x2-300", 300, ("img_ring", R.FL_X2), mode="bf16x2"),
    case("img-fused-512", 512, ("img_fused", 0), mode="bf16", rows="bf16"),
    case("img-ring-512", 512, ("img_ring", 0), mode="bf16", rows="bf16", env={"MSM_TICA_IMG_FUSED": "0"}),
]
CARRY_LENS = (9000, 8000, 10000)
CARRY_CASES = [case("img-carry-%s" % c, 256, ("img_ring", 0), mode="bf16", rows="bf16", lens=CARRY_LENS,
                    env={"MSM_TICA_IMG_FUSED": "0", "MSM_TICA_IMG_CARRY": c}) for c in ("1", "2")]
SEGMENT_CASES = [case("seg-128", 128, ("symw", R.FL_VEC), lens=(2000,)), case("seg-512", 512, ("sym", 0), lens=(2000,)),
                 case("seg-f64mode", 130, ("cg64", 0), mode="f64", lens=(2000,))]
SEGMENTS = ((0, 700), (700, 1500), (1500, 2000))     # owned left frames of the three slices of the one trajectory


class Handle:
    """msm_tica_* on device tensors."""

    def __init__(self, F, mode, lag=LAG):
        from msmbuilder_amd import _lib
        self.L, self.F, self.lag, self._lib = _lib.lib(), F, lag, _lib
        self.h = C.c_void_p()
        _lib.check(self.L.msm_tica_create(C.byref(self.h), F, lag, MODES[mode]))

    def _bind(self):
        import torch
        self._lib.set_stream(torch.cuda.current_stream().cuda_stream)

    def accumulate(self, seqs, check=True):
        """One launch over device tensors (rows contiguous, common row stride).  Returns the library's code."""
        self._bind()
        n = len(seqs)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in seqs])
        rows = (C.c_int64 * n)(*[s.shape[0] for s in seqs])
        skipped = C.c_int64(0)
        self.launch = dict(dtype_bytes=seqs[0].element_size(), ld=seqs[0].stride(0), n_rows=[s.shape[0] for s in seqs],
                           ptr16=all(s.data_ptr() % 16 == 0 for s in seqs if s.shape[0] > self.lag),
                           ptr16_all=all(s.data_ptr() % 16 == 0 for s in seqs))
        rc = self.L.msm_tica_accumulate_batch(self.h, ptrs, rows, n, self.launch["dtype_bytes"], self.launch["ld"], 1, 1, C.byref(skipped))
        if check:
            self._lib.check(rc)
        return rc

    def accumulate_segments(self, X, segments):
        """Slices [ob, min(oe + lag, len)) of ONE trajectory, each owning the left frames [ob, oe), in one launch."""
        self._bind()
        n, length = len(segments), X.shape[0]
        slices = [X[ob:min(oe + self.lag, length)] for ob, oe in segments]
        ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in slices])
        rows = (C.c_int64 * n)(*[s.shape[0] for s in slices])
        seg4 = (C.c_int64 * (4 * n))(*[v for ob, oe in segments for v in (length, ob, ob, oe)])
        skipped = C.c_int64(0)
        self._lib.check(self.L.msm_tica_accumulate_segments(self.h, ptrs, rows, seg4, n, X.element_size(), X.stride(0), 1, 1, C.byref(skipped)))

    def packed(self):
        """[C | G | s0 | stau | n_observations | n_sequences] as float64."""
        out = np.zeros(int(self.L.msm_tica_packed_size(self.h)), dtype=np.float64)
        self._lib.check(self.L.msm_tica_export_packed(self.h, out.ctypes.data, 0))
        return out

    def reset(self):
        self._lib.check(self.L.msm_tica_reset(self.h))

    def flag(self, name):
        v = C.c_int(-1)
        self._lib.check(getattr(self.L, name)(self.h, C.byref(v)))
        return v.value

    def close(self):
        self._lib.check(self.L.msm_tica_destroy(self.h))
        self.h = None


def host_rows(c, seed=None):
    """The case's trajectories as float64 numpy arrays of the values the device will hold."""
    import torch
    lens = c["lens"]
    seqs = [s[:k] for s, k in zip(_ar1(c["F"] + len(lens) if seed is None else seed, len(lens), max(lens), c["F"]), lens)]
    if c["rows"] == "f64":
        return [s.astype(np.float64) + 1e-9 * np.arange(s.shape[1]) for s in seqs]      # (not representable in float32)
    if c["rows"] == "bf16":
        return [torch.from_numpy(s).to(torch.bfloat16).to(torch.float64).numpy() for s in seqs]
    return [s.astype(np.float64) for s in seqs]


def device_rows(c, host):
    import torch
    dt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}[c["rows"]]
    out = []
    for s in host:
        t = torch.from_numpy(s).to("cuda").to(dt)
        if c["layout"] == "one float in":        # rows of a wider buffer that start one element into it
            buf = torch.zeros(t.shape[0], c["F"] + 4, dtype=dt, device="cuda")
            buf[:, 1:1 + c["F"]] = t
            t = buf[:, 1:1 + c["F"]]
        out.append(t)
    torch.cuda.synchronize()
    return out


_ORACLES = {}


def oracle(c, host, lag=LAG):
    """(C, G, s0, stau, n_observations, n_sequences) in float64; shared by the cases on the same rows."""
    key = (c["F"], c["rows"], tuple((s.shape[0], float(s.sum())) for s in host))
    if key not in _ORACLES:
        F = c["F"]
        Cm, G, s0, st, nobs, nseq = np.zeros((F, F)), np.zeros((F, F)), np.zeros(F), np.zeros(F), 0, 0
        for X in host:
            n = X.shape[0]
            if n <= lag:
                continue
            t = np.arange(n)
            w = (t < n - lag).astype(np.float64) + (t >= lag)
            Cm += X[:-lag].T @ X[lag:]
            G += (X * w[:, None]).T @ X
            s0 += X[:-lag].sum(0)
            st += X[lag:].sum(0)
            nobs, nseq = nobs + n, nseq + 1
        _ORACLES[key] = (Cm, G, s0, st, nobs, nseq)
    return _ORACLES[key]


def check_packed(c, h, packed, ora):
    """h: the handle, or whether its lagged moment is the symmetrised one."""
    F = c["F"]
    Cm, G, s0, st, nobs, nseq = ora
    gotC, gotG = packed[:F * F].reshape(F, F), packed[F * F:2 * F * F].reshape(F, F)
    if h if isinstance(h, bool) else h.flag("msm_tica_lagged_symmetrised"):
        # only the symmetric part of the lagged moment is promised (a launch of such a handle that takes a C/G kernel, as
        # float64 rows of 129 features do, adds the raw moment to it)
        Cm, gotC = 0.5 * (Cm + Cm.T), 0.5 * (gotC + gotC.T)
    tol = dict(rtol=1e-12, atol=1e-9) if c["mode"] == "f64" else dict(rtol=0, atol=ATOL_SCALE[c["mode"]] * np.abs(G).max())
    np.testing.assert_allclose(gotC, Cm, **tol)
    np.testing.assert_allclose(gotG, G, **tol)
    np.testing.assert_allclose(packed[2 * F * F:2 * F * F + F], s0, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(packed[2 * F * F + F:2 * F * F + 2 * F], st, rtol=1e-12, atol=1e-9)
    assert list(packed[-2:]) == [nobs, nseq]


def check_plan(c, h):
    """The handle's last plan: the expected path and flavour, and msm_tica_plan's / the restated dispatch's of its inputs."""
    def sw(name):
        return int(os.environ[name]) if name in os.environ else None
    geom, plan, nchunks, nsuper = R.last_plan(h.h)
    p = dict(zip(R.PLAN_FIELDS, plan))
    assert (R.PATHS[p["path"]], p["flavour"]) == c["want"], (p, geom)
    kw = dict(ptr16=h.launch["ptr16"], ptr16_all=h.launch["ptr16_all"], fold_env=sw("MSM_TICA_FOLD"), fused_env=sw("MSM_TICA_IMG_FUSED"))
    args = (geom, h.launch["dtype_bytes"], h.launch["ld"], h.launch["n_rows"])
    assert R.library_plan(*args, **kw) == plan
    assert R.plan(*args, **kw) == plan
    assert nchunks >= 1
    return geom, p, nchunks, nsuper


@pytest.fixture
def switches(gpu, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def run_case(c):
    """Fresh handle, one launch, plan and oracle checks.  Returns (packed state, (geometry, plan, chunks, super-chunks))."""
    host = host_rows(c)
    dev = device_rows(c, host)
    h = Handle(c["F"], c["mode"])
    try:
        h.accumulate(dev)
        info = check_plan(c, h)
        packed = h.packed()
        check_packed(c, h, packed, oracle(c, host))
        return packed, info
    finally:
        h.close()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_path_and_flavour(switches, c):
    for k, v in c["env"].items():
        switches.setenv(k, v)
    packed, (geom, p, nchunks, nsuper) = run_case(c)
    if c["name"] == "sym-2048-search":
        # one trajectory, no chunk table: the search leaves 4096 (12,500 frames on 3 cohorts: 9 chunks of 1536), and the
        # remainder cohort takes its share of them
        assert p["single"] == 1 and p["kc"] == 1536 and nchunks == 9
        assert R.n_main(p, nchunks) == 8
    if c["want"][0] == "img_fused":
        assert nsuper == 0


def test_carried_pack_and_prepass_agree_bit_for_bit(switches):
    """MSM_TICA_IMG_CARRY=1 (the multiply packs the next super-chunk) against =2 (the same super-chunks, every one packed by
    the pre-pass kernel), on enough frames for two super-chunks at the default ring: the same packets, the same state."""
    out = {}
    for c in CARRY_CASES:
        for k, v in c["env"].items():
            switches.setenv(k, v)
        host = host_rows(c)
        dev = device_rows(c, host)
        h = Handle(c["F"], c["mode"])
        try:
            h.accumulate(dev)
            geom, p, nchunks, nsuper = check_plan(c, h)
            assert nsuper >= 2
            assert h.flag("msm_tica_last_img_carried") == (1 if c["env"]["MSM_TICA_IMG_CARRY"] == "1" else 0)
            out[c["name"]] = h.packed()
            check_packed(c, h, out[c["name"]], oracle(c, host))
        finally:
            h.close()
    assert np.array_equal(out["img-carry-1"], out["img-carry-2"])


def run_segments(c):
    host = host_rows(c)
    dev = device_rows(c, host)
    h = Handle(c["F"], c["mode"])
    try:
        h.accumulate_segments(dev[0], SEGMENTS)
        return h, host, h.packed()
    except Exception:
        h.close()
        raise


@pytest.mark.parametrize("c", SEGMENT_CASES, ids=[c["name"] for c in SEGMENT_CASES])
def test_segments_of_one_trajectory(switches, c):
    """msm_tica_accumulate_segments: three slices that together own every left frame of one trajectory add up to the
    trajectory (the fp32 kernels take one more column-sum pass over the right frames of the owned pairs)."""
    h, host, packed = run_segments(c)
    try:
        geom, plan, nchunks, nsuper = R.last_plan(h.h)
        p = dict(zip(R.PLAN_FIELDS, plan))
        assert (R.PATHS[p["path"]], p["flavour"]) == c["want"]
        # msm_tica_plan takes whole trajectories only: the segments' plan is held to the restated dispatch
        n_rows = [min(oe + LAG, c["lens"][0]) - ob for ob, oe in SEGMENTS]
        segs = [(c["lens"][0], ob, oe) for ob, oe in SEGMENTS]
        assert R.plan(geom, 4, c["F"], n_rows, ptr16=True, segs=segs) == plan
        assert p["single"] == 0 and p["fold"] == 0 and p["total"] == c["lens"][0] and p["nvalid"] == len(SEGMENTS)
        assert p["shifted"] == (0 if c["mode"] == "f64" else 1)
        check_packed(c, h, packed, oracle(c, host))
    finally:
        h.close()


def run_pooled(c, other_seed=7):
    """[state after list A, after A again on the reset handle, after list B of the same lengths] on ONE handle."""
    hostA, hostB = host_rows(c), host_rows(c, seed=other_seed)
    devA, devB = device_rows(c, hostA), device_rows(c, hostB)
    h = Handle(c["F"], c["mode"])
    out = []
    try:
        for dev in (devA, devA, devB):      # the second launch finds the first one's chunk table, the third must not
            h.reset()
            h.accumulate(dev)
            out.append(h.packed())
    finally:
        h.close()
    return out, (hostA, hostB), (devA, devB)


def test_table_cache_hit_then_miss(switches):
    c = case("pooled-512", 512, ("sym", 0))
    out, hosts, devs = run_pooled(c)
    fresh = []
    for dev, host in zip(devs, hosts):
        h = Handle(c["F"], c["mode"])
        try:
            h.accumulate(dev)
            check_plan(c, h)
            fresh.append(h.packed())
            check_packed(c, h, fresh[-1], oracle(c, host))
        finally:
            h.close()
    assert np.array_equal(out[0], fresh[0]) and np.array_equal(out[1], fresh[0]) and np.array_equal(out[2], fresh[1])
    assert not np.array_equal(fresh[0], fresh[1])


def run_nan_then_good(c):
    """Good launch (the slabs are dirty), a launch with one NaN away from the boundary rows (rejected), a good launch."""
    import torch
    host = host_rows(c)
    dev = device_rows(c, host)
    bad = [d.clone() for d in dev]
    bad[1][300, 5] = float("nan")
    torch.cuda.synchronize()
    h = Handle(c["F"], c["mode"])
    try:
        h.accumulate(dev)
        rc = h.accumulate(bad, check=False)
        folded_bad = R.last_plan(h.h)[1][R.PLAN_FIELDS.index("fold")]
        h.accumulate(dev[:2])
        return rc, folded_bad, h.packed(), host, dev
    finally:
        h.close()


def test_rejected_folded_launch_restores_the_slabs(switches):
    from msmbuilder_amd import _lib
    c = case("nan-512-fold", 512, ("sym", R.FL_FOLD), env={"MSM_TICA_FOLD": "2"})
    switches.setenv("MSM_TICA_FOLD", "2")
    rc, folded_bad, packed, host, dev = run_nan_then_good(c)
    assert rc == _lib.MSM_ERR_NONFINITE and folded_bad == 1
    h = Handle(c["F"], c["mode"])
    try:
        h.accumulate(dev)
        h.accumulate(dev[:2])
        check_plan(dict(c, want=("sym", R.FL_FOLD)), h)
        want = h.packed()
    finally:
        h.close()
    assert np.array_equal(packed, want)
    a, b = oracle(c, host), oracle(c, host[:2])
    check_packed(c, True, packed, tuple(x + y for x, y in zip(a, b)))


def test_fold_switch_is_read_per_launch_at_the_default_threshold(switches):
    """131,200 frames of 512 features are 2^26 elements and more: folded column sums by default, the separate column-sum pass
    with MSM_TICA_FOLD=0 (and with a negative value the default again), the same moments either way."""
    import torch
    F, n = 512, 131200
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn(n, F, generator=g, device="cuda") + torch.linspace(-3.0, 3.0, F, device="cuda")
    host = [X.double().cpu().numpy()]
    c = case("fold-switch", F, None, lens=(n,))
    ora = oracle(c, host)
    for value, fold in ((None, 1), ("0", 0), ("-1", 1)):
        if value is None:
            switches.delenv("MSM_TICA_FOLD", raising=False)
        else:
            switches.setenv("MSM_TICA_FOLD", value)
        h = Handle(F, "f32")
        try:
            h.accumulate([X])
            geom, plan, nchunks, nsuper = R.last_plan(h.h)
            p = dict(zip(R.PLAN_FIELDS, plan))
            assert p["total"] * F >= 1 << 26 and R.PATHS[p["path"]] == "sym"
            assert (p["fold"], h.flag("msm_tica_last_folded")) == (fold, fold), value
            assert R.plan(geom, 4, F, [n], fold_env=None if value is None else int(value) if int(value) >= 0 else None) == plan
            check_packed(c, h, h.packed(), ora)
        finally:
            h.close()


def test_fused_kernel_asks_alignment_of_skipped_trajectories_too(switches):
    """bfloat16-stored rows of 512 features take the fused kernel by default -- unless ANY pointer of the table is off a
    16-byte boundary, a skipped trajectory's included: then the image ring."""
    import torch
    c = case("fused-skipped-misaligned", 512, ("img_ring", 0), mode="bf16", rows="bf16")
    host = host_rows(c)
    dev = device_rows(c, host)
    short = torch.zeros(LAG * 512 + 8, dtype=torch.bfloat16, device="cuda")[1:1 + LAG * 512].view(LAG, 512)   # lag rows: skipped
    assert short.data_ptr() % 16 == 2
    h = Handle(c["F"], c["mode"])
    try:
        h.accumulate(dev + [short])
        assert h.launch["ptr16"] and not h.launch["ptr16_all"]
        check_plan(c, h)
        check_packed(c, h, h.packed(), oracle(c, host))
        h.reset()
        h.accumulate(dev)
        check_plan(dict(c, want=("img_fused", 0)), h)
    finally:
        h.close()
