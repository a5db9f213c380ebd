"""CPU tier of the tICA launch plan: the library's one dispatch (tica_plan of csrc/tica_plan.h, asked through msm_tica_plan:
needs no device) against the dispatch restated in tests/tica_plan_ref.py, over the full product of the seam values.

The geometry is passed in: 512 and 256 resident slots of every kernel flavour on 256 compute units (512 is what the
comment on the sum/difference kernel's remainder cohort states for the card -- "2,048 features: 104 of 512 slots"; the
function is pure, so both must hold)."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_plan_ref as R  # noqa: E402

SWEEP_F = (1, 3, 4, 16, 17, 96, 97, 128, 129, 256, 257, 260, 512, 768, 2048, 3968, 4096) + (2044,)   # (+ a width with a remainder cohort AND edge tiles)
MODES = (R.F32, R.F64, R.BF16, R.BF16X2)
DTYPES = (2, 4, 8)
SWITCH_FOLD = (None, 0, 2)
SWITCH_FUSED = (None, 0, 1)
SLOTS = (512, 256)
LAG = 10
CHECKED = 242568     # cases of the sweep below: a change of this number is a change of the sweep


def _split(total):
    """`total` frames as three ragged trajectories, every one longer than 2 * LAG."""
    a, b = total // 2, total // 3
    return [a, b, total - a - b]


def launch_shapes(g, S, bk):
    """Row tables on both sides of every threshold of the chunk sizing and the folding rule, for a path of S cohorts and
    K-steps of bk frames: one trajectory (the `single` form) and several."""
    F = g["F"]
    kmin = min(R.KCMAX, max(256, 4 * bk))
    totals = [S * bk, S * bk + 1,                               # kc = ceil(total / S) against one K-step
              S * R.KCMAX, S * R.KCMAX + 1,                     # ... against KCMAX: the load-balance search begins
              int(S * R.KCMAX * 2.5), int(S * R.KCMAX * 7.35),  # ... inside it (sizes other than 4096 win)
              16 * R.KCMAX * S - 1, 16 * R.KCMAX * S,           # ... and where it ends
              R.cdiv(1 << 26, F) - 1, R.cdiv(1 << 26, F),       # total * F = 2^26: the default folding threshold
              8 * S * kmin, 8 * S * kmin + 1]                   # whole-matrix rule: eight chunks per workgroup
    shapes = []
    for t in sorted(set(totals)):
        t = max(t, 8 * LAG)
        shapes += [[t], _split(t)]
    big = 40 * LAG
    shapes += [[LAG, big], [LAG + 1, big], [2 * LAG - 1, big, big], [2 * LAG, big, big],   # both sides of lag and 2 lag
               [8 * LAG] * 4, [8 * LAG - 1] * 4,                # 2 lag nvalid > total / 4: the boundary rows would be a pass
               [LAG], [3, LAG, 0]]                              # nothing valid
    return shapes


def stage(g, dtype_bytes, aligned):
    """(S, bk) of the path this handle takes for these rows, from the reference."""
    p = dict(zip(R.PLAN_FIELDS, R.plan(g, dtype_bytes, g["F"], [50 * LAG], ptr16=aligned)))
    return p["S"], p["bk"]


def test_library_plan_equals_the_restated_dispatch():
    checked, seen, searched = 0, set(), set()
    expect = 0
    for slots, F, mode, sym_env in itertools.product(SLOTS, SWEEP_F, MODES, (None, 0)):
        if sym_env == 0 and mode != R.F32:
            continue                # (MSM_TICA_SYM=0 at create: the fp32 mode's C/G kernel at every width)
        g = R.geometry(F, LAG, mode, slots, sym_env=sym_env)
        for dtype_bytes, aligned in itertools.product(DTYPES, (True, False)):
            if dtype_bytes == 2 and not g["img_on"]:
                continue            # the entry rejects bfloat16 rows on a handle without the image path
            shapes = launch_shapes(g, *stage(g, dtype_bytes, aligned))
            expect += len(shapes) * len(SWITCH_FOLD) * len(SWITCH_FUSED)
            for n_rows, fold, fused in itertools.product(shapes, SWITCH_FOLD, SWITCH_FUSED):
                want = R.plan(g, dtype_bytes, F, n_rows, ptr16=aligned, fold_env=fold, fused_env=fused)
                got = R.library_plan(g, dtype_bytes, F, n_rows, ptr16=aligned, fold_env=fold, fused_env=fused)
                assert got == want, (slots, F, mode, sym_env, dtype_bytes, aligned, fold, fused, n_rows, dict(zip(R.PLAN_FIELDS, got)),
                                     dict(zip(R.PLAN_FIELDS, want)))
                p = dict(zip(R.PLAN_FIELDS, want))
                seen.add((R.PATHS[p["path"]], p["flavour"]))
                if R.PATHS[p["path"]] in ("cg64", "cg32", "sym") and p["total"] < 16 * R.KCMAX * p["S"]:
                    searched.add(p["kc"])
                checked += 1
    assert checked == expect == CHECKED
    assert {s[0] for s in seen} == set(R.PATHS)
    want_flavours = {("none", 0), ("cg64", 0),
                     ("cg32", R.FL_ALIGNED), ("cg32", R.FL_ALIGNED | R.FL_EDGE), ("cg32", R.FL_EDGE),
                     ("sym", 0), ("sym", R.FL_EDGE), ("sym", R.FL_FOLD), ("sym", R.FL_REM), ("sym", R.FL_REM | R.FL_EDGE),
                     ("sym", R.FL_REM | R.FL_FOLD),
                     ("symw", 0), ("symw", R.FL_VEC), ("symw64", 0), ("symw64", R.FL_VEC),
                     ("img_ring", 0), ("img_ring", R.FL_FOLD), ("img_ring", R.FL_X2), ("img_ring", R.FL_X2 | R.FL_FOLD),
                     ("img_fused", 0), ("img_fused", R.FL_X2)}
    assert seen == want_flavours
    assert searched - {4096}, "the load-balance search never left 4096"


@pytest.mark.parametrize("slots", SLOTS)
def test_switches_at_create_change_the_geometry_not_the_rule(slots):
    """MSM_TICA_SYM / MSM_TICA_SYMW / MSM_TICA_SYMW64 are read at create: the geometry they leave takes the 128-wide
    kernels, and the plan of such a geometry is the reference's."""
    for F, envs in itertools.product((96, 128, 256, 260, 512, 2048), ({"sym_env": 0}, {"symw_env": 0}, {"symw64_env": 0})):
        g = R.geometry(F, LAG, R.F32, slots, **envs)
        for dtype_bytes, aligned, n_rows in itertools.product((4, 8), (True, False), ([5000], [700, 1300, 900])):
            want = R.plan(g, dtype_bytes, F, n_rows, ptr16=aligned)
            assert R.library_plan(g, dtype_bytes, F, n_rows, ptr16=aligned) == want
            path = R.PATHS[want[0]]
            if "sym_env" in envs:
                assert path == ("cg32" if dtype_bytes == 4 else "cg64")
            if "symw_env" in envs and dtype_bytes == 4:
                assert path == ("sym" if F > 128 and F % 4 == 0 and aligned else "cg32")
            if "symw64_env" in envs and dtype_bytes == 8:
                assert path == "cg64"


def test_reference_names_the_paths_of_known_shapes():
    """The restated dispatch itself, on shapes whose path the kernels' headers state."""
    def path(F, mode, dtype_bytes, n_rows, **kw):
        p = dict(zip(R.PLAN_FIELDS, R.plan(R.geometry(F, LAG, mode, 512), dtype_bytes, F, n_rows, **kw)))
        return R.PATHS[p["path"]], p["flavour"]
    assert path(512, R.F32, 4, [100000]) == ("sym", 0)
    assert path(512, R.F32, 4, [1000000]) == ("sym", R.FL_FOLD)
    assert path(2048, R.F32, 4, [5000]) == ("sym", R.FL_REM)
    assert path(171, R.F32, 4, [5000]) == ("symw", R.FL_VEC)
    assert path(3, R.F32, 4, [5000]) == ("symw", 0)
    assert path(129, R.F32, 8, [5000]) == ("cg64", 0)
    assert path(4096, R.F32, 4, [5000]) == ("cg32", R.FL_ALIGNED)      # no whole sum/difference cohort is resident
    assert path(512, R.BF16, 2, [5000]) == ("img_fused", 0)
    assert path(768, R.BF16X2, 2, [5000]) == ("img_ring", R.FL_X2)
    assert path(4096, R.BF16, 4, [5000]) == ("cg32", R.FL_ALIGNED)     # 256-wide tiles beyond one resident round
    g = R.geometry(2048, LAG, R.F32, 512)
    assert (g["sym_cohorts"], g["sym_grid"], g["S_sym"]) == (3, 512, 4)   # "2,048 features: 104 of 512 slots, two rounds"
    p = dict(zip(R.PLAN_FIELDS, R.plan(g, 4, 2048, [12500])))
    assert (p["rem_R"], p["rem_rounds"]) == (104, 2)


def test_a_geometry_without_cohorts_is_rejected():
    """msm_tica_plan divides the frames by the cohorts of the chosen path: a geometry no handle can have is an error."""
    for F, mode, field in ((512, R.F32, "sym_cohorts"), (512, R.F32, "S32"), (64, R.F32, "symw_S"), (64, R.F32, "symw_S64"),
                           (512, R.BF16, "S_img"), (130, R.F64, "S64")):
        g = R.geometry(F, LAG, mode, 512)
        R.library_plan(g, 4, F, [5000])
        g[field] = 0
        with pytest.raises(ValueError):
            R.library_plan(g, 4, F, [5000])
