"""CPU tier of the sum/difference kernel's unit table (csrc/tica_sym_units.h, asked through msm_tica_sym_units: needs no
device): which workgroup of a cohort computes which 64 x 64 blocks of H and D, unpacked (one workgroup per upper tile) and
packed (the diagonal tiles of a group of four share out the blocks of one of them).

Nothing here is derived from the header: the needed blocks are restated from what tica_export_sym_kernel reads -- every
block of an off-diagonal upper tile, and the blocks (0,0), (0,1), (1,1) of a diagonal one.

Also the chunk walks of a packed launch (tica_sym_walk through msm_tica_sym_walk): every chunk once; the groups of chunks that
share an fp32 partial are a strided geometry's, restated here from the kernel's chunk loop -- the packed cohorts' own, or the
unpacked cohorts' where that costs nothing; and the fullest packed cohort is never heavier than the plain stride's by more
than 1 %, at the sizes where a partial is a coarse granule included."""
import ctypes as C

import pytest

UNIT_INTS = 23      # X, Y, colsum, 4 x {row panel, row offset, column panel, column offset, slab tile}
TS = range(2, 65)


def units(T, pack):
    from msmbuilder_amd import _lib
    L = _lib.lib()
    n = L.msm_tica_sym_units(T, pack, None, 0)
    assert n > 0
    buf = (C.c_int * (n * UNIT_INTS))()
    assert L.msm_tica_sym_units(T, pack, buf, n) == n
    v = list(buf)
    out = []
    for u in range(n):
        r = v[u * UNIT_INTS:(u + 1) * UNIT_INTS]
        waves = [dict(zip(("row_panel", "row_off", "col_panel", "col_off", "slab_tile"), r[3 + 5 * w:8 + 5 * w])) for w in range(4)]
        out.append(dict(X=r[0], Y=r[1], colsum=r[2], waves=waves))
    return out


def slab_tile(T, I, J):
    """Index of the upper tile (I, J) in the row-major order of the upper triangle."""
    return sum(T - i for i in range(I)) + (J - I)


def needed_blocks(T):
    """{(slab tile, row offset, column offset)} the export reads."""
    need = set()
    for I in range(T):
        for J in range(I, T):
            for ro in (0, 64):
                for co in (0, 64):
                    if I < J or ro <= co:
                        need.add((slab_tile(T, I, J), ro, co))
    return need


def owned_blocks(T, table):
    """[(slab tile, row offset, column offset)] of every wave, with the tile checked against the panels the wave reads."""
    tiles = {slab_tile(T, I, J): (I, J) for I in range(T) for J in range(I, T)}
    owned = []
    for u in table:
        assert 0 <= u["X"] < T and 0 <= u["Y"] < T
        assert len(u["waves"]) == 4
        for w in u["waves"]:
            assert w["row_panel"] in (0, 1) and w["col_panel"] in (0, 1)
            assert w["row_off"] in (0, 64) and w["col_off"] in (0, 64)
            rows = u["Y"] if w["row_panel"] else u["X"]      # every wave's panels are its unit's X or Y tile ...
            cols = u["Y"] if w["col_panel"] else u["X"]
            assert tiles[w["slab_tile"]] == (rows, cols)     # ... and they are the rows and columns of the slab tile it merges into
            owned.append((w["slab_tile"], w["row_off"], w["col_off"]))
    return owned


@pytest.mark.parametrize("pack", (0, 1))
def test_every_needed_block_has_exactly_one_owner(pack):
    for T in TS:
        table = units(T, pack)
        owned = owned_blocks(T, table)
        need = needed_blocks(T)
        got = [b for b in owned if b in need]
        assert len(got) == len(set(got)), (T, pack)          # no needed block twice
        assert set(got) == need, (T, pack)                   # ... and none missing
        spare = [b for b in owned if b not in need]          # the mirrored corner of a diagonal tile nobody packed
        assert len(spare) == len(set(spare)) == (T if not pack else T % 4), (T, pack)
        assert len(owned) == 4 * len(table)


@pytest.mark.parametrize("pack", (0, 1))
def test_every_column_block_has_one_column_sum_writer(pack):
    for T in TS:
        writers = [u["X"] for u in units(T, pack) if u["colsum"]]
        assert sorted(writers) == list(range(T)), (T, pack)
        assert all(u["colsum"] in (0, 1) for u in units(T, pack))


def test_unpacked_table_is_the_row_major_upper_triangle():
    for T in TS:
        table = units(T, 0)
        assert [(u["X"], u["Y"]) for u in table] == [(I, J) for I in range(T) for J in range(I, T)]
        for t, u in enumerate(table):
            assert u["colsum"] == int(u["X"] == u["Y"])
            assert u["waves"] == [dict(row_panel=0, row_off=64 * (w >> 1), col_panel=1, col_off=64 * (w & 1), slab_tile=t)
                                  for w in range(4)]


def test_packed_table_drops_one_unit_per_group_of_four_diagonal_tiles():
    for T in TS:
        table = units(T, 1)
        assert len(table) == T * (T + 1) // 2 - T // 4
        assert len(units(T, 0)) == T * (T + 1) // 2
        # the groups: donor 4g + 1 has no unit of its own, the three others stage it as Y and give it wave 3
        pairs = [(u["X"], u["Y"]) for u in table]
        for g in range(T // 4):
            d = 4 * g + 1
            assert (d, d) not in pairs
            lent = []
            for X in (4 * g, 4 * g + 2, 4 * g + 3):
                u = table[pairs.index((X, d))]
                own = slab_tile(T, X, X)
                assert [(w["row_panel"], w["row_off"], w["col_panel"], w["col_off"], w["slab_tile"]) for w in u["waves"][:3]] == \
                    [(0, 0, 0, 0, own), (0, 0, 0, 64, own), (0, 64, 0, 64, own)]
                w = u["waves"][3]
                assert (w["row_panel"], w["col_panel"], w["slab_tile"]) == (1, 1, slab_tile(T, d, d))
                lent.append((w["row_off"], w["col_off"]))
            assert lent == [(0, 0), (0, 64), (64, 64)]
        for I in range(4 * (T // 4), T):                      # the T mod 4 last diagonal tiles stay whole
            assert (I, I) in pairs
        # every unit of a whole tile is the unpacked table's, but for the donor's column sums on (d, d + 1)
        plain = {(u["X"], u["Y"]): u for u in units(T, 0)}
        donors = {4 * g + 1 for g in range(T // 4)}
        for u in table:
            if u["waves"][3]["row_panel"] == 0:
                want = dict(plain[(u["X"], u["Y"])])
                if u["X"] in donors and u["Y"] == u["X"] + 1:
                    want["colsum"] = 1
                assert u == want


def test_bad_arguments_are_rejected():
    from msmbuilder_amd import _lib
    L = _lib.lib()
    assert L.msm_tica_sym_units(0, 1, None, 0) < 0
    assert L.msm_tica_sym_units(4, 1, None, 3) < 0
    buf = (C.c_int * (2 * UNIT_INTS))()
    assert L.msm_tica_sym_units(4, 1, buf, 2) == 9         # a short buffer gets the first units, the count is the table's
    assert list(buf)[:2] == [0, 1]


def walk(rows, S0, S, kc, kflush):
    """(the cohorts' walks as [(chunk, merges after it)], whether the unpacked partials were kept)"""
    from msmbuilder_amd import _lib
    cap = S + 1 + len(rows)
    buf = (C.c_int * cap)()
    arr = (C.c_int * max(1, len(rows)))(*rows)
    kept = _lib.lib().msm_tica_sym_walk(arr, len(rows), S0, S, kc, kflush, buf, cap)
    assert kept in (0, 1)
    v = [x & 0xffffffff for x in buf]
    off, ent = v[:S + 1], v[S + 1:]
    return [[(e & 0x7fffffff, e >> 31) for e in ent[off[s]:off[s + 1]]] for s in range(S)], kept


def strided_partials(rows, stride, kc, kflush):
    """The groups of chunks between two merges of the kernel, per cohort: cohort v of `stride` walks v, v + stride, ... and
    merges when another kc frames would pass kflush, or at its last chunk (restated from tica_sym_f32_kernel's chunk loop)."""
    cohorts = []
    for v in range(min(stride, len(rows))):
        acc, group, groups = 0, [], []
        for c in range(v, len(rows), stride):
            group.append(c)
            acc += rows[c]
            if acc + kc > kflush or c + stride >= len(rows):
                groups.append(tuple(group))
                acc, group = 0, []
        cohorts.append(groups)
    return cohorts


def load(rows, chunks):
    return sum(rows[c] + 16 for c in chunks)       # frames + the prologue of a chunk, as the plan's balance search counts


def chunked(total, S, bk=32, kcmax=4096):
    """One trajectory of `total` frames cut as the plan cuts it for S cohorts (kc = total / S in K-steps, at most 4096)."""
    kc = min(kcmax, max(bk, -(-(-(-total // S)) // bk) * bk))
    nch = -(-total // kc)
    piece = -(-(-(-total // nch)) // bk) * bk
    return [min(piece, total - r) for r in range(0, total, piece)], kc


def walk_cases():
    import random
    rnd = random.Random(5)
    cases = [([3360, 3360, 3280] * 1000, 51, 56, 4096, 8192), ([3360, 3360, 3280] * 1000, 51, 56, 4096, 4096),
             ([4096] * 700 + [17], 14, 15, 4096, 8192), ([32] * 5, 24, 25, 32, 8192), ([], 51, 56, 4096, 8192), ([700], 34, 36, 704, 8192)]
    cases += [([rnd.randint(1, 2048) for _ in range(rnd.randint(1, 900))], 34, 36, 2048, 8192) for _ in range(5)]
    # small and medium launches, where a group of up to kflush frames is a coarse granule: one trajectory of 100k .. 2M
    # frames, and 50 / 100 / 200 trajectories of 10,000, at the cohorts of 512 and 1,024 features
    for S0, S in ((51, 56), (14, 15)):
        for total in (100000, 200000, 500000, 1000000, 2000000):
            rows, kc = chunked(total, S)
            cases.append((rows, S0, S, kc, 8192))
        for n_seq in (50, 100, 200):
            kc = min(4096, -(-(-(-n_seq * 10000 // S)) // 32) * 32)
            rows = chunked(10000, 1, kcmax=kc)[0] * n_seq
            cases.append((rows, S0, S, kc, 8192))
        cases.append(([rnd.randint(11, 700) for _ in range(200)], S0, S, min(4096, 32 * -(-(70000 // S) // 32)), 8192))
    return cases


def test_packed_walk_is_a_strided_geometrys_partials_and_never_heavier_than_the_plain_stride():
    kept_some, strode_some = False, False
    for rows, S0, S, kc, kflush in walk_cases():
        w, kept = walk(rows, S0, S, kc, kflush)
        assert len(w) == S
        assert sorted(c for cohort in w for c, _ in cohort) == list(range(len(rows)))      # every chunk once
        got = []
        for cohort in w:
            groups, group = [], []
            for c, merge in cohort:
                group.append(c)
                if merge:
                    groups.append(tuple(group))
                    group = []
            assert not group                                     # a cohort's walk ends on a merge
            got.append(groups)
        own, unpacked = strided_partials(rows, S, kc, kflush), strided_partials(rows, S0, kc, kflush)
        stride_worst = max([load(rows, [c for g in cohort for c in g]) for cohort in own] or [0])
        worst = max(load(rows, [c for g in cohort for c in g]) for cohort in got)
        if kept:       # the unpacked cohorts' partials, whole, and it cost at most 1 % of the fullest cohort
            assert sorted(g for cohort in got for g in cohort) == sorted(g for cohort in unpacked for g in cohort)
            assert worst * 100 <= stride_worst * 101
            kept_some = True
        else:          # the packed cohorts stride themselves
            assert got[:len(own)] == own and not any(got[len(own):])
            strode_some = True
        # ... so where the chunks are about equal (one trajectory, or equal ones: with ragged chunks which stride is luckier is
        # chance) the fullest packed cohort is no heavier than the fullest of the fewer unpacked cohorts
        unpacked_worst = max([load(rows, [c for g in cohort for c in g]) for cohort in unpacked] or [0])
        if rows and 4 * min(rows) >= 3 * max(rows):
            assert worst * 100 <= unpacked_worst * 101, (len(rows), S0, S, kc)
    assert kept_some and strode_some


def test_bench_sized_walk_keeps_the_unpacked_partials():
    """10M frames as 1,000 trajectories of 10,000 on 56 cohorts (51 unpacked): the partials of the unpacked cohorts are kept."""
    rows = [3360, 3360, 3280] * 1000
    assert walk(rows, 51, 56, 4096, 8192)[1] == 1
    assert walk(chunked(100000, 56)[0], 51, 56, chunked(100000, 56)[1], 8192)[1] == 0       # 56 chunks: the cohorts stride


def test_walk_rejects_a_short_buffer():
    from msmbuilder_amd import _lib
    rows = (C.c_int * 3)(5, 5, 5)
    buf = (C.c_int * 8)()
    assert _lib.lib().msm_tica_sym_walk(rows, 3, 2, 4, 32, 8192, buf, 7) < 0
    assert _lib.lib().msm_tica_sym_walk(rows, 3, 2, 4, 32, 8192, buf, 8) in (0, 1)
