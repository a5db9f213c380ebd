"""Exact replay of the device k-means++ seeding (msmbuilder_amd/csrc/kpp.hip) in int64 numpy, and the inputs on which the
device result is determined to the last bit.  TEST INFRASTRUCTURE, not product code; shares nothing with the kernels.

Why lattice rows make the seeding exact.  Rows with small integer coordinates, |x| <= amp with F (2 amp)^2 < 2^24:

  * every product, dot product and squared norm is an integer below 2^53, so the float64 FMA chains of the thread-per-row
    kernel and the lane-strided and butterfly sums of the wave-per-row kernel give the same integer in any order;
  * ``-2 x.c + |c|^2 + |x|^2`` is the exact squared distance, a non-negative integer below 2^24: the clamp does nothing
    and the rounding to float32 is exact;
  * the running sums (block scan, ``s - v[3]``, block prefix, per-block potentials, their tree sums) are integers below
    2^53: exact in float64 whatever their order.

Two roundings remain, each ONE operation with one possible answer: ``(T)potential`` (float32 rows: the integer total
rounded to float32; float64 rows: exact) and ``u * pot`` in float64.  So the device's ids must equal ``replay``'s id for
id, with no tolerance, and ``centers`` must be the bits of ``X[ids]``.

One round of ``replay`` is scikit-learn's ``_kmeans_plusplus`` (sklearn/cluster/_kmeans.py:163-259) with the caller's
``first`` and uniforms ``u[K - 1][L]``:

    closest   int64 exact squared distances to the nearest chosen centre
    pot       the int sum rounded to dtype
    cand      min(searchsorted(cumsum(closest), u * pot, 'left'), n - 1)
    pots      sum(min(closest, d(cand_j))) rounded to dtype, j = 0 .. L - 1
    winner    the first minimum of pots

tests/test_kpp_ref.py holds the replay to ``sklearn.cluster.kmeans_plusplus`` itself (float64 lattice rows, where
scikit-learn is exact too) and to ``oracle.kpp_oracle.kmeans_plusplus_f64`` (float32 lattice rows), and checks that every
named case of ``CASES`` reaches the path it is named for; tests/test_gpu_kpp.py holds the device to the replay.
"""
import collections
import functools

import numpy as np

RPB = 1024           # rows of a scan block (kpp.hip: KPP_RPB)
NT = 256             # threads of a workgroup (KPP_NT): the pick kernel's prefix gives thread t the blocks [t per, (t + 1) per)
LMAX = 16            # most candidates per round (KPP_LMAX)
TILE_BYTES = 60000   # candidate rows beyond L F sizeof(T) bytes go through a device buffer
LONGPRE_NB = 7168    # more scan blocks than this: the block prefix lives in device memory

_CHUNK = 1 << 22     # elements of one distance chunk


def max_amp(F):
    """The largest amplitude with F (2 amp)^2 < 2^24: every squared distance between rows of |x| <= amp fits float32."""
    amp = int(np.sqrt((2 ** 24 - 1) / F) / 2)
    while F * (2 * (amp + 1)) ** 2 < 2 ** 24:
        amp += 1
    while F * (2 * amp) ** 2 >= 2 ** 24:
        amp -= 1
    assert amp >= 1, "rows too wide for a float32 lattice"
    return amp


def lattice(n, F, seed, dtype, amp=None):
    """[n, F] rows of integers in [-amp, amp] (``RandomState(seed).randint``), amp <= max_amp(F); default min(40, max_amp)."""
    top = max_amp(F)
    amp = min(40, top) if amp is None else amp
    assert 0 <= amp <= top
    return np.random.RandomState(seed).randint(-amp, amp + 1, size=(n, F)).astype(dtype)


def wrapper_draws(n, K, random_state, dtype=np.float64):
    """(first, u, L) exactly as ``minibatchkmeans.kmeans_plusplus`` (and scikit-learn) draws them from ``random_state`` for
    rows of ``dtype``: one ``choice`` under uniform weights of the rows' type, then (K - 1) x L uniforms."""
    L = 2 + int(np.log(K))
    w = np.ones(n, dtype=dtype)
    first = int(random_state.choice(n, p=w / w.sum()))
    u = np.ascontiguousarray(random_state.uniform(size=(max(K - 1, 0), L)), dtype=np.float64)
    return first, u, L


def _as_int(X):
    X = np.asarray(X)
    assert X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] >= 1
    assert np.isfinite(X).all(), "replay: rows must be finite"
    Xi = X.astype(np.int64)
    assert (Xi == X).all(), "replay: rows must be integer-valued (lattice data)"
    return Xi


def _sqdist(Xi, c):
    """int64 exact squared distances of every row to the row c, in row chunks."""
    n, F = Xi.shape
    out = np.empty(n, dtype=np.int64)
    step = max(1, _CHUNK // F)
    for s in range(0, n, step):
        diff = Xi[s:s + step] - c
        out[s:s + step] = np.einsum("ij,ij->i", diff, diff)
    return out


def _round(total, dtype):
    """The integer total rounded once to dtype, as a float64 (what the device keeps in *P.pot)."""
    assert 0 <= total < 2 ** 53, "replay: a running sum reaches 2^53"
    return float(np.float64(int(total)).astype(dtype))


class _State:
    """The seeding after some rounds: ``closest`` (int64), ``pot`` (rounded to dtype) and the ids chosen so far."""

    def __init__(self, X, first, dtype):
        self.dtype = np.dtype(dtype)
        assert self.dtype in (np.dtype(np.float32), np.dtype(np.float64))
        self.Xi = _as_int(X)
        self.n = self.Xi.shape[0]
        assert 0 <= first < self.n
        self.dmax = 2 ** 24 if self.dtype == np.float32 else 2 ** 53
        self.closest = self._dist(first)
        self.pot = _round(self.closest.sum(), self.dtype)
        self.ids = [int(first)]

    def _dist(self, row):
        d = _sqdist(self.Xi, self.Xi[row])
        assert int(d.max()) < self.dmax, "replay: a squared distance does not fit the rows' type exactly"
        return d

    def cum(self):
        c = np.cumsum(self.closest)
        assert int(c[-1]) < 2 ** 53, "replay: a running sum reaches 2^53"
        return c.astype(np.float64)   # exact

    def draw(self, cumf, u_row):
        """(targets r = u * pot, searchsorted index before the clip)."""
        r = np.asarray(u_row, dtype=np.float64) * np.float64(self.pot)
        return r, np.searchsorted(cumf, r, side="left")

    def advance(self, cand):
        """Evaluate the candidates; returns (pots rounded to dtype as float64, winner slot)."""
        ds, pots = [], []
        memo = {}
        for c in cand:
            c = int(c)
            if c not in memo:
                d = np.minimum(self.closest, self._dist(c))
                memo[c] = (d, _round(d.sum(), self.dtype))
            ds.append(memo[c][0])
            pots.append(memo[c][1])
        pots = np.asarray(pots)
        b = int(np.argmin(pots))   # first minimum
        self.closest, self.pot = ds[b], float(pots[b])
        self.ids.append(int(cand[b]))
        return pots, b


def _new_stats():
    return dict(clipped=0,            # draws beyond the last bin, clipped to n - 1
                clipped_visible=0,    # ... where row n - 1 has zero width: without the clip rule another row would be drawn
                tied_rounds=0,        # rounds whose minimal potential is shared by two slots or more
                tied_distinct=0,      # ... of which the first and the last minimum are different rows
                zero_bin=0,           # candidates on a row of zero width (a row that coincides with a chosen centre)
                zero_pot_rounds=0,    # rounds that start at potential 0
                on_edge=0,            # draws with u * pot == cum[cand] exactly (pot > 0)
                flat_edge=0,          # ... followed by a zero-width row: side='right' would skip the flat stretch
                edge_block_last=0,    # ... on the last row of a block: u * pot equals the block's inclusive prefix
                edge_block_first=0,   # ... on the first row of a block other than block 0
                edge_chunk_last=0,    # ... on the last row of the last block of a pick-kernel chunk (per >= 2)
                block_last=0,         # candidates on the last row of a 1024-row block
                block_first=0,        # candidates on the first row of a block other than block 0
                quad_last=0,          # candidates on the last row of a scan thread's quad
                chunk_last=0,         # candidates on the last row of the last block of a pick-kernel chunk (per >= 2)
                cands=[])             # [K - 1][L] the candidates of every round


def replay(X, K, first, u, dtype):
    """ids [K] (int64) of the seeding of the lattice rows X in the arithmetic of ``dtype``, and what the case exercised."""
    st = _State(X, first, dtype)
    n = st.n
    assert 1 <= K <= n
    nb = -(-n // RPB)
    per = -(-nb // NT)
    stats = _new_stats()
    if K > 1:
        u = np.asarray(u, dtype=np.float64)
        assert u.ndim == 2 and u.shape[0] == K - 1 and 1 <= u.shape[1] <= LMAX
        assert ((0 <= u) & (u < 1)).all()
    for rnd in range(K - 1):
        cumf = st.cum()
        r, raw = st.draw(cumf, u[rnd])
        cand = np.minimum(raw, n - 1)
        zero_pot = st.pot == 0
        stats["zero_pot_rounds"] += int(zero_pot)
        for rj, ij, cj in zip(r, raw, cand):
            if ij >= n:
                stats["clipped"] += 1
                stats["clipped_visible"] += int(st.closest[n - 1] == 0)
                continue
            stats["zero_bin"] += int(st.closest[cj] == 0)
            edge = not zero_pot and rj == cumf[cj]
            blast, bfirst = cj % RPB == RPB - 1, cj % RPB == 0 and cj > 0
            clast = per >= 2 and blast and (cj // RPB) % per == per - 1
            if edge:
                stats["on_edge"] += 1
                stats["flat_edge"] += int(cj + 1 < n and st.closest[cj + 1] == 0)
                stats["edge_block_last"] += int(blast)
                stats["edge_block_first"] += int(bfirst)
                stats["edge_chunk_last"] += int(clast)
            stats["block_last"] += int(blast)
            stats["block_first"] += int(bfirst)
            stats["quad_last"] += int(cj % 4 == 3)
            stats["chunk_last"] += int(clast)
        pots, b = st.advance(cand)
        tied = np.nonzero(pots == pots[b])[0]
        if len(tied) > 1:
            stats["tied_rounds"] += 1
            stats["tied_distinct"] += int(cand[tied[-1]] != cand[b])
        stats["cands"].append(cand.copy())
    return np.asarray(st.ids, dtype=np.int64), stats


Planned = collections.namedtuple("Planned", "round slot want row kind")   # kind: 'edge' (u pot == cum[row]) or 'above'


def _edge_pair(cumf, closest, pot, i):
    """(row, u, u_above): a row of non-zero width at or next to i whose bin edge is hit exactly, ``u * pot == cum[row]`` in
    float64, and the next uniform above it whose product exceeds the edge.  None if no row within 8 of i allows it."""
    n = len(cumf)
    for k in (0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7, -8, 8):
        row = i + k
        if not 0 <= row < n or closest[row] == 0:
            continue
        c = cumf[row]
        if not 0 < c <= pot:
            continue
        u0 = c / pot
        for v in (u0, np.nextafter(u0, 0.0), np.nextafter(u0, 1.0)):
            if not (0 <= v < 1 and v * pot == c):
                continue
            w = v
            for _ in range(4):
                w = np.nextafter(w, 1.0)
                if w * pot > c:
                    break
            if w < 1 and w * pot > c:
                return row, float(v), float(w)
    return None


def edge_uniforms(X, K, L, first, targets, dtype=None, seed=0):
    """u [K - 1][L] built round by round so that chosen draws land exactly on a bin edge and on the next float above it.

    Slots (2m, 2m + 1) of a round take the next target row i of ``targets`` (cycled): slot 2m gets u with
    ``u * pot == cum[i]`` exactly in float64 -- side='left' lands on row i, side='right' would not -- and slot 2m + 1 the
    next float64 above it whose product exceeds cum[i], which lands on the next row of non-zero width.  A target whose
    product cannot be made exact, or whose row has zero width, moves to a neighbouring row.  Every other slot (an odd L's
    last one, a round at potential 0) keeps a uniform of ``RandomState(seed)``.  Returns (u, plan): plan lists the
    constructed draws as ``Planned(round, slot, want, row, kind)`` with the row each must land on."""
    dtype = np.asarray(X).dtype if dtype is None else dtype
    st = _State(X, first, dtype)
    assert 1 <= L <= LMAX and 1 <= K <= st.n
    u = np.ascontiguousarray(np.random.RandomState(seed).uniform(size=(max(K - 1, 0), L)))
    plan, t = [], 0
    for rnd in range(K - 1):
        cumf = st.cum()
        if st.pot > 0:
            for m in range(L // 2):
                want = int(targets[t % len(targets)])
                t += 1
                got = _edge_pair(cumf, st.closest, np.float64(st.pot), want)
                if got is None:
                    continue
                row, v, w = got
                u[rnd, 2 * m], u[rnd, 2 * m + 1] = v, w
                above = min(int(np.searchsorted(cumf, w * np.float64(st.pot), side="left")), st.n - 1)
                plan.append(Planned(rnd, 2 * m, want, row, "edge"))
                plan.append(Planned(rnd, 2 * m + 1, want, above, "above"))
        _, raw = st.draw(cumf, u[rnd])
        st.advance(np.minimum(raw, st.n - 1))
    return u, plan


def seam_targets(n):
    """Rows whose bin edges matter to the scan and pick kernels of an n-row sample, the most telling first (a case with few
    rounds uses only the head of the list): the last row of the last full block; where the pick kernel gives a thread
    ``per`` >= 2 blocks, the last row of a chunk in the middle, of the last whole chunk and of a block inside a chunk; the
    first row of a block; block 0's last row and its successor; a middle block's; the last row of a scan thread's quad; the
    last row."""
    nb = -(-n // RPB)
    per = -(-nb // NT)
    full = n // RPB   # whole blocks
    last = lambda b: b * RPB + RPB - 1
    rows = [last(full - 1)]                                       # 'above' lands in the part block behind it, if any
    if per >= 2:
        whole = nb // per   # whole chunks
        rows += [last((whole // 2) * per + per - 1), last(whole * per - 1), last((whole // 2) * per)]
    rows += [last(full - 1) + 1, last(0), last(0) + 1, last(full // 2), 5 * RPB + 7, n - 1]
    seen, out = set(), []
    for r in rows:
        if 0 <= r < n and r not in seen:
            seen.add(r)
            out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The case table, shared by tests/test_kpp_ref.py (CPU: the replay is honest, every case reaches its path) and
# tests/test_gpu_kpp.py (the device equals the replay).
#
#   rows     'lattice' (seed, amp) | 'same' (every row the same lattice row)
#            | 'dup_last' (lattice, then row n - 1 := row `first`: the last bin has zero width)
#   draws    'random' (RandomState(seed + 1000).uniform) | 'edge' (edge_uniforms on seam_targets(n)) | 'zero' (u = 0)
#            | 'clip' (u[:, 0] = 0, u[:, -1] = 1 - 2^-53)
#   L        None: 2 + int(log K), the wrapper's
#   expect   {stat: minimum}, asserted on the CPU tier for every dtype of the case
Case = collections.namedtuple("Case", "name n F K L first rows seed amp draws dtypes expect small")
BOTH = ("float32", "float64")


def _case(name, n, F, K, L=None, first=0, rows="lattice", seed=0, amp=None, draws="random", dtypes=BOTH, expect=None,
          small=False):
    return Case(name, n, F, K, L, first, rows, seed, amp, draws, tuple(dtypes), dict(expect or {}), small)


CLIP_VISIBLE_SEED = 0   # a seed whose total rounds up in float32 (asserted through `expect` on the CPU tier)


def _table():
    t = []
    # n seams on thread-per-row rows: one block, the 1024-row scan block either side, a part block, K == n for the small
    for F in (1, 3):
        for i, n in enumerate((1, 2, 1023, 1024, 1025, 1281, 2047)):
            K = n if n <= 2 else 7
            t.append(_case("n%d_F%d" % (n, F), n, F, K, first=(0, n - 1, n // 2)[(i + F) % 3], seed=10 + i, small=True))
    t.append(_case("k_equals_n_narrow", 50, 2, 50, first=49, amp=1, seed=3, small=True,
                   expect=dict(tied_rounds=1, tied_distinct=1, zero_pot_rounds=1, zero_bin=1)))
    t.append(_case("k_equals_n_wave", 40, 32, 40, first=20, amp=1, seed=4, small=True))
    # F seams: the kernel switch at 32, the lane stride at 64, the gather stride at 256, 16-byte loads (F % 4 == 0 for
    # float32, F % 2 == 0 for float64) and not
    for F in (31, 32, 33, 34, 63, 64, 65, 257):
        t.append(_case("F%d" % F, 300, F, 6, first=299 if F % 2 else 150, seed=20 + F, small=F <= 65))
    # the 32 rows of a wave-per-row workgroup
    for n in (31, 32, 33):
        for F in (32, 33):
            t.append(_case("wave_n%d_F%d" % (n, F), n, F, 5, first=n - 1, seed=30 + n, small=True))
    # L seams through the C entry
    for L in (1, 16):
        t.append(_case("L%d_narrow" % L, 1500, 3, 5, L=L, first=700, seed=40 + L))
        t.append(_case("L%d_wave" % L, 200, 40, 5, L=L, first=199, seed=42 + L))
    # either side of the 60,000-byte staging tile at L = 16 (937 x 16 x 4 = 59,968; 938 x 16 x 4 = 60,032; 468 / 469 x 16 x 8)
    for F in (937, 938, 940):
        t.append(_case("tile_F%d" % F, 300, F, 5, L=16, first=7, seed=50, dtypes=("float32",)))
    for F in (468, 469, 470):
        t.append(_case("tile_F%d" % F, 300, F, 5, L=16, first=7, seed=51, dtypes=("float64",)))
    # bin edges at block, quad and chunk boundaries
    edge = dict(on_edge=10, edge_block_last=1, edge_block_first=1, block_first=2, quad_last=1)
    t.append(_case("edge_small", 2500, 2, 6, L=4, first=5, seed=60, draws="edge", expect=edge))
    # the pick kernel's chunked prefix: nb = 256 (per = 1), 257 (per = 2, thread 128 owns one block), 513 (per = 3, threads
    # 171 .. 255 own none), 514 (per = 3, thread 171 owns one block: 525,313 rows = 513 full blocks and one row)
    chunk = dict(edge, edge_chunk_last=1)
    t.append(_case("pick_nb256", 262144, 2, 6, L=4, first=5, seed=61, draws="edge", expect=edge))
    t.append(_case("pick_nb257", 262145, 2, 6, L=4, first=262144, seed=62, draws="edge", expect=chunk))
    t.append(_case("pick_nb513", 525312, 2, 6, L=4, first=5, seed=64, draws="edge", dtypes=("float32",), expect=chunk))
    t.append(_case("pick_nb514", 525313, 2, 6, L=4, first=5, seed=63, draws="edge", expect=chunk))
    # the block prefix in device memory: nb = 7168 keeps it in LDS, 7169 does not
    # (the seeds are ones at which both constructed edges could be kept on their target rows)
    for nb, n, seed in ((7168, 7340032, 65), (7169, 7340033, 66)):
        t.append(_case("longpre_nb%d" % nb, n, 1, 3, L=2, first=5, seed=seed, amp=2000, draws="edge", dtypes=("float32",),
                       expect=dict(on_edge=2, edge_block_last=2, edge_chunk_last=1, block_first=1)))
    # ties, duplicates, zero potential
    t.append(_case("all_rows_equal", 1100, 3, 6, first=600, rows="same", seed=70,
                   expect=dict(zero_pot_rounds=5, tied_rounds=5, zero_bin=5)))
    t.append(_case("ties_amp2", 1025, 2, 40, first=1024, amp=2, seed=71, small=True,
                   expect=dict(tied_rounds=1, tied_distinct=1, zero_pot_rounds=1)))
    # u = 0 with row 0 the first centre: side='left' keeps drawing row 0, a bin of zero width, and with L = 1 it is the pick
    t.append(_case("zero_u_first0", 1500, 3, 4, L=1, first=0, seed=72, draws="zero", expect=dict(zero_bin=3)))
    # the clip: a float32 potential rounded UP exceeds the float64 total, and u close to 1 falls beyond the last bin
    for seed in (0, 4):
        t.append(_case("clip_seed%d" % seed, 300000, 2, 3, L=2, first=5, seed=seed, draws="clip", dtypes=("float32",),
                       expect=dict(clipped=1)))
    # ... with L = 1, so the clipped draw IS the pick, and row n - 1 a copy of the first centre: a draw that is not clipped
    # lands on the last row of non-zero width instead, a different id
    t.append(_case("clip_visible", 300000, 2, 3, L=1, first=5, rows="dup_last", seed=CLIP_VISIBLE_SEED, draws="clip",
                   dtypes=("float32",), expect=dict(clipped=1, clipped_visible=1)))
    return t


CASES = collections.OrderedDict((c.name, c) for c in _table())
assert len(CASES) == len(_table())


def case_ids():
    return [(c.name, d) for c in CASES.values() for d in c.dtypes]


@functools.lru_cache(maxsize=8)
def case_inputs(name, dtype):
    """(X, K, first, u, L, plan) of a case for rows of ``dtype``; plan is edge_uniforms' (empty for other draws)."""
    c = CASES[name]
    K = c.K
    L = c.L if c.L is not None else 2 + int(np.log(K))
    X = lattice(c.n, c.F, c.seed, dtype, c.amp)
    if c.rows == "same":
        X[:] = X[0]
    elif c.rows == "dup_last":
        X[c.n - 1] = X[c.first]
    else:
        assert c.rows == "lattice"
    plan = []
    if c.draws == "random":
        u = np.ascontiguousarray(np.random.RandomState(c.seed + 1000).uniform(size=(max(K - 1, 0), L)))
    elif c.draws == "clip":
        u = np.ascontiguousarray(np.random.RandomState(c.seed + 1000).uniform(size=(K - 1, L)))
        u[:, 0] = 0.0
        u[:, -1] = 1.0 - 2.0 ** -53
    elif c.draws == "zero":
        u = np.zeros((K - 1, L))
    else:
        assert c.draws == "edge"
        u, plan = edge_uniforms(X, K, L, c.first, seam_targets(c.n), dtype, seed=c.seed + 1000)
    X.setflags(write=False)
    u.setflags(write=False)
    return X, K, c.first, u, L, tuple(plan)


@functools.lru_cache(maxsize=None)
def case_replay(name, dtype):
    """(ids, stats) of a case, computed once per session and shared; the ids array is read-only."""
    X, K, first, u, L, _ = case_inputs(name, dtype)
    ids, stats = replay(X, K, first, u, dtype)
    ids.setflags(write=False)
    return ids, stats
