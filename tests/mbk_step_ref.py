"""Exact reference of one MiniBatchKMeans step and of what surrounds it (plain numpy; shares nothing with the kernels).

What is exact, and why:

  * labels     the exact float64 argmin of kmeans_label_ref (lowest index among equals).  The inputs of the tests are
               "blobs" (``gen_blobs``): rows 0.05 sigma around randn centres, initial centres 0.025 sigma off them.  On
               them no row is a near-tie under the labelling rule (``near_ties == 0`` is asserted for every labelled
               batch before a device result is looked at), so the kernels' labels must EQUAL the exact ones on every row.
  * update     scikit-learn's streaming mean (_k_means_minibatch.pyx, unit sample weights) in the rows' own type T:
                   acc = c_j * w_j;  acc = acc + x_b over the members of centre j IN BATCH ORDER;
                   w_new = w_j + T(cnt);  c_new = acc * (T(1) / w_new)
               Every operation is one IEEE operation of T with no freedom of order, so the device's centres and counts
               must be bit-equal (tests/test_mbk_step_ref.py holds this arithmetic to scikit-learn's own
               _mini_batch_step bit for bit).  A centre with no member keeps its bits.
  * batch sums float64, added sequentially in batch order from 0.0: the device's fp64 accumulator is the same chain.
  * inertia    sum_i ||x_i - c_label(i)||^2 in float64 under the PRE-update centres; the device's is held to
               kmeans_label_ref.inertia_rtol (derived there).
  * apply_packed   (c * w + s) / w_new in float64, rounded once to T.  float32 handles: c * w is exact in float64 (24 + 24
               bits), so a fused and an unfused numerator agree and the result is bit-exact.  float64 handles: the
               numerator may or may not be fused; with u = 2^-53 the unfused form errs by at most
               u |c w| + u |c w + s| in the numerator and u |v| in the quotient, the fused form by less, so
                   |got - v| <= 3 u (|c w| + |s|) / w_new < 2^-51 (|c w| + |s|) / w_new      (``apply_packed_bound``)
               against the exact rational v (fractions.Fraction).
  * convergence    scikit-learn's _mini_batch_convergence (tol == 0, not verbose) in Python floats, fed the DEVICE's own
               inertias, so that ``ewa < ewa_min`` never hangs on a rounding difference between device and reference.
"""
import collections
import fractions

import numpy as np

import kmeans_label_ref as R

StepResult = collections.namedtuple("StepResult", "centers counts labels inertia sums cnts near_ties")


def gen_blobs(n, m, K, dtype, seed, spread=0.05):
    """X = C[own] + spread * randn, initial centres C + 0.5 * spread * randn.  Returns X, the initial centres and ``own``."""
    rs = np.random.RandomState(seed)
    C = rs.randn(K, m)
    own = rs.randint(0, K, n)
    X = (C[own] + spread * rs.randn(n, m)).astype(dtype)
    C0 = (C + 0.5 * spread * rs.randn(K, m)).astype(dtype)
    return X, C0, own


def batch_with_counts(own, counts, seed):
    """A shuffled batch index list with exactly counts[j] rows of blob j (drawn with replacement, so rows repeat)."""
    rs = np.random.RandomState(seed)
    parts = []
    for j, c in enumerate(counts):
        if c:
            pool = np.nonzero(own == j)[0]
            assert len(pool), "blob %d has no row" % j
            parts.append(rs.choice(pool, int(c), replace=True))
    idx = np.concatenate(parts)
    rs.shuffle(idx)
    return np.ascontiguousarray(idx, dtype=np.int64)


def step(Xb, C, w):
    """One step on the batch rows Xb from centres C and counts w (all of one type T); nothing is modified."""
    T = Xb.dtype.type
    assert C.dtype == Xb.dtype and w.dtype == Xb.dtype
    B, K = Xb.shape[0], C.shape[0]
    ref, dref, sec, dsec = R.exact_argmin(Xb, C)
    if K > 1:
        rows = np.arange(B)
        u = R.unit_roundoff(Xb.dtype)
        near = float(np.mean(dsec - dref <= R.pair_bound(Xb, C, rows, ref, u) + R.pair_bound(Xb, C, rows, sec, u)))
    else:
        near = 0.0
    inertia = R.exact_inertia(Xb, C, ref)
    acc = C * w[:, None]                       # T(c * w), one rounding
    sums = np.zeros(C.shape, dtype=np.float64)
    X64 = Xb.astype(np.float64)
    for b in range(B):                         # batch order: each centre's members are added in the order they come
        j = ref[b]
        acc[j] = acc[j] + Xb[b]
        sums[j] = sums[j] + X64[b]
    cnt = np.bincount(ref, minlength=K)
    w_new = w + cnt.astype(T)
    hit = cnt > 0
    centers = C.copy()
    counts = w.copy()
    alpha = T(1) / w_new[hit]
    centers[hit] = acc[hit] * alpha[:, None]
    counts[hit] = w_new[hit]
    assert centers.dtype == Xb.dtype and counts.dtype == Xb.dtype
    return StepResult(centers, counts, ref.astype(np.int32), inertia, sums, cnt.astype(np.float64), near)


def apply_packed(C, w, packed):
    """mbk_apply_kernel's computation on packed = [K*m float64 sums | K counts | inertia]: new centres and counts."""
    T = C.dtype.type
    K, m = C.shape
    s = np.asarray(packed[:K * m], dtype=np.float64).reshape(K, m)
    nj = np.asarray(packed[K * m:K * m + K], dtype=np.float64)
    hit = nj > 0.0
    w_new = (w.astype(np.float64) + nj).astype(C.dtype)
    centers, counts = C.copy(), w.copy()
    num = C[hit].astype(np.float64) * w[hit].astype(np.float64)[:, None] + s[hit]
    centers[hit] = (num / w_new[hit].astype(np.float64)[:, None]).astype(C.dtype)
    counts[hit] = w_new[hit]
    assert centers.dtype.type is T
    return centers, counts


def apply_packed_bound(C, w, packed):
    """float64 handles: (v, bound) of the module docstring -- the exact rational value of every updated centre element,
    rounded to float64 for the comparison (one more half ulp of v, which the slack between 3 u and 2^-51 covers), and
    2^-51 (|c w| + |s|) / w_new.  Untouched centres: v = c, bound = 0."""
    K, m = C.shape
    s = np.asarray(packed[:K * m], dtype=np.float64).reshape(K, m)
    nj = np.asarray(packed[K * m:K * m + K], dtype=np.float64)
    v = C.astype(np.float64).copy()
    bound = np.zeros(C.shape)
    F = fractions.Fraction
    for j in np.nonzero(nj > 0.0)[0]:
        wj = F(float(w[j]))
        wn = F(float(np.float64(w[j]) + nj[j]))
        for f in range(m):
            cw = F(float(C[j, f])) * wj
            sf = F(float(s[j, f]))
            v[j, f] = float((cw + sf) / wn)
            bound[j, f] = float((abs(cw) + abs(sf)) / wn) * 2.0 ** -51
    return v, bound


def replay_convergence(inertias, B, alpha, max_no_improvement, first_step, state5):
    """scikit-learn's MiniBatchKMeans._mini_batch_convergence (tol == 0, not verbose) over a run's batch inertias, in
    Python floats and the host's operation order.  state5 = (ewa, ewa_min, no_improvement, have_ewa, have_min) before the
    run; max_no_improvement < 0 or None: never fires.  A step after the one that fires is not executed.  Returns
    (the six state values, steps executed, fired)."""
    ewa, ewa_min, no_imp, have_ewa, have_min = (float(v) for v in state5)
    steps, fired = 0, False
    for s, inertia in enumerate(inertias):
        steps += 1
        if first_step + s == 0:        # "ignore first iteration because it's inertia from initialization"
            continue
        bi = float(inertia) / float(B)
        if have_ewa == 0.0:
            ewa, have_ewa = bi, 1.0
        else:
            ewa = ewa * (1.0 - alpha) + bi * alpha
        if have_min == 0.0 or ewa < ewa_min:
            no_imp, ewa_min, have_min = 0.0, ewa, 1.0
        else:
            no_imp += 1.0
        if max_no_improvement is not None and max_no_improvement >= 0 and no_imp >= max_no_improvement:
            fired = True
            break
    return (ewa, ewa_min, no_imp, have_ewa, have_min, float(steps)), steps, fired


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_mbk_step.py (seeded; tests/test_mbk_step_ref.py asserts on the host that none of them holds
# a near-tie, which is what lets the GPU tests leave no row out)
# ---------------------------------------------------------------------------------------------------------------------
# handle step, B x m x K -> (label kernel, centre splits) that msm_kmeans_label_plan must report, and the update kernel
STEP_F32 = {
    (1000, 10, 1000): ("small", 32, "small"),    # small label kernel with centre splits + wave-per-centre update
    (1024, 32, 40): ("small", 3, "small"),       # small update exactly at its 1,024-row cap
    (1025, 32, 40): ("small", 3, "general"),     # same label kernel, workgroup-per-centre update
    (300, 64, 100): ("label64", 2, "small"),     # 64 x 64 label tiles, small update
    (1024, 512, 257): ("label64", 5, "small"),   # small update: 512 features per round, one round
    (1024, 513, 60): ("label64", 1, "small"),    # second round; odd width: no 16-byte loads in inertia / gather
    (4096, 40, 300): ("label64", 5, "general"),  # exactly one 4,096-row member chunk
    (4097, 40, 300): ("v4", 3, "general"),       # two chunks; split V4 labelling: the inertia kernel merges candidates
    (4200, 260, 130): ("v4", 2, "general"),      # second 256-feature tile of the general update
    (5000, 33, 3): ("scalar", 1, "general"),     # scalar label kernel, no split
    (9000, 3, 2): ("small", 1, "general"),       # small label kernel with the general update, three chunks
}
STEP_F64 = {
    (1000, 10, 1000): ("f64", 8, "small"),
    (1024, 32, 40): ("f64", 1, "small"),
    (1025, 32, 40): ("f64", 1, "general"),
    (1024, 513, 60): ("f64", 1, "small"),
    (4097, 40, 300): ("f64", 3, "general"),
    (4200, 260, 130): ("f64", 2, "general"),
}
# stateless step, B x m x K -> {f64: (label kernel, centre splits)}; the update is always mbk_update_kernel
STATELESS = {
    (700, 300, 129): {False: ("v4", 1), True: ("f64", 2)},
    (1000, 10, 1000): {False: ("scalar", 1), True: ("f64", 8)},
    (4097, 8, 6): {False: ("v4", 1), True: ("f64", 1)},
}
# edges, name -> (B, m, K); both types.  "tails": centres with 0, 1, 2, 3 and 5 members (the 4-wide member tail of the
# small update), B no multiple of 64, initial counts a mix of zeros and integers up to 1e5.  "whole": one centre takes
# the whole batch, initial counts all zero (the first step: c * 0 + sum x).
EDGES = {
    "tails-small": (1003, 32, 40), "whole-small": (1024, 32, 40),
    "tails-general": (4133, 40, 300), "whole-general": (4097, 40, 300),
}
EDGE_PLANS = {
    ("tails-small", False): ("small", 3, "small"), ("whole-small", False): ("small", 3, "small"),
    ("tails-general", False): ("v4", 3, "general"), ("whole-general", False): ("v4", 3, "general"),
    ("tails-small", True): ("f64", 1, "small"), ("whole-small", True): ("f64", 1, "small"),
    ("tails-general", True): ("f64", 3, "general"), ("whole-general", True): ("f64", 3, "general"),
}
# queued runs: name -> (n, m, K, B, S, max_no_improvement, first_step, blob seed); RUN_PLANS: (label kernel, centre splits)
RUNS = {
    "b256": (20000, 10, 50, 256, 12, 10, 0, 1),       # first_step == 0: step 0 is excluded from the average
    "b1024": (20000, 24, 200, 1024, 8, 3, 5, 2),      # first_step > 0 and a carried-over state
    "b2000": (30000, 40, 16, 2000, 6, -1, 0, 3),      # no criterion (max_no_improvement = None)
    "b4100": (8000, 8, 12, 4100, 5, 2, 0, 5),       # stops early at step index 3: 0 < steps_done < S
}
RUN_PLANS = {
    ("b256", False): ("small", 4), ("b1024", False): ("small", 13), ("b2000", False): ("label64", 1),
    ("b4100", False): ("small", 1),
    ("b256", True): ("f64", 1), ("b1024", True): ("f64", 2), ("b2000", True): ("f64", 1), ("b4100", True): ("f64", 1),
}
PROBE_ROWS = 20000


def mixed_counts(K, dtype, seed):
    """Initial counts: about a third zeros, the rest integers up to 1e5 (exact in float32)."""
    rs = np.random.RandomState(seed)
    w = rs.randint(1, 100001, K).astype(dtype)
    w[rs.rand(K) < 0.35] = 0
    w[0] = 0
    w[K - 1] = 100000
    return w


def step_case(B, m, K, dtype, seed=None):
    """Handle / stateless step input: X (n = B + B // 8 rows), C0, w0, batch indices drawn with replacement."""
    seed = B + m + K if seed is None else seed
    n = B + B // 8
    X, C0, _ = gen_blobs(n, m, K, dtype, seed)
    rs = np.random.RandomState(seed + 1)
    idx = np.ascontiguousarray(rs.randint(0, n, B), dtype=np.int64)
    return X, C0, mixed_counts(K, dtype, seed + 2), idx


def edge_case(name, dtype):
    B, m, K = EDGES[name]
    seed = 1000 + B
    X, C0, own = gen_blobs(max(4 * K, 2000), m, K, dtype, seed)
    counts = np.zeros(K, dtype=np.int64)
    if name.startswith("whole"):
        counts[7] = B
        w0 = np.zeros(K, dtype=dtype)
    else:
        counts[:10] = (0, 1, 2, 3, 5, 0, 5, 3, 2, 1)
        rest = B - counts.sum()
        counts[10:] = rest // (K - 10)
        counts[10:10 + rest % (K - 10)] += 1
        w0 = mixed_counts(K, dtype, seed + 2)
    assert counts.sum() == B
    return X, C0, w0, batch_with_counts(own, counts, seed + 1), counts


def run_case(name, dtype):
    """Queued-run input: X, C0, w0 (all zero: a fit's start), the [S][B] batch indices of RandomState(1)."""
    n, m, K, B, S = RUNS[name][:5]
    X, C0, _ = gen_blobs(n, m, K, dtype, seed=RUNS[name][7])
    idx = np.ascontiguousarray(np.random.RandomState(1).randint(0, n, S * B).reshape(S, B), dtype=np.int64)
    return X, C0, np.zeros(K, dtype=dtype), idx


def run_reference(name, dtype, nsteps=None):
    """The reference steps of a queued run, one StepResult per step."""
    X, C, w, idx = run_case(name, dtype)
    out = []
    for s in range(len(idx) if nsteps is None else nsteps):
        r = step(X[idx[s]], C, w)
        out.append(r)
        C, w = r.centers, r.counts
    return out
