"""Timings of the kernel feature map at 1M x 64 float32 rows, L = 512 (profiles/nystroem_probe.txt): the fused map, the scratch
route, the folded KernelTICA.transform against the unfused composition, and scikit-learn on the host as context.

Usage:  python scripts/nystroem_probe.py [output file]      (PROBE_N=rows for a smaller run)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, F, L, K = int(os.environ.get("PROBE_N", 1000000)), 64, 512, 10
OUT = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=5, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return np.array(ts)


def fmt(ts):
    return "median %.2f ms (min %.2f, max %.2f, %d runs)" % (np.median(ts), ts.min(), ts.max(), len(ts))


def main():
    import torch
    from msmbuilder_amd import KernelTICA, LandmarkNystroem, tICA
    from msmbuilder_amd.decomposition import kernel_approximation as ka
    rs = np.random.RandomState(0)
    # a slow 4-dimensional latent walk seen through 64 channels, so that the tICA behind the folded transform is a real one
    z = np.cumsum(rs.randn(N, 4).astype(np.float32) * 0.02, axis=0)
    z = np.sin(z)
    Xh = (z @ rs.randn(4, F).astype(np.float32) + 0.3 * rs.randn(N, F).astype(np.float32)).astype(np.float32)
    lm = np.ascontiguousarray(Xh[rs.permutation(N)[:L]])
    X = torch.as_tensor(Xh, device="cuda")
    say("Nystroem kernel feature map on one MI355X (msm_kernel_map_f32; DESIGN 3.4b), written by scripts/nystroem_probe.py")
    say("%d x %d float32 rows on the device, L = %d landmarks, rbf, gamma = 1/F" % (N, F, L))
    say("every time is the wall clock around a CALL that ends in a stream synchronise (uploads of landmarks and B, launches,")
    say("synchronise), not a kernel time; no counters were taken.  Per figure: three rounds that alternate the two variants,")
    say("each round one warm-up call and two timed calls per variant (six timed calls each).  flop = 2 N L F + 2 N L^2 as the")
    say("algorithm needs them (kernel functions not counted); 'call rate' = flop / call time.")
    say("plan: %r" % (ka.kernel_map_plan(L, L, F, 4),))
    ny = LandmarkNystroem(landmarks=lm).fit([X[:10]])
    flop1, flop2 = 2.0 * N * L * F, 2.0 * N * L * L

    def run_map():
        return ny.transform([X])[0]

    os.environ.pop("MSM_NYSTROEM_FUSED", None)
    a = run_map()
    os.environ["MSM_NYSTROEM_FUSED"] = "0"
    b = run_map()
    say("fused and scratch results bit-identical: %s" % bool(torch.equal(a, b)))
    del a, b
    tf, tsc = [], []
    for _ in range(3):
        os.environ.pop("MSM_NYSTROEM_FUSED", None)
        tf.append(timed(run_map, reps=2, warm=1))
        os.environ["MSM_NYSTROEM_FUSED"] = "0"
        tsc.append(timed(run_map, reps=2, warm=1))
    os.environ.pop("MSM_NYSTROEM_FUSED", None)
    tf, tsc = np.concatenate(tf), np.concatenate(tsc)
    for name, t in (("fused map   (N x L float32 out)", tf), ("scratch route (same result)   ", tsc)):
        say("%s: %s  -> call rate %.1f TFLOP/s fp64 over %.3g flop; output %.2f GB (%.2f TB/s of call time)"
            % (name, fmt(t), (flop1 + flop2) / np.median(t) / 1e9, flop1 + flop2, N * L * 4 / 1e9, N * L * 4 / np.median(t) / 1e9))
    # KernelTICA: fit on the first 200,000 rows, transform all rows
    t0 = time.perf_counter()
    m = KernelTICA(n_components=K, lag_time=10, landmarks=lm).fit([X[:200000]])
    torch.cuda.synchronize()
    say("KernelTICA.fit of 200,000 rows (features on the device, tICA accumulation, solve): %.1f ms; eigenvalues %s"
        % ((time.perf_counter() - t0) * 1e3, np.array2string(m.eigenvalues_[:4], precision=4)))

    def folded():
        return m.transform([X])[0]

    def unfused():
        return tICA.transform(m, m._nystroem.transform([X]))[0]

    yf, yu = folded(), unfused()
    say("folded against unfused transform: max |difference| %.3g (scale %.3g)" % (float((yf - yu).abs().max()), float(yu.abs().max())))
    del yf, yu
    tfo, tun = [], []
    for _ in range(3):
        tfo.append(timed(folded, reps=2, warm=1))
        tun.append(timed(unfused, reps=2, warm=1))
    tfo, tun = np.concatenate(tfo), np.concatenate(tun)
    say("KernelTICA.transform, k = %d, folded  (one launch, P = k)      : %s" % (K, fmt(tfo)))
    say("KernelTICA.transform, k = %d, unfused (map, then projection)   : %s" % (K, fmt(tun)))
    # context: the reference's host composition (scikit-learn) on this machine's CPUs, 100,000 rows
    from sklearn.metrics.pairwise import pairwise_kernels
    nh = min(N, 100000)
    M = np.ascontiguousarray(ny.normalization_.T)
    t0 = time.perf_counter()
    emb = pairwise_kernels(Xh[:nh], lm, metric="rbf", filter_params=True, gamma=1.0 / F)
    feats = np.dot(emb, M)
    th = time.perf_counter() - t0
    say("context, not a target: scikit-learn pairwise_kernels + np.dot on the host, %d rows: %.0f ms (%.3g rows/s; %s output)"
        % (nh, th * 1e3, nh / th, feats.dtype))
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
