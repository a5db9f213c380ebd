#!/usr/bin/env python
"""scripts/rmsd_probe.py -- what the rmsd metric costs on one MI355X; writes profiles/rmsd_probe.txt.

    python scripts/rmsd_probe.py            # needs the GPU
    python scripts/rmsd_probe.py --out DIR  # write the file into DIR instead of profiles/

float32 conformations resident in HBM, three shapes (frames x atoms): 280,000 x 264 (28 trajectories of 10,000 frames),
1,000,000 x 22 and 200,000 x 1,000.  Per shape, the median of a few calls (a host clock around a call that ends in a device
synchronise, after a warm-up call) and its ratio to a floor computed from the shape:

    prepare                one read of xyz + one write of the image, at 8.0 TB/s
    dist, KCenters.fit     one read of the image per pass, at 8.0 TB/s (K = 100 passes; the frames prepared beforehand)
    assign_nearest, pdist  18 A flops per pair on the fp32 MFMA at 157.3 TFLOP/s (K = 1,000 centres; 5,000 frames)

The epilogue (the quartic and Newton, once per pair, independent of A) is not timed by itself: the tile kernel is run
at A and at A / 2 atoms on the same frames, and t(A) = main(A) + epilogue with main linear in A gives epilogue ~ 2 t(A/2) -
t(A) (launch overhead included); its share is that over t(A).
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(280000, 264), (1000000, 22), (200000, 1000)]
HBM_PEAK = 8.0e12      # bytes / s, specification
MFMA_PEAK = 157.3e12   # fp32 flop / s, specification
K_CENTERS, K_ASSIGN, N_PDIST = 100, 1000, 5000
REPEATS = 5


def timed(fn, repeats=REPEATS):
    import torch
    fn()   # warm-up: code objects, the library's scratch, torch's allocator
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del out
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    import torch
    from msmbuilder_amd import _lib, libdistance as L
    from msmbuilder_amd.cluster.kcenters import _KCenters
    _lib.ensure_device(0)
    lines = ["The rmsd metric on one MI355X, float32 conformations resident in HBM; written by scripts/rmsd_probe.py on %s."
             % datetime.date.today().isoformat(),
             "ms: median of %d calls (3 for KCenters.fit, assign_nearest and pdist) (min .. max), host clock around a synchronised call, after one warm-up call." % REPEATS,
             "floors: HBM at %.1f TB/s (prepare: xyz read + image written; dist / k-centers: the image read once per pass);"
             % (HBM_PEAK / 1e12),
             "        fp32 MFMA at %.1f TFLOP/s, 18 A flops per pair (assign_nearest at K = %d, pdist of %d frames)."
             % (MFMA_PEAK / 1e12, K_ASSIGN, N_PDIST),
             "epilogue: 2 t(A/2) - t(A) of the same call on the first A/2 atoms (see the script's docstring), and its share of t(A).",
             "%-18s %-34s %10s %22s %10s %8s" % ("frames x atoms", "call", "ms", "(min .. max)", "floor ms", "x floor")]

    def row(shape, name, t, floor_ms):
        lines.append("%-18s %-34s %10.3f %22s %10.4f %8.1f" % (shape, name, t[0], "(%.3f .. %.3f)" % (t[1], t[2]), floor_ms,
                                                              t[0] / floor_ms))
        print(lines[-1], flush=True)

    for n, A in SHAPES:
        shape = "%d x %d" % (n, A)
        g = torch.Generator(device="cuda").manual_seed(0)
        xyz = torch.randn((n, A, 3), generator=g, device="cuda", dtype=torch.float32)
        image_bytes = 3 * A * ((n + 63) // 64 * 64) * 4 + 8 * n
        row(shape, "prepare (RmsdFrames)", timed(lambda: L.RmsdFrames(xyz)), (xyz.numel() * 4 + image_bytes) / HBM_PEAK * 1e3)
        frames = L.RmsdFrames(xyz)
        y = L.RmsdFrames(xyz[:1].contiguous())
        row(shape, "dist (one pass)", timed(lambda: L.dist(frames, y, "rmsd")), image_bytes / HBM_PEAK * 1e3)
        kc = _KCenters(n_clusters=K_CENTERS, metric="rmsd", random_state=0)
        row(shape, "KCenters.fit K=%d (prepared)" % K_CENTERS, timed(lambda: kc.fit(frames), 3),
            K_CENTERS * image_bytes / HBM_PEAK * 1e3)
        row(shape, "KCenters.fit K=%d (with prepare)" % K_CENTERS, timed(lambda: kc.fit(xyz), 3),
            (K_CENTERS * image_bytes + xyz.numel() * 4 + image_bytes) / HBM_PEAK * 1e3)
        centres = L.RmsdFrames(xyz[:K_ASSIGN].contiguous())
        t_full = timed(lambda: L.rmsd_assign(frames, centres), 3)
        row(shape, "assign_nearest K=%d" % K_ASSIGN, t_full, 18.0 * A * n * K_ASSIGN / MFMA_PEAK * 1e3)
        sub = L.RmsdFrames(xyz[:N_PDIST].contiguous())
        p_full = timed(lambda: L.pdist(sub, "rmsd"), 3)
        row(shape, "pdist of %d frames" % N_PDIST, p_full, 18.0 * A * N_PDIST * (N_PDIST - 1) / 2 / MFMA_PEAK * 1e3)
        del frames, centres, sub, y
        # the same two calls on the first half of the atoms
        half = xyz[:, :A // 2, :].contiguous()
        del xyz
        frames = L.RmsdFrames(half)
        centres = L.RmsdFrames(half[:K_ASSIGN].contiguous())
        sub = L.RmsdFrames(half[:N_PDIST].contiguous())
        t_half = timed(lambda: L.rmsd_assign(frames, centres), 3)
        p_half = timed(lambda: L.pdist(sub, "rmsd"), 3)
        for name, full, hf in (("assign_nearest", t_full, t_half), ("pdist", p_full, p_half)):
            epi = 2.0 * hf[0] - full[0]
            lines.append("%-18s %-34s t(A/2) = %.3f ms, epilogue ~ %.3f ms = %.0f %% of t(A)"
                         % (shape, name + " epilogue", hf[0], epi, 100.0 * epi / full[0]))
            print(lines[-1], flush=True)
        del frames, centres, sub, half
        torch.cuda.empty_cache()
    lines.append("Not measured: host-resident input (the upload dominates), the kernels under rocprofv3, more than one GPU.")
    with open(os.path.join(args.out, "rmsd_probe.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
