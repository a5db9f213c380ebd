#!/usr/bin/env python
"""scripts/bace_probe.py -- what BACE lumping costs on the card: the initial Bayes-factor matrix, the merge loop, the whole
``BACE.from_msm`` on block-structured dense counts, next to the Jensen-Shannon condensed pdist of as many rows (the same
two logarithms per element for the same n (n - 1) / 2 pairs) -- and, with ``--reference``, the reference's own
``BACE.from_msm`` on the CPU (needs the reference tree; no device).

    python scripts/bace_probe.py [--sizes 1024 4096] [--blocks 8] [--reference 400 1024]

The times of the initial matrix and of the loop are device events inside ``msm_bace_fit``; the pdist is timed by device
events on the same stream around the call (its host clock is printed beside it); ``from_msm`` is a host clock around a call
that ends in a device synchronise.  Every device number is the second of two runs.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block_counts(n, k, seed):
    rs = np.random.RandomState(seed)
    lab = np.arange(n) % k
    return np.floor(rs.gamma(1.0, 1.0, (n, n)) * np.where(lab[:, None] == lab[None, :], 1.0, 0.02) * 200.0)


class Fitted(object):
    """What ``from_msm`` reads of a fitted MSM."""

    def __init__(self, counts, model):
        n = len(counts)
        self._model = model
        self.transmat_, self.populations_, self.countsmat_ = None, np.full(n, 1.0 / n), counts
        self.mapping_, self.n_states_ = dict(zip(range(n), range(n))), n

    def get_params(self):
        return self._model.get_params()


def device(sizes, blocks):
    import torch
    from msmbuilder_amd import BACE, MarkovStateModel, _lib
    from msmbuilder_amd.lumping import bace as B
    from msmbuilder_amd.utils import divergence
    _lib.ensure_device(0)
    print("device:", torch.cuda.get_device_name(0))
    for n in sizes:
        C = block_counts(n, blocks, n)
        w = C.sum(1) + 1
        keep = np.ones(n, dtype=np.int32)
        dC = torch.as_tensor(C, device='cuda')
        rows = torch.as_tensor(C / C.sum(1, keepdims=True), device='cuda')
        for _ in range(2):
            merges, values, ms = B.bace_merges(dC, w, keep, blocks, timings=True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            divergence.divergence_pdist(rows, 'js_divergence')
            e1.record()
            torch.cuda.synchronize()
            t_js, ev_js = time.perf_counter() - t0, e0.elapsed_time(e1)
            t0 = time.perf_counter()
            lumped = BACE.from_msm(Fitted(C, MarkovStateModel(verbose=False)), blocks, filter=0)
            t_all = time.perf_counter() - t0
        n_merges = len(merges) - 1
        sizes_ = sorted(np.bincount(lumped.microstate_mapping_).tolist())
        print("n = %6d  blocks = %d  merges = %d" % (n, blocks, n_merges))
        print("    initial matrix            %10.3f ms   (%.3g pair-columns/s)" % (ms[0], n * (n - 1) / 2.0 * n / (ms[0] * 1e-3)))
        print("    js_divergence pdist       %10.3f ms   by device events, as the initial matrix: initial matrix / pdist = %.2f" % (ev_js, ms[0] / ev_js))
        print("      (host clock around the call, output allocation included: %.3f ms)" % (t_js * 1e3))
        print("    merge loop                %10.3f ms   %.1f us per merge" % (ms[1], ms[1] * 1e3 / max(n_merges, 1)))
        print("    msm_bace_fit, both        %10.3f ms" % ms[2])
        print("    BACE.from_msm (filter=0)  %10.3f ms   macrostate sizes %s" % (t_all * 1e3, sizes_ if len(sizes_) <= 16 else len(sizes_)))
        sys.stdout.flush()


def reference(sizes, blocks):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import warnings
    warnings.simplefilter("ignore")
    import make_golden_bace as G
    MSM, BACE = G.load()
    for n in sizes:
        C = block_counts(n, blocks, n)
        with np.errstate(all='ignore'):
            t0 = time.perf_counter()
            lumped = BACE.from_msm(Fitted(C, MSM(verbose=False)), blocks, filter=0)
            t = time.perf_counter() - t0
        print("reference on the CPU  n = %6d  blocks = %d  BACE.from_msm (filter=0) %10.3f s   macrostate sizes %s"
              % (n, blocks, t, sorted(np.bincount(lumped.map_dict[blocks]).tolist())))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reference", type=int, nargs="*", default=None)
    a = ap.parse_args()
    if a.reference is not None:
        reference(a.reference or [400, 1024], a.blocks)
    else:
        device(a.sizes, a.blocks)


if __name__ == "__main__":
    main()
