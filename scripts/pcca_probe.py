#!/usr/bin/env python
"""scripts/pcca_probe.py -- times of the PCCA+ objectives on the device (csrc/pcca.hip) at n = 1,024, 4,096 and 16,384 states
and m = 6 macrostates, written to profiles/pcca_probe.txt.

Per size: the set-up (``msm_pcca_create`` from device arrays: the copies, T V and the moments); one evaluation of each kind
with a mapping that differs from the previous evaluation's and with a repeated one, as the mean over a loop between two
device events after a warm-up (an evaluation ends in a stream synchronise, so this is what a search pays per call); the same
evaluation by the numpy host functions of ``msmbuilder_amd.lumping.pcca_plus`` on this machine, and the ratio.

The yardstick of a kind-2 evaluation with a new mapping is a plain read-only reduction over the same n^2 doubles
(``torch.sum``), timed in the same run, plus the evaluation's own small launches, timed at n = 64 where T is nothing.

Usage:  python scripts/pcca_probe.py [--sizes 1024,4096,16384] [--out profiles/pcca_probe.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msmbuilder_amd import _lib  # noqa: E402
from msmbuilder_amd.lumping import pcca_plus as PP  # noqa: E402

KINDS = ('crispness', 'metastability', 'crisp_metastability')


def system(n, m, seed=0):
    """A row-stochastic T with m blocks, pi, and a V of noisy block indicators (column 0 all ones): enough states sit near a
    tie that a small change of alpha moves the mapping."""
    rs = np.random.RandomState(seed)
    home = np.arange(n) % m
    T = rs.random_sample((n, n))
    T *= np.where(home[:, None] == home[None, :], 1.0, 0.02)
    T /= T.sum(axis=1)[:, None]
    pi = rs.uniform(0.5, 1.5, n)
    pi /= pi.sum()
    V = np.zeros((n, m))
    V[:, 0] = 1.0
    V[np.arange(n), home] = 1.0
    V[:, 1:] += 0.35 * rs.standard_normal((n, m - 1))
    return T, pi, np.ascontiguousarray(V)


class Events(object):
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().msm_event_create(C.byref(self.a)))
        _lib.check(_lib.lib().msm_event_create(C.byref(self.b)))

    def time(self, fn, reps):
        ms = C.c_float(0.0)
        _lib.check(_lib.lib().msm_event_record(self.a))
        for _ in range(reps):
            fn()
        _lib.check(_lib.lib().msm_event_record(self.b))
        _lib.check(_lib.lib().msm_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value * 1e3 / reps     # microseconds per call


def two_alphas(handle, V, m):
    """alpha0 (the initial A) and a nearby alpha whose mapping differs and is feasible."""
    A = PP.fill_A(np.linalg.inv(V[PP.index_search(V), :]), V)
    a0 = A[1:, 1:].ravel().copy()
    rs = np.random.RandomState(1)
    handle.objective(2, a0)
    for scale in (0.01, 0.02, 0.05, 0.1, 0.2):
        for _ in range(20):
            a1 = a0 * (1 + scale * rs.standard_normal(a0.size))
            value, info = handle.objective(2, a1)
            back = handle.objective(2, a0)[1]
            if info.tolist() == [1, m, 0, 1] and back.tolist() == [1, m, 0, 1]:
                return a0, a1
    raise RuntimeError("no second feasible mapping found")


def probe(n, m, events, lines, host_reps):
    import torch
    T, pi, V = system(n, m)
    dT, dpi, dV = [torch.as_tensor(x, device='cuda') for x in (T, pi, V)]
    torch.cuda.synchronize()
    PP.PccaHandle(dT, dpi, dV).close()                      # warm-up
    made = []
    setup = events.time(lambda: made.append(PP.PccaHandle(dT, dpi, dV)), 3)
    for h in made[1:]:
        h.close()
    handle = made[0]
    a0, a1 = two_alphas(handle, V, m)
    flip = [a0, a1]
    reps = 200 if n <= 4096 else 40
    row = {}
    for kind in range(3):
        for _ in range(10):
            handle.objective(kind, a0)
        count = [0]

        def new_mapping():
            count[0] += 1
            handle.objective(kind, flip[count[0] % 2])

        row[kind, 'repeat'] = events.time(lambda: handle.objective(kind, a0), reps)
        row[kind, 'new'] = events.time(new_mapping, reps)
    torch.sum(dT)
    torch.cuda.synchronize()
    reduce_us = events.time(lambda: (torch.sum(dT), torch.cuda.synchronize()), 20)
    flat_map, square_map = PP.get_maps(np.zeros((m, m)))
    host = {}
    for kind, name in enumerate(KINDS):
        fn = getattr(PP, name)
        fn(a0, T, V, square_map, pi)
        t0 = time.perf_counter()
        for _ in range(host_reps):
            fn(a0, T, V, square_map, pi)
        host[kind] = (time.perf_counter() - t0) / host_reps * 1e6
    handle.close()
    lines.append("n = %d, m = %d: set-up %.0f us (T V and the moments, T already on the device); read-only reduction of T %.1f us"
                 % (n, m, setup, reduce_us))
    for kind, name in enumerate(KINDS):
        lines.append("  %-20s new mapping %9.1f us   repeated mapping %9.1f us   numpy on the host %12.1f us   host / device (new) %8.1f x"
                     % (name, row[kind, 'new'], row[kind, 'repeat'], host[kind], host[kind] / row[kind, 'new']))
    return row, reduce_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcca_probe.txt"))
    args = ap.parse_args()
    import torch
    _lib.ensure_device()
    events = Events()
    m = 6
    lines = ["PCCA+ objectives on the device: %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")),
             "times per call between two device events after a warm-up; every evaluation ends in a stream synchronise", ""]
    small, _ = probe(64, m, events, lines, 20)
    launches = small[2, 'new']
    lines.append("  -> the kind-2 evaluation's own launches, upload and read-back (n = 64): %.1f us" % launches)
    lines.append("")
    for n in [int(x) for x in args.sizes.split(",")]:
        row, reduce_us = probe(n, m, events, lines, 20 if n <= 1024 else (5 if n <= 4096 else 2))
        lines.append("  -> kind 2, new mapping: %.1f us against reduction %.1f us + launches %.1f us = %.1f us: ratio %.2f"
                     % (row[2, 'new'], reduce_us, launches, reduce_us + launches, row[2, 'new'] / (reduce_us + launches)))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
