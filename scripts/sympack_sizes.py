"""Profiling helper: the fp32 sum/difference kernel (HIP events) on packed handles below bench size, with the packing switch
on and off in one process -- widths 512 .. 1024, one long trajectory or many, 70k .. 2M frames."""
import ctypes as C, os, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from msmbuilder_amd import tICA, _lib

LAG = 100
CASES = [(512, [100000]), (512, [200000]), (512, [500000]), (512, [10000] * 50), (512, [10000] * 100), (512, [10000] * 200),
         (640, [10000] * 50), (768, [10000] * 50), (1024, [200000]), (1024, [10000] * 100),
         (1024, list(np.random.RandomState(11).randint(111, 701, size=200)))]


def kernel_ms(seqs, lag):
    best = None
    for it in range(5):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = tICA(lag_time=lag).fit(seqs)
        ms = C.c_float()
        _lib.check(_lib.lib().msm_tica_last_kernel_ms(m._handle, C.byref(ms)))
        best = ms.value if best is None else min(best, ms.value)
    return best


for F, lens in CASES:
    lens = [int(k) for k in lens]
    X = torch.randn(sum(lens), F, device="cuda")
    seqs = list(torch.split(X, lens))
    lag = LAG if min(lens) > 4 * LAG else 10
    out = {}
    for rnd in range(2):
        for name, value in (("packed", None), ("off", "0")) if rnd == 0 else (("off", "0"), ("packed", None)):
            if value is None:
                os.environ.pop("MSM_TICA_SYM_PACK", None)
            else:
                os.environ["MSM_TICA_SYM_PACK"] = value
            out.setdefault(name, []).append(kernel_ms(seqs, lag))
    os.environ.pop("MSM_TICA_SYM_PACK", None)
    p, o = min(out["packed"]), min(out["off"])
    print("F=%-5d %4d x %-7s frames %8d  off %s ms  packed %s ms  packed/off %.3f" % (
        F, len(lens), lens[0] if len(set(lens)) == 1 else "ragged", sum(lens), " ".join("%.3f" % v for v in out["off"]),
        " ".join("%.3f" % v for v in out["packed"]), p / o), flush=True)
    del X, seqs
