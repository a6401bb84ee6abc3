#!/usr/bin/env python3
"""What the PDCCH blind search's decodes cost in one device call (include/srsran_amd/phy_conv_abi.h: srsran_hip_pdcch_dci_decode_multi), and one frame through
the handle API (srsran_viterbi_decode_f).

    multi44   22 locations x 2 format sizes on a 25-PRB, CFI-3 region (21 CCE): the search space of tests/test_gpu_conv.py
    multi88   22 locations x 4 format sizes (27, 31, 39, 43 bits) on the same region
    handle    srsran_viterbi_decode_f, one 40-bit tail-biting frame (the PBCH's)
Host to host around the C call, after a warm-up; median / p90 of the timed calls in microseconds.  There is nothing to compare with on this host: the parent
commit has no device path for these decodes and the reference's own decode time is not available where this runs.  One JSON line at the end; the lines are
appended to --out.

    python tools/measure/pdcch_time.py [--calls 300] [--tag NAME] [--out profiles/pdcch_time.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import conv_model as M
from srslte_amd import capi
from test_gpu_conv import search_space


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def timed(fn, calls, warm=20):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return round(pct(t, 0.5), 1), round(pct(t, 0.9), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdcch_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    capi.check(L.srsran_hip_warmup(1), "warmup")
    llr, cands44, _ = search_space()
    locs = [(n, lv) for n, lv, _ in cands44[::2]]  # the 22 locations, in the order of the search space
    result = {"tag": a.tag, "calls": a.calls}
    lines = []
    for name, sizes in (("multi44", (27, 31)), ("multi88", (27, 31, 39, 43))):
        cl = [(n, lv, s) for n, lv in locs for s in sizes]
        n = len(cl)
        cand = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*c) for c in cl])
        res = (capi.HipPdcchRes * n)()

        def call():
            assert L.srsran_hip_pdcch_dci_decode_multi(llr.ctypes.data, llr.size, n, cand, res) == 0

        p50, p90 = timed(call, a.calls)
        decoded = sum(1 for r in res if r.decoded)
        result[name] = {"candidates": n, "decoded": decoded, "p50_us": p50, "p90_us": p90}
        lines.append("%-8s %3d candidates (%3d decoded)  p50 %8.1f us  p90 %8.1f us  (%.2f us per decoded candidate)" % (name, n, decoded, p50, p90, p50 / decoded))
    q = capi.Viterbi()
    assert L.srsran_viterbi_init(C.byref(q), capi.SRSRAN_VITERBI_37, (C.c_int * 3)(*M.POLY), 40, True) == 0
    rng = np.random.default_rng(3)
    sym = (2.0 * (2.0 * M.encode(rng.integers(0, 2, 40), True) - 1.0) + rng.standard_normal(120)).astype(np.float32)
    data = np.zeros(40, np.uint8)

    def one():
        assert L.srsran_viterbi_decode_f(C.byref(q), sym.ctypes.data, data.ctypes.data, 40) == 40

    p50, p90 = timed(one, a.calls)
    result["handle"] = {"frame_bits": 40, "p50_us": p50, "p90_us": p90}
    lines.append("%-8s one 40-bit frame, srsran_viterbi_decode_f  p50 %8.1f us  p90 %8.1f us" % ("handle", p50, p90))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("# pdcch_time %s (host to host, %d calls each)\n" % (a.tag, a.calls))
        for ln in lines:
            print(ln)
            fh.write(ln + "\n")
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
