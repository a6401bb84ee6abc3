#!/usr/bin/env python3
"""What a PRACH detection costs in one device call (include/srsran_amd/phy_prach_abi.h: srsran_hip_prach_detect_offset, srsran_hip_prach_detect_multi), beside
the same detection's transforms made the way a caller can make them without the call: one srsran_dft_run_c of N_ifft_prach points (forward, mirror, norm)
plus one backward 839-point srsran_dft_run_c per searched root, through the handle API -- each its own upload, launch, download and host wait.  That path
leaves the spectrum products, |.|^2, the means and the window searches to the host, which are NOT timed here: it is a lower bound of the per-transform way.

    6prb_1root     6 PRB (N = 1536),  zero_corr_zone 1: one searched root, 64 windows
    6prb_64roots   6 PRB,             zero_corr_zone 0: 64 searched roots
    100prb_1root   100 PRB at the standard symbol size (N = 24,576), zero_corr_zone 1
    100prb_64roots 100 PRB, zero_corr_zone 0
    multi8         8 occasions of the 100-PRB, 64-root cell in one srsran_hip_prach_detect_multi
Host to host around the C calls, after a warm-up; median / p90 of the timed calls in microseconds.  There is no CPU reference time: the reference's transform
backend is not available where this runs.  One JSON line at the end; the lines are appended to --out.

    python tools/measure/prach_time.py [--calls 200] [--tag NAME] [--out profiles/prach_time.txt]
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

import prach_model as M
from srslte_amd import capi


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def timed(fn, calls, warm=10):
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prach_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    order = np.ascontiguousarray(M.root_order(), np.uint32)  # Table 5.7.2-4 is the caller's: here the recorded one
    capi.check(L.srsran_hip_prach_set_root_order(order.ctypes.data), "set_root_order")
    rng = np.random.default_rng(7)
    result, lines = {"tag": a.tag, "calls": a.calls}, []
    for name, nof_prb, zcz in (("6prb_1root", 6, 1), ("6prb_64roots", 6, 0), ("100prb_1root", 100, 1), ("100prb_64roots", 100, 0)):
        L.srsran_use_standard_symbol_size(nof_prb == 100)
        cfg = capi.HipPrachCfg(nof_prb, 0, 22, zcz, 0, 0, 0, 0.0)
        h, info = C.c_void_p(), capi.HipPrachInfo()
        try:
            capi.check(L.srsran_hip_prach_create(C.byref(h), C.byref(cfg)), "create")
        finally:
            L.srsran_use_standard_symbol_size(False)
        capi.check(L.srsran_hip_prach_info(h, C.byref(info)), "info")
        N, R = info.N_ifft_prach, info.num_ra_preambles
        sig = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
        ind, toff, p2a, n = np.zeros(128, np.uint32), np.zeros(128, np.float32), np.zeros(128, np.float32), C.c_uint32()

        def one():
            assert L.srsran_hip_prach_detect_offset(h, 0, sig.ctypes.data, N, ind.ctypes.data, toff.ctypes.data, p2a.ctypes.data, 128, C.byref(n)) == 0

        p50, p90 = timed(one, a.calls)
        # the per-transform way: the transforms alone
        big, small = capi.DftPlan(), capi.DftPlan()
        assert L.srsran_dft_plan_c(C.byref(big), N, capi.DFT_FORWARD) == 0 and L.srsran_dft_plan_c(C.byref(small), M.N_ZC, capi.DFT_BACKWARD) == 0
        L.srsran_dft_plan_set_mirror(C.byref(big), True)
        L.srsran_dft_plan_set_norm(C.byref(big), True)
        spectrum, cs, out = np.zeros(N, np.complex64), np.ones(M.N_ZC, np.complex64), np.zeros(M.N_ZC, np.complex64)

        def per_transform():
            L.srsran_dft_run_c(C.byref(big), sig.ctypes.data, spectrum.ctypes.data)
            for _ in range(R):
                L.srsran_dft_run_c(C.byref(small), cs.ctypes.data, out.ctypes.data)

        q50, q90 = timed(per_transform, max(20, a.calls // 4), warm=3)
        L.srsran_dft_plan_free(C.byref(big))
        L.srsran_dft_plan_free(C.byref(small))
        result[name] = {"N": N, "roots": R, "call_p50_us": p50, "call_p90_us": p90, "per_transform_p50_us": q50, "per_transform_p90_us": q90}
        lines.append("%-15s N %5d, %2d roots: one call p50 %8.1f us  p90 %8.1f us | %2d transforms through the handle API p50 %9.1f us  p90 %9.1f us  (x%.1f)" %
                     (name, N, R, p50, p90, R + 1, q50, q90, q50 / p50))
        if name == "100prb_64roots":
            occ = (capi.HipPrachOcc * 8)(*[capi.HipPrachOcc(o, N, sig.ctypes.data) for o in range(8)])
            res = (capi.HipPrachRes * 8)()

            def multi():
                assert L.srsran_hip_prach_detect_multi(h, 8, occ, res) == 0

            p50, p90 = timed(multi, a.calls)
            result["multi8"] = {"N": N, "roots": R, "occasions": 8, "call_p50_us": p50, "call_p90_us": p90}
            lines.append("%-15s N %5d, %2d roots, 8 occasions: one call p50 %8.1f us  p90 %8.1f us  (%.1f us per occasion)" % ("multi8", N, R, p50, p90, p50 / 8))
        L.srsran_hip_prach_destroy(h)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("# prach_time %s (host to host, %d calls each)\n" % (a.tag, a.calls))
        for ln in lines:
            print(ln)
            fh.write(ln + "\n")
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
