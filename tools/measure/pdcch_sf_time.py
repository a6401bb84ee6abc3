#!/usr/bin/env python3
"""What the device front end and the device mean rule of the PDCCH search cost (include/srsran_amd/phy_conv_abi.h): srsran_hip_pdcch_search_sf -- received grids
and estimates in, every candidate's result out -- against srsran_hip_pdcch_dci_decode_multi on soft bits that are ALREADY on the host (what the search cost
before, less the host's own srsran_pdcch_extract_llr, which is not timed here), and srsran_hip_pdcch_extract_llr by itself.

    25prb    25 PRB, 2 ports, 2 antennas, CFI 3 (20 CCE, 10 planes of 900 points)
    100prb   100 PRB, 2 ports, 2 antennas, CFI 3 (84 CCE, 10 planes of 3600 points)
44 candidates (22 locations x 2 format sizes) on each; the grids are random QPSK points with unit estimates, so every candidate passes the mean rule and is
decoded in both calls.  Host to host around the C calls, after a warm-up; the calls ALTERNATE call by call in one process, so drift of the clocks hits them alike;
median / p90 in microseconds.  The difference of the medians is the cost of the upload of the planes, the front-end launch and the device mean rule; it is one
machine's figure, and the two calls differ by tens of microseconds at most, so small differences between runs mean nothing.  The lines are appended to --out.

    python tools/measure/pdcch_sf_time.py [--calls 300] [--tag NAME] [--out profiles/pdcch_sf_time.txt]
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

import pdcch_map_model as PM
from srslte_amd import capi

LOCATIONS = ([(n, 0) for n in range(8)] + [(n, 1) for n in range(0, 14, 2)] + [(n, 2) for n in range(0, 20, 4)] + [(0, 3), (8, 3)])  # 8 + 7 + 5 + 2
SIZES = (27, 31)


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdcch_sf_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    capi.check(L.srsran_hip_warmup(1), "warmup")
    rng = np.random.default_rng(5)
    result, lines = {"tag": a.tag, "calls": a.calls}, []
    assert len(LOCATIONS) == 22
    for name, nof_prb in (("25prb", 25), ("100prb", 100)):
        d = PM.describe(nof_prb, 2, 17, 3, sf_idx=3, nof_rx=2)
        sf = capi.HipPdcchSf(*[d[f] for f in PM.FIELDS])
        nregs = L.srsran_hip_regs_pdcch_nregs(C.byref(sf))
        nof_llr, npts = 8 * nregs, 3 * 12 * nof_prb
        rx = [((rng.choice([-1.0, 1.0], npts) + 1j * rng.choice([-1.0, 1.0], npts)) * np.sqrt(0.5)).astype(np.complex64) for _ in range(2)]
        one = np.ones(npts, np.complex64)
        y = (C.c_void_p * 4)(rx[0].ctypes.data, rx[1].ctypes.data, None, None)
        h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in [[one.ctypes.data, one.ctypes.data, None, None]] * 2 + [[None] * 4] * 2])
        cl = [(n, lv, s) for n, lv in LOCATIONS for s in SIZES]
        n = len(cl)
        cand, res, res2 = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*c) for c in cl]), (capi.HipPdcchRes * n)(), (capi.HipPdcchRes * n)()
        llr = np.zeros(nof_llr, np.float32)

        def search():
            assert L.srsran_hip_pdcch_search_sf(C.byref(sf), y, h, C.c_float(0.0), n, cand, res) == 0

        def extract():
            assert L.srsran_hip_pdcch_extract_llr(C.byref(sf), y, h, C.c_float(0.0), llr.ctypes.data) == nof_llr

        def multi():
            assert L.srsran_hip_pdcch_dci_decode_multi(llr.ctypes.data, nof_llr, n, cand, res2) == 0

        fns = [("search_sf", search), ("extract_llr", extract), ("multi", multi)]
        for _ in range(20):
            for _, fn in fns:
                fn()
        assert bytes(res) == bytes(res2), "the two searches differ"
        t = {k: [] for k, _ in fns}
        for _ in range(a.calls):
            for k, fn in fns:
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e6)
        decoded = sum(1 for r in res if r.decoded)
        r = {"nof_cce": nregs // 9, "candidates": n, "decoded": decoded}
        for k, _ in fns:
            r[k] = {"p50_us": round(pct(t[k], 0.5), 1), "p90_us": round(pct(t[k], 0.9), 1)}
        r["front_end_and_mean_us"] = round(r["search_sf"]["p50_us"] - r["multi"]["p50_us"], 1)
        result[name] = r
        lines.append("%-7s %2d CCE, %d candidates (%d decoded)  search_sf p50 %7.1f p90 %7.1f us | multi on host soft bits p50 %7.1f p90 %7.1f us | "
                     "extract_llr p50 %7.1f p90 %7.1f us | search_sf - multi %6.1f us" %
                     (name, nregs // 9, n, decoded, r["search_sf"]["p50_us"], r["search_sf"]["p90_us"], r["multi"]["p50_us"], r["multi"]["p90_us"],
                      r["extract_llr"]["p50_us"], r["extract_llr"]["p90_us"], r["front_end_and_mean_us"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("# pdcch_sf_time %s (host to host, %d calls each, alternating call by call)\n" % (a.tag, a.calls))
        for ln in lines:
            print(ln)
            fh.write(ln + "\n")
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
