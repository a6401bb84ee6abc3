#!/usr/bin/env python3
"""What the control side of a subframe costs from the received grids alone (include/srsran_amd/phy_conv_abi.h): srsran_hip_pdcch_search_est -- the estimator,
PCFICH, PHICH, the PDCCH front end and every candidate decode in one device call -- against the chain a caller needed before it, srsran_hip_chest_dl_estimate then
srsran_hip_pdcch_search_sf with the estimates it brought down (which still LACKS the host's PCFICH between the two: that chain is handed the CFI).

    25prb    25 PRB, 2 ports, 2 antennas (CFI 3: 20 CCE)
    100prb   100 PRB, 2 ports, 2 antennas (CFI 3: 84 CCE)
44 candidates (22 locations x 2 format sizes) in the list of CFI 3, those of them that fit in the lists of CFI 1 and 2, four PHICH resources.  The grids are
random QPSK points; the PCFICH's 16 REs are redrawn until the call decodes CFI 3, so that both legs search the same region with the same 44 candidates.  Host
to host around the C calls, after a warm-up; the legs ALTERNATE call by call in one process, so drift of the clocks hits them alike; median / p90 in microseconds.
One machine's figures; nothing is asserted on them.  The lines are appended to --out.

    python tools/measure/pdcch_est_time.py [--calls 300] [--tag NAME] [--out profiles/pdcch_est_time.txt]
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


def qpsk(rng, n):
    return ((rng.choice([-1.0, 1.0], n) + 1j * rng.choice([-1.0, 1.0], n)) * np.sqrt(0.5)).astype(np.complex64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdcch_est_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    capi.check(L.srsran_hip_warmup(1), "warmup")
    rng = np.random.default_rng(5)
    result, lines = {"tag": a.tag, "calls": a.calls}, []
    for name, nof_prb in (("25prb", 25), ("100prb", 100)):
        d = PM.describe(nof_prb, 2, 17, 3, sf_idx=3, nof_rx=2)
        sf = capi.HipPdcchSf(*[d[f] for f in PM.FIELDS])
        nof_cce = []
        for cfi in (1, 2, 3):
            one = capi.HipPdcchSf(*[dict(d, cfi=cfi)[f] for f in PM.FIELDS])
            nof_cce.append(L.srsran_hip_regs_pdcch_nregs(C.byref(one)) // 9)
        npts = 14 * 12 * nof_prb
        rx = [qpsk(rng, npts) for _ in range(2)]
        pilots = [qpsk(rng, 8 * nof_prb), qpsk(rng, 4 * nof_prb)]
        est = capi.HipChestDl()
        est.nof_prb, est.nof_ports, est.id, est.cp_nsymb, est.nof_rx, est.sf_idx = nof_prb, 2, 17, 7, 2, 3
        est.estimator_alg, est.noise_alg, est.filter_type = 1, 0, 2  # INTERPOLATE, REFS, no filter
        est.pilots[0], est.pilots[1] = pilots[0].ctypes.data, pilots[1].ctypes.data
        state, out, out2 = capi.HipChestDlState(), capi.HipChestDlRes(), capi.HipChestDlRes()
        y = (C.c_void_p * 4)(rx[0].ctypes.data, rx[1].ctypes.data, None, None)
        ce = [[np.zeros(npts, np.complex64) for _ in range(2)] for _ in range(2)]
        h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in [[g.ctypes.data for g in r] + [None] * 2 for r in ce] + [[None] * 4] * 2])
        all44 = [(n, lv, s) for n, lv in LOCATIONS for s in SIZES]
        lists = [[k for k in all44 if k[0] + (1 << k[1]) <= nof_cce[c]] for c in range(3)]
        assert len(lists[2]) == 44
        flat = [k for x in lists for k in x]
        cand = (capi.HipPdcchCand * len(flat))(*[capi.HipPdcchCand(*k) for k in flat])
        cand3 = (capi.HipPdcchCand * 44)(*[capi.HipPdcchCand(*k) for k in lists[2]])
        opt = capi.HipPdcchEst((C.c_uint32 * 3)(*[len(x) for x in lists]), 0, 4)
        res, res2, ph = (capi.HipPdcchRes * 44)(), (capi.HipPdcchRes * 44)(), (capi.HipPhichRes * 4)()
        r = (capi.HipPhichResource * 4)(*[capi.HipPhichResource(g, s) for g, s in ((0, 0), (0, 5), (1, 2), (1, 7))])
        cfi, corr = C.c_uint32(0), C.c_float(0)

        def search_est():
            assert L.srsran_hip_pdcch_search_est(C.byref(sf), C.byref(est), C.byref(state), y, C.byref(opt), cand, res, r, ph, C.byref(cfi), C.byref(corr), C.byref(out)) == 0

        def chain():
            assert L.srsran_hip_chest_dl_estimate(C.byref(est), C.byref(state), y, h, C.byref(out2)) == 0
            assert L.srsran_hip_pdcch_search_sf(C.byref(sf), y, h, C.c_float(out2.noise_estimate), 44, cand3, res2) == 0

        idx = np.zeros(16, np.uint32)
        assert L.srsran_hip_regs_pcfich_table(C.byref(sf), idx.ctypes.data) == 16
        for _ in range(200):  # redraw the PCFICH's REs until they say CFI 3
            search_est()
            if cfi.value == 3:
                break
            for g in rx:
                g[idx] = qpsk(rng, 16)
        assert cfi.value == 3, "no draw of the PCFICH REs decoded to CFI 3"
        fns = [("search_est", search_est), ("estimate_then_search_sf", chain)]
        for _ in range(20):
            for _, fn in fns:
                fn()
        assert bytes(res) == bytes(res2) and bytes(out) == bytes(out2), "the two legs differ"
        t = {k: [] for k, _ in fns}
        for _ in range(a.calls):
            for k, fn in fns:
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e6)
        rr = {"nof_cce": nof_cce, "candidates": [len(x) for x in lists], "decoded": sum(1 for x in res if x.decoded)}
        for k, _ in fns:
            rr[k] = {"p50_us": round(pct(t[k], 0.5), 1), "p90_us": round(pct(t[k], 0.9), 1)}
        rr["one_call_minus_two_us"] = round(rr["search_est"]["p50_us"] - rr["estimate_then_search_sf"]["p50_us"], 1)
        result[name] = rr
        lines.append("%-7s %2d CCE, 44 candidates (%d decoded), 4 PHICH resources  search_est p50 %7.1f p90 %7.1f us | chest_dl_estimate + search_sf (no PCFICH) "
                     "p50 %7.1f p90 %7.1f us | one call - two calls %7.1f us" %
                     (name, nof_cce[2], rr["decoded"], rr["search_est"]["p50_us"], rr["search_est"]["p90_us"], rr["estimate_then_search_sf"]["p50_us"],
                      rr["estimate_then_search_sf"]["p90_us"], rr["one_call_minus_two_us"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("# pdcch_est_time %s (host to host, %d calls each, alternating call by call)\n" % (a.tag, a.calls))
        for ln in lines:
            print(ln)
            fh.write(ln + "\n")
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
