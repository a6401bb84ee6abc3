#!/usr/bin/env python3
"""What PUCCH receive costs in one device call (include/srsran_amd/phy_pucch_abi.h: srsran_hip_pucch_decode_multi), beside a loop of single calls over the same
jobs: 1, 16, 64 and 256 jobs on cells of 25 and 100 PRB, format 1A and format 2 with 11 bits timed separately.  The jobs are distinct resources of one
subframe (n_pucch = 0, 1, 2, ...) on a grid of noise: what a job costs does not depend on what it finds.  Host to host around the C calls, after a warm-up,
with the profiler off; median / p90 of the timed calls in microseconds.  Nothing is asserted on the figures.  There is no CPU reference time: the reference
cannot run where this does.  One JSON line at the end; the lines are appended to --out.

    python tools/measure/pucch_time.py [--calls 200] [--tag NAME] [--out profiles/pucch_time.txt]
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

import pucch_model as M
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pucch_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    base, basis = M.tables()  # the two tables are the caller's: here the recorded ones
    base, basis = np.ascontiguousarray(base), np.ascontiguousarray(basis)
    capi.check(L.srsran_hip_pucch_set_tables(base.ctypes.data, basis.ctypes.data), "set_tables")
    rng = np.random.default_rng(7)
    result, lines = {"tag": a.tag, "calls": a.calls}, []
    sf = capi.HipPucchSf(7, 0)
    for nof_prb in (25, 100):
        cell = capi.HipPucchCell(nof_prb, 0, 150)
        grid = (0.7 * (rng.standard_normal((14, 12 * nof_prb)) + 1j * rng.standard_normal((14, 12 * nof_prb)))).astype(np.complex64)
        for name, fmt, nbits in (("1a", M.F1A, 0), ("2_11bit", M.F2, 11)):
            for n in (1, 16, 64, 256):
                jobs = (capi.HipPucchJob * n)(*[capi.HipPucchJob(fmt, i, 0, 1, 0, 0, 0x1234, nbits, 1, 3, (C.c_float * 3)(0.3333, 0.3334, 0.3333), 0.5, 0.5, 0.5, 0.0)
                                                for i in range(n)])
                res = (capi.HipPucchRes * n)()

                def multi():
                    assert L.srsran_hip_pucch_decode_multi(C.byref(cell), C.byref(sf), n, jobs, grid.ctypes.data, res) == 0

                def loop():
                    for i in range(n):
                        assert L.srsran_hip_pucch_decode(C.byref(cell), C.byref(sf), C.byref(jobs[i]), grid.ctypes.data, C.byref(res[i])) == 0

                p50, p90 = timed(multi, a.calls)
                q50, q90 = timed(loop, max(10, a.calls // max(1, n // 4)), warm=2)
                key = "%dprb_f%s_%d" % (nof_prb, name, n)
                result[key] = {"multi_p50_us": p50, "multi_p90_us": p90, "loop_p50_us": q50, "loop_p90_us": q90}
                lines.append("%-22s one call p50 %8.1f us  p90 %8.1f us (%6.2f us per job) | %3d single calls p50 %9.1f us  p90 %9.1f us  (x%.1f)" %
                             (key, p50, p90, p50 / n, n, q50, q90, q50 / p50))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("# pucch_time %s (host to host, %d calls each)\n" % (a.tag, a.calls))
        for ln in lines:
            print(ln)
            fh.write(ln + "\n")
        fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
