#!/usr/bin/env python3
"""What the PUSCH channel estimator inside the grant call costs (include/srsran_amd/phy_chan_abi.h: srsran_hip_pusch_decode_est{,_multi}).

    two_step  srsran_hip_pusch_decode{,_multi} with the ce grid and the noise estimate ALREADY IN HAND (what srsran_hip_chest_ul_estimate_pusch returned once,
              outside the timed region): the call a caller made before the estimator moved to the device.  It does not include the host estimator such a
              caller pays on top (srsran_chest_ul_estimate_pusch on a CPU core, per UE and TTI).
    est       srsran_hip_pusch_decode_est{,_multi} on the grid alone
on one grant of 6, 25 and 100 PRB (full allocation of such a cell) and on a TTI of 25 grants of 4 PRB on a 100-PRB cell.  The signals are those of
tests/test_gpu_chan.py with a DMRS row put into the grid; every call decodes.  The two routes alternate call by call in one loop after a warm-up of both;
soft buffers are reset outside the timed region.  Median / p90 of the timed calls in microseconds, host to host, and the median of the per-iteration
difference.  One JSON line at the end.

    python tools/measure/chest_ul_time.py [--calls 300] [--tag NAME] [--out FILE]
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

import oracle_api as O
import test_gpu_chan as T
from grant_helpers import _rx_softbuffer
from srslte_amd import capi
from test_gpu_chest_ul import _est, _with_dmrs

#         name      cell PRBs, grants: (first PRB, L_prb, mod, tbs, snr)
SHAPES = [("6prb", 6, [(0, 6, 1, 600, 12.0)]), ("25prb", 25, [(0, 25, 2, 6200, 20.0)]), ("100prb", 100, [(0, 100, 3, 36696, 29.0)]),
          ("tti_25x4prb", 100, [(4 * i, 4, 1, 328, 10.0) for i in range(25)])]
vp = C.c_void_p


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    assert lib.srsran_hip_set_device(0) == 0 and lib.srsran_hip_warmup(1) == 0
    warm = max(30, args.calls // 10)
    rows = []
    for name, nof_prb, ues in SHAPES:
        n = len(ues)
        rng = np.random.default_rng(nof_prb + n)
        grants, ests = (capi.HipPuschRx * n)(), (capi.HipChestUl * n)()
        grids, ces, rs, pays = [], [], [], []
        for i, (a, L_prb, mod, tbs, snr) in enumerate(ues):
            bits = rng.integers(0, 2, tbs).astype(np.uint8)
            grid, h, seed = T._pusch_signal(rng, nof_prb, 7, (a, a), L_prb, 0, mod, tbs, 0, 0x70 + i, 5, 101, snr, bits)
            rs.append(_with_dmrs(rng, grid, h, nof_prb, 7, (a, a), L_prb, snr))
            grants[i] = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, 144 * L_prb, seed, 8, 0, 1), nof_prb, 7, (C.c_uint32 * 2)(a, a), L_prb, 0, 0.0, 0)
            ests[i] = _est(capi, rs[i])
            grids.append(grid)
            ces.append(np.zeros(grid.size, np.complex64))
            pays.append(np.packbits(bits))
        gp, cp = (vp * n)(*[g.ctypes.data for g in grids]), (vp * n)(*[c.ctypes.data for c in ces])
        eo = (capi.HipChestUlRes * n)()
        assert lib.srsran_hip_chest_ul_estimate_pusch_multi(n, grants, ests, gp, cp, eo) == 0, capi.last_error()
        for i in range(n):  # the estimates in hand
            grants[i].noise_estimate = eo[i].noise_estimate
        sbs = [_rx_softbuffer(capi, O.cbsegm(u[3])["C"], np.int16) for u in ues]
        datas = [np.zeros(u[3] // 8 + 16, np.uint8) for u in ues]
        sbp, dp = (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]), (vp * n)(*[d.ctypes.data for d in datas])
        res = (capi.HipGrantRes * n)()
        two = lambda: lib.srsran_hip_pusch_decode_multi(n, grants, gp, cp, sbp, dp, res)  # noqa: E731
        est = lambda: lib.srsran_hip_pusch_decode_est_multi(n, grants, ests, None, gp, sbp, dp, res, None, eo)  # noqa: E731
        tm = {"two_step": [], "est": []}
        for it in range(warm + args.calls):
            for what, fn in (("two_step", two), ("est", est)):
                for sb, rws, _, flags in sbs:  # (outside the timed region: a fresh soft buffer)
                    flags[:] = False
                    sb.tb_crc = False
                    for r in rws:
                        r[:] = 0
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert rc == 0, (name, what, rc, capi.last_error())
                for i in range(n):
                    assert res[i].crc_ok == 1 and np.array_equal(datas[i][:ues[i][3] // 8], pays[i]), (name, what, i)
                if it >= warm:
                    tm[what].append(dt)
        row = dict(shape=name, grants=n, calls=args.calls, two_step_p50_us=round(pct(tm["two_step"], 0.5), 1), two_step_p90_us=round(pct(tm["two_step"], 0.9), 1),
                   est_p50_us=round(pct(tm["est"], 0.5), 1), est_p90_us=round(pct(tm["est"], 0.9), 1),
                   est_minus_two_step_p50_us=round(pct([b - a for a, b in zip(tm["two_step"], tm["est"])], 0.5), 1))
        rows.append(row)
        print("%-6s %-12s %2d grant(s)   _decode with estimates in hand p50 %6.1f p90 %6.1f us | _decode_est p50 %6.1f p90 %6.1f us | est - two_step, call by call, p50 %+5.1f us" %
              (args.tag, name, n, row["two_step_p50_us"], row["two_step_p90_us"], row["est_p50_us"], row["est_p90_us"], row["est_minus_two_step_p50_us"]), flush=True)
    line = json.dumps({"tool": "chest_ul_time", "tag": args.tag, "unit": "us, host to host", "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
