#!/usr/bin/env python3
"""Host-to-host latency of one PUSCH transmit grant (include/srsran_amd/phy_chan_abi.h), 16-QAM, at 6, 25 and 100 PRB:

    one_call      srsran_hip_pusch_encode without control information: one host wait
    one_call_uci  the same with (Q'ack, Q'ri, Q'cqi) = (24, 5, 60); nothing to compare it with: before this call such a grant did not reach the device
    three_waits   the only route there was for the grant without control information: srsran_hip_ulsch_encode -> srsran_hip_modulate_bytes with scrambling ->
                  srsran_dft_precoding through the handle API -> the host copy of the 12 rows into the grid.  Three host waits.

The routes alternate call by call in one loop after a warm-up of all of them (so drift and clock changes hit them alike); the first round checks that the two
routes without control information fill the same grid.  The three_waits route's row copies are numpy slice assignments made from this script, the one-call
route's are the library's memcpy: a few microseconds of interpreter time sit in the three_waits column on top of its three ctypes calls.  Median / p90 of the
timed calls in microseconds; one JSON line at the end.

    python tools/measure/pusch_tx_time.py [--calls 300] [--out FILE]
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
from grant_helpers import _tx_softbuffer
from srslte_amd import capi

GRANTS = [("6prb", 6, 1544), ("25prb", 25, 6200), ("100prb", 100, 36696)]  # name, L_prb = cell width, tbs
MOD, QM, COLS, UCI = 2, 4, 12, (24, 5, 60)


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    assert lib.srsran_hip_set_device(0) == 0 and lib.srsran_hip_warmup(1) == 0
    warm = max(30, args.calls // 10)
    rows_out = []
    for name, L_prb, tbs in GRANTS:
        rng = np.random.default_rng(L_prb)
        nsc, H = 12 * L_prb, COLS * 12 * L_prb
        seed = O.pusch_seed(0x46, 14, 211)
        pay = rng.integers(0, 256, tbs // 8).astype(np.uint8)
        sb = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
        tb = capi.HipGrantTb(MOD, tbs, 0, H, seed, 0, 0, 1)
        g = capi.HipPuschTx(tb, L_prb, 7, (C.c_uint32 * 2)(0, 0), L_prb, 0)
        uci = capi.HipPuschUci(*UCI)
        ack, ri, cqi = (np.tile(np.array([1, 2, 3, 3], np.uint8), UCI[0]), np.tile(np.array([0, 2, 3, 3], np.uint8), UCI[1]), rng.integers(0, 2, UCI[2] * QM).astype(np.uint8))
        uin = capi.HipPuschUciIn(ack.ctypes.data, ri.ctypes.data, cqi.ctypes.data)
        grid1, grid2, grid3 = (np.zeros((14, nsc), np.complex64) for _ in range(3))
        q, d, z = np.zeros(H * QM // 8, np.uint8), np.zeros(H, np.complex64), np.zeros((COLS, nsc), np.complex64)
        pre = capi.DftPrecoding()
        assert lib.srsran_dft_precoding_init_tx(C.byref(pre), L_prb) == 0
        syms = [s for s in range(14) if s % 7 != 3]

        def one_call():
            return lib.srsran_hip_pusch_encode(C.byref(g), None, None, C.byref(sb[0]), O.P(pay), O.P(grid1))

        def one_call_uci():
            return lib.srsran_hip_pusch_encode(C.byref(g), C.byref(uci), C.byref(uin), C.byref(sb[0]), O.P(pay), O.P(grid3))

        def three_waits():
            rc = lib.srsran_hip_ulsch_encode(C.byref(tb), COLS, C.byref(sb[0]), O.P(pay), O.P(q))
            rc |= 0 if lib.srsran_hip_modulate_bytes(MOD, O.P(q), O.P(d), H * QM, seed, 1, 1.0) == H else 1
            rc |= lib.srsran_dft_precoding(C.byref(pre), O.P(d), O.P(z), L_prb, COLS)
            for row, s in enumerate(syms):
                grid2[s] = z[row]
            return rc

        routes = (("one_call", one_call), ("three_waits", three_waits), ("one_call_uci", one_call_uci))
        tm = {k: [] for k, _ in routes}
        for i in range(warm + args.calls):
            for what, fn in routes:
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert rc == 0, (name, what, rc, capi.last_error())
                if i >= warm:
                    tm[what].append(dt)
            if i == 0:
                err = float(np.abs(grid1 - grid2).max())
                assert err < 1e-4 and np.abs(grid2).max() > 0.1, (name, err)
        lib.srsran_dft_precoding_free(C.byref(pre))
        row = dict(grant=name, L_prb=L_prb, nof_re=H, tbs=tbs, calls=args.calls)
        for k in tm:
            row[k + "_p50_us"], row[k + "_p90_us"] = round(pct(tm[k], 0.5), 1), round(pct(tm[k], 0.9), 1)
        rows_out.append(row)
        print("%-7s nof_re %5d tbs %5d | one call p50 %6.1f p90 %6.1f us | three waits p50 %6.1f p90 %6.1f us | one call with UCI %s p50 %6.1f p90 %6.1f us" %
              (name, H, tbs, row["one_call_p50_us"], row["one_call_p90_us"], row["three_waits_p50_us"], row["three_waits_p90_us"], UCI, row["one_call_uci_p50_us"],
               row["one_call_uci_p90_us"]), flush=True)
    line = json.dumps({"tool": "pusch_tx_time", "unit": "us, host to host", "mod": "16qam", "uci": UCI, "rows": rows_out})
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
