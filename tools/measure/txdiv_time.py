#!/usr/bin/env python3
"""Host-to-host latency of the transmit-diversity PDSCH codeword calls (include/srsran_amd/phy_chan_abi.h) against the per-stage path through the library.

receive   A: one srsran_hip_pdsch_decode_txdiv
          B: srsran_predecoding_diversity_multi + srsran_layerdemap_diversity (host buffers) + srsran_hip_pdsch_decode with ce == NULL
transmit  A: one srsran_hip_pdsch_encode_txdiv
          B: srsran_hip_pdsch_encode (two layers) + srsran_layermap_diversity + srsran_precoding_diversity
for a 100-PRB 64-QAM grant (15000 REs, tbs 75376) and a 6-PRB one (QPSK, 300 REs, tbs 328), on 2 ports x 1 and 2 receive antennas and 4 ports x 2.  A and B
alternate call by call in one loop after a warm-up of both; every pair of results is compared.  p50 / p90 of the timed calls in microseconds; one JSON
line at the end.

    python tools/measure/txdiv_time.py [--calls 300] [--out FILE]
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
import srslte_amd as S
from srslte_amd import capi

GRANTS = [(3, 75376, 15000), (1, 328, 300)]  # mod, tbs, nof_re
ANTENNAS = [(2, 1), (2, 2), (4, 2)]          # ports, receive antennas
SB, ITERS, SCALING = 18600, 10, 0.8


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def planes(arrs):
    return capi.PlaneArray(*[a.ctypes.data for a in arrs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = S.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    capi.check(lib.srsran_hip_set_device(0), "set_device")
    rows_out = []
    warm = max(20, args.calls // 10)
    for mod, tbs, n in GRANTS:
        for ports, nrx in ANTENNAS:
            Qm = O.QM[mod]
            rng = np.random.default_rng(n + ports + nrx)
            nb = O.cbsegm(tbs)["C"]
            seed = O.pdsch_seed(0x1234, 0, 10, 301)
            payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
            # transmit, both ways
            gt = capi.HipPdschTxdivTx(capi.HipGrantTb(mod, tbs, 0, n, seed, 0, 0, 2), ports, SCALING)
            g1 = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, 0, n, seed, 0, 0, 2), 1.0)
            txrows = [[np.zeros(SB, np.uint8) for _ in range(nb)] for _ in range(2)]
            sbt = [capi.SoftbufferTx(nb, SB, (C.c_void_p * nb)(*[r.ctypes.data for r in rr])) for rr in txrows]
            out_a, out_b = np.zeros((ports, n), np.complex64), np.zeros((ports, n), np.complex64)
            d, x = np.zeros(n, np.complex64), np.zeros((ports, n // ports), np.complex64)
            pa, pb, px = planes(list(out_a)), planes(list(out_b)), planes(list(x))

            def tx_a():
                return lib.srsran_hip_pdsch_encode_txdiv(C.byref(gt), C.byref(sbt[0]), O.P(payload), pa)

            def tx_b():
                rc = lib.srsran_hip_pdsch_encode(C.byref(g1), C.byref(sbt[1]), O.P(payload), O.P(d))
                lib.srsran_layermap_diversity(O.P(d), px, ports, n)
                return rc if rc else (0 if lib.srsran_precoding_diversity(px, pb, ports, n // ports, SCALING) == n else -1)

            assert tx_a() == 0 and tx_b() == 0, capi.last_error()
            # receive: the transmitted planes through a channel that is constant over each pair / quad, a little noise
            t = 0.9 + 0.1 * (rng.standard_normal((ports, nrx, n // ports)) + 1j * rng.standard_normal((ports, nrx, n // ports)))
            h = np.ascontiguousarray(np.repeat(t, ports, axis=2).astype(np.complex64))
            sigma = 10 ** (-{1: 9.0, 3: 28.0}[mod] / 20) / np.sqrt(2)
            y = np.einsum("krn,kn->rn", h.astype(np.complex128), out_a.astype(np.complex128)) + sigma * (rng.standard_normal((nrx, n)) + 1j * rng.standard_normal((nrx, n)))
            y = np.ascontiguousarray(y.astype(np.complex64))
            gr = capi.HipPdschTxdivRx(capi.HipGrantTb(mod, tbs, 0, n, seed, ITERS, 0, 2), ports, nrx, SCALING, 0)
            g0 = capi.HipPdschRx(capi.HipGrantTb(mod, tbs, 0, n, seed, ITERS, 0, 2), 1.0, 0.0)
            sbr = []
            for _ in range(2):
                rows = [np.zeros(SB, np.int16) for _ in range(nb)]
                keep = [np.zeros(SB // 8, np.uint8) for _ in range(nb)]
                flags = np.zeros(nb, np.bool_)
                sbr.append((capi.SoftbufferRx(nb, SB, (C.c_void_p * nb)(*[r.ctypes.data for r in rows]), (C.c_void_p * nb)(*[k.ctypes.data for k in keep]),
                                              flags.ctypes.data_as(C.POINTER(C.c_bool)), False), rows, keep, flags))
            py = planes(list(y))
            ph = capi.PlaneMatrix(*[planes([h[k][r] for r in range(nrx)]) for k in range(ports)])
            xe, de = np.zeros((ports, n // ports), np.complex64), np.zeros(n, np.complex64)
            pxe = planes(list(xe))
            data_a, data_b = np.zeros(tbs // 8 + 16, np.uint8), np.zeros(tbs // 8 + 16, np.uint8)
            res_a, res_b = capi.HipGrantRes(), capi.HipGrantRes()

            def reset(k):
                sbr[k][3][:] = False
                sbr[k][0].tb_crc = False
                for r in sbr[k][1]:
                    r[:] = 0

            def rx_a():
                return lib.srsran_hip_pdsch_decode_txdiv(C.byref(gr), py, ph, C.byref(sbr[0][0]), O.P(data_a), C.byref(res_a))

            def rx_b():
                lib.srsran_predecoding_diversity_multi(py, ph, pxe, None, nrx, ports, n, SCALING)
                lib.srsran_layerdemap_diversity(pxe, O.P(de), ports, n // ports)
                return lib.srsran_hip_pdsch_decode(C.byref(g0), O.P(de), None, C.byref(sbr[1][0]), O.P(data_b), C.byref(res_b))

            tm = {"rx_a": [], "rx_b": [], "tx_a": [], "tx_b": []}
            for k in range(warm + args.calls):
                reset(0)
                reset(1)  # (outside the timed region: a fresh soft buffer for both)
                for name, fn in (("rx_a", rx_a), ("rx_b", rx_b), ("tx_a", tx_a), ("tx_b", tx_b)):
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = (time.perf_counter() - t0) * 1e6
                    assert rc == 0, (name, rc, capi.last_error())
                    if k >= warm:
                        tm[name].append(dt)
                assert res_a.crc_ok == 1 and res_b.crc_ok == 1 and np.array_equal(data_a[:tbs // 8], payload) and np.array_equal(data_b, data_a), (mod, n, ports, nrx)
                assert abs(res_a.avg_iterations_block - res_b.avg_iterations_block) < 1e-6, (mod, n, ports, nrx)
                assert np.array_equal(out_a.view(np.uint32), out_b.view(np.uint32)), (mod, n, ports, nrx)
            row = dict(mod=mod, nof_re=n, tbs=tbs, nof_cb=nb, ports=ports, nof_rx=nrx, calls=args.calls)
            for name in tm:
                row[name + "_p50_us"], row[name + "_p90_us"] = round(pct(tm[name], 0.5), 1), round(pct(tm[name], 0.9), 1)
            rows_out.append(row)
            print("mod %d nof_re %5d tbs %5d (%2d blocks) %d ports x %d rx   receive: one call p50 %6.1f p90 %6.1f us | per stage p50 %6.1f p90 %6.1f us   "
                  "transmit: one call p50 %6.1f p90 %6.1f us | per stage p50 %6.1f p90 %6.1f us" %
                  (mod, n, tbs, nb, ports, nrx, row["rx_a_p50_us"], row["rx_a_p90_us"], row["rx_b_p50_us"], row["rx_b_p90_us"], row["tx_a_p50_us"],
                   row["tx_a_p90_us"], row["tx_b_p50_us"], row["tx_b_p90_us"]), flush=True)
    line = json.dumps({"tool": "txdiv_time", "unit": "us, host to host", "rows": rows_out})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
