#!/usr/bin/env python3
"""Host-to-host latency of the spatial-multiplexing PDSCH grant calls (include/srsran_amd/phy_chan_abi.h) against the per-stage path through the library.

receive   A: one srsran_hip_pdsch_decode_mimo
          B: srsran_hip_predecoding_mimo (host buffers) + srsran_hip_pdsch_decode with ce == NULL per codeword
transmit  A: one srsran_hip_pdsch_encode_mimo
          B: srsran_hip_pdsch_encode per codeword + srsran_hip_precoding_mimo
for a 100-PRB grant of two 64-QAM codewords (15000 REs, tbs 75376 each: 26 code blocks), a 6-PRB one of two QPSK codewords (300 REs, tbs 328 each) and a
one-layer 100-PRB grant (64-QAM, 15000 REs, tbs 75376); two layers: codebook 1 with the MMSE decoder at noise 0 (what srsran_pdsch_decode runs by default),
one layer: codebook 0.  A and B alternate call by call in one loop after a warm-up of both; every pair of results is compared.  p50 / p90 of the timed
calls in microseconds; one JSON line at the end.  Not measured here: kernel times alone, and the reference's CPU time for the same stages.

    python tools/measure/spmux_time.py [--calls 300] [--out FILE]
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
import spmux_model as M
import srslte_amd as S
from srslte_amd import capi

GRANTS = [("100prb_2x64qam", 2, 1, ((3, 75376), (3, 75376)), 15000), ("6prb_2xqpsk", 2, 1, ((1, 328), (1, 328)), 300), ("100prb_1layer_64qam", 1, 0, ((3, 75376),), 15000)]
SB, ITERS, SCALING = 18600, 10, 0.8
MUX = capi.TXSCHEME_SPATIALMUX


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def planes(arrs):
    return capi.PlaneArray(*[a.ctypes.data for a in arrs])


def rx_softbuffer(nb):
    rows = [np.zeros(SB, np.int16) for _ in range(nb)]
    keep = [np.zeros(SB // 8, np.uint8) for _ in range(nb)]
    flags = np.zeros(nb, np.bool_)
    return (capi.SoftbufferRx(nb, SB, (C.c_void_p * nb)(*[r.ctypes.data for r in rows]), (C.c_void_p * nb)(*[k.ctypes.data for k in keep]),
                              flags.ctypes.data_as(C.POINTER(C.c_bool)), False), rows, keep, flags)


def tx_softbuffer(nb):
    rows = [np.zeros(SB, np.uint8) for _ in range(nb)]
    return capi.SoftbufferTx(nb, SB, (C.c_void_p * nb)(*[r.ctypes.data for r in rows])), rows


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
    for name, layers, cb, tbs_mod, n in GRANTS:
        rng = np.random.default_rng(n + layers)
        seeds = [O.pdsch_seed(0x1234, k, 10, 301) for k in range(layers)]
        nb = [O.cbsegm(tbs)["C"] for _, tbs in tbs_mod]
        pays = [rng.integers(0, 256, tbs // 8).astype(np.uint8) for _, tbs in tbs_mod]
        tb_tx = [capi.HipGrantTb(mod, tbs, 0, n, seeds[k], 0, 0, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
        tb_rx = [capi.HipGrantTb(mod, tbs, 0, n, seeds[k], ITERS, 0, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
        # transmit, both ways
        gt = capi.HipPdschMimoTx((capi.HipGrantTb * 2)(*tb_tx), layers, layers, MUX, cb, SCALING)
        g1 = [capi.HipPdschTx(tb_tx[k], 1.0) for k in range(layers)]
        sbt = [[tx_softbuffer(nb[k]) for k in range(layers)] for _ in range(2)]
        sbtp = (C.POINTER(capi.SoftbufferTx) * 2)(*[C.pointer(s[0]) for s in sbt[0]])
        payp = (C.c_void_p * 2)(*[p.ctypes.data for p in pays])
        out_a, out_b, x = np.zeros((2, n), np.complex64), np.zeros((2, n), np.complex64), np.zeros((2, n), np.complex64)
        pa, pb, px = planes(list(out_a)), planes(list(out_b)), planes(list(x))

        def tx_a():
            return lib.srsran_hip_pdsch_encode_mimo(C.byref(gt), sbtp, payp, pa)

        def tx_b():
            for k in range(layers):
                rc = lib.srsran_hip_pdsch_encode(C.byref(g1[k]), C.byref(sbt[1][k][0]), O.P(pays[k]), O.P(x[k]))
                if rc:
                    return rc
            return lib.srsran_hip_precoding_mimo(px, pb, layers, 2, cb, n, SCALING, MUX)

        assert tx_a() == 0 and tx_b() == 0, capi.last_error()
        # receive: the transmitted planes through a well-conditioned channel, noise 35 dB below the signal
        h = M.channel(rng, n)
        sigma = 10 ** (-35 / 20) / np.sqrt(2)
        y = np.einsum("krn,kn->rn", h.astype(np.complex128), out_a.astype(np.complex128)) + sigma * (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))
        y = np.ascontiguousarray(y.astype(np.complex64))
        gr = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tb_rx), layers, layers, MUX, cb, capi.MIMO_DECODER_MMSE, 2, SCALING, 0.0)
        g0 = [capi.HipPdschRx(tb_rx[k], 1.0, 0.0) for k in range(layers)]
        sbr = [[rx_softbuffer(nb[k]) for k in range(layers)] for _ in range(2)]
        sbrp = (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbr[0]])
        py = planes(list(y))
        ph = capi.PlaneMatrix(*[planes([h[k][r] for r in range(2)]) for k in range(2)])
        xe = np.zeros((2, n), np.complex64)
        pxe = planes(list(xe))
        data_a = [np.zeros(tbs // 8 + 16, np.uint8) for _, tbs in tbs_mod]
        data_b = [np.zeros(tbs // 8 + 16, np.uint8) for _, tbs in tbs_mod]
        dap = (C.c_void_p * 2)(*[a.ctypes.data for a in data_a])
        res_a, res_b = (capi.HipGrantRes * 2)(), (capi.HipGrantRes * 2)()

        def reset(side):
            for sb, rows, _, flags in sbr[side]:
                flags[:] = False
                sb.tb_crc = False
                for r in rows:
                    r[:] = 0

        def rx_a():
            return lib.srsran_hip_pdsch_decode_mimo(C.byref(gr), py, ph, sbrp, dap, res_a)

        def rx_b():
            rc = lib.srsran_hip_predecoding_mimo(py, ph, pxe, None, 2, 2, layers, cb, n, MUX, SCALING, 0.0, capi.MIMO_DECODER_MMSE)
            for k in range(layers):
                rc = rc or lib.srsran_hip_pdsch_decode(C.byref(g0[k]), O.P(xe[k]), None, C.byref(sbr[1][k][0]), O.P(data_b[k]), C.byref(res_b[k]))
            return rc

        tm = {"rx_a": [], "rx_b": [], "tx_a": [], "tx_b": []}
        for i in range(warm + args.calls):
            reset(0)
            reset(1)  # (outside the timed region: fresh soft buffers for both)
            for what, fn in (("rx_a", rx_a), ("rx_b", rx_b), ("tx_a", tx_a), ("tx_b", tx_b)):
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert rc == 0, (what, rc, capi.last_error())
                if i >= warm:
                    tm[what].append(dt)
            for k, (_, tbs) in enumerate(tbs_mod):
                assert res_a[k].crc_ok == 1 and res_b[k].crc_ok == 1 and np.array_equal(data_a[k][:tbs // 8], pays[k]) and np.array_equal(data_b[k], data_a[k]), (name, k)
                assert res_a[k].avg_iterations_block == res_b[k].avg_iterations_block, (name, k)
            assert np.array_equal(out_a, out_b), name
        row = dict(grant=name, layers=layers, codebook_idx=cb, nof_re=n, tbs=[t for _, t in tbs_mod], nof_cb=sum(nb), calls=args.calls)
        for what in tm:
            row[what + "_p50_us"], row[what + "_p90_us"] = round(pct(tm[what], 0.5), 1), round(pct(tm[what], 0.9), 1)
        rows_out.append(row)
        print("%-20s nof_re %5d (%2d blocks)   receive: one call p50 %6.1f p90 %6.1f us | per stage p50 %6.1f p90 %6.1f us   "
              "transmit: one call p50 %6.1f p90 %6.1f us | per stage p50 %6.1f p90 %6.1f us" %
              (name, n, sum(nb), row["rx_a_p50_us"], row["rx_a_p90_us"], row["rx_b_p50_us"], row["rx_b_p90_us"], row["tx_a_p50_us"], row["tx_a_p90_us"],
               row["tx_b_p50_us"], row["tx_b_p90_us"]), flush=True)
    line = json.dumps({"tool": "spmux_time", "unit": "us, host to host", "rows": rows_out})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
