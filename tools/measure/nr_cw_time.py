#!/usr/bin/env python3
"""Host-to-host latency of the NR codeword calls (include/srsran_amd/phy_nr_chan_abi.h) against the per-stage calls that did the same work before them.

receive   A: one srsran_hip_nr_cw_decode with channel estimates
          B: srsran_predecoding_single + srsran_demod_soft_demodulate_b + negate (host) + srsran_sequence_apply_c + srsran_hip_sch_nr_decode_tb
transmit  A: one srsran_hip_nr_cw_encode
          B: srsran_hip_sch_nr_encode_tb + bit packing (host) + srsran_hip_modulate_bytes with scrambling
for the eight shapes of tests/test_gpu_nr_cw.py and one 8-block 256-QAM transport block (12672 REs, the size of a 100 MHz slot).  A and B alternate call by
call in one loop after a warm-up of both; every pair of results is compared.  p50 / p90 of the timed calls in microseconds; one JSON line at the end.

    python tools/measure/nr_cw_time.py [--calls 300] [--out FILE]
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

QM = {1: 2, 2: 4, 3: 6, 4: 8}
SHAPES = [(1, 24, 24, 0.5), (1, 156, 120, 0.4), (2, 513, 1032, 0.5), (2, 1999, 3848, 0.48), (3, 2049, 4104, 0.35), (3, 2050, 9480, 0.8),
          (4, 2100, 9000, 0.55), (4, 4133, 25104, 0.76), (4, 12672, 67368, 0.67)]
ESN0 = {1: 6.0, 2: 13.0, 3: 19.0, 4: 26.0}
SBW, DS = 66 * 384, 8448 // 8


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = S.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    capi.check(lib.srsran_hip_set_device(0), "set_device")
    dec_tb, enc_tb = lib.srsran_hip_sch_nr_decode_tb, lib.srsran_hip_sch_nr_encode_tb
    dec_tb.restype, dec_tb.argtypes = C.c_int, [C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    enc_tb.restype, enc_tb.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
    rows_out = []
    warm = max(20, args.calls // 10)
    for mod, n, tbs, R in SHAPES:
        G, seed = n * QM[mod], lib.srsran_hip_sequence_nr_seed(0x4601, 0, 500)
        cfg = O.sch_nr_tb_info(tbs, R, mod, G, 1, 0)
        cfg.Nref = (66 if cfg.bg == 0 else 50) * cfg.Z
        rng = np.random.default_rng(n)
        payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
        e_tx = O.sch_nr_encode_tb(cfg, 0, payload)
        d = O.modulate_bytes(mod, np.packbits(e_tx), G, seed, True, 1.0).astype(np.complex128)
        sigma = np.sqrt(10.0 ** (-ESN0[mod] / 10.0) / 2.0)
        d = d + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        h = rng.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
        y, h = (d * h).astype(np.complex64), h.astype(np.complex64)
        max_cb = cfg.C
        rows = [np.zeros(SBW, np.int8) for _ in range(max_cb)]
        keep = [np.zeros(DS, np.uint8) for _ in range(max_cb)]
        flags = np.zeros(max_cb, np.bool_)
        sb = capi.SoftbufferRx(max_cb, SBW, (C.c_void_p * max_cb)(*[r.ctypes.data for r in rows]), (C.c_void_p * max_cb)(*[k.ctypes.data for k in keep]),
                               flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
        tb = capi.HipNrTb(R, tbs, mod, 0, 1, G, 0, 0, 0, 0, 0)
        g = capi.HipNrCwRx(capi.HipNrTb(R, tbs, mod, 0x100, 1, G, 0, 0, 0, 0, 0), n, seed, 0.8, 6, 0.0, 0)
        res = capi.HipNrTbResult()
        out_a, out_b = np.zeros(tbs // 8, np.uint8), np.zeros(tbs // 8, np.uint8)
        x, llr, e = np.zeros(n, np.complex64), np.zeros(G, np.int8), np.zeros(G, np.int8)
        crc, avg = C.c_bool(False), C.c_float(0)

        def rx_a():
            flags[:] = False
            return lib.srsran_hip_nr_cw_decode(C.byref(g), O.P(y), O.P(h), C.byref(sb), O.P(out_a), C.byref(res))

        def rx_b():
            flags[:] = False
            lib.srsran_predecoding_single(O.P(y), O.P(h), O.P(x), None, n, 1.0, 0.0)
            lib.srsran_demod_soft_demodulate_b(mod, O.P(x), O.P(llr), n)
            np.negative(llr, out=llr)
            lib.srsran_sequence_apply_c(O.P(llr), O.P(e), G, seed)
            return dec_tb(0.8, 6, C.byref(tb), O.P(e), C.byref(sb), O.P(out_b), C.byref(crc), C.byref(avg))

        gt = capi.HipNrCwTx(tb, n, seed, 1.0, 0)
        sym_a, sym_b, bits = np.zeros(n, np.complex64), np.zeros(n, np.complex64), np.zeros(G, np.uint8)

        def tx_a():
            return lib.srsran_hip_nr_cw_encode(C.byref(gt), O.P(payload), O.P(sym_a))

        def tx_b():
            rc = enc_tb(C.byref(tb), O.P(payload), O.P(bits))
            packed = np.packbits(bits)
            return rc if rc else (0 if lib.srsran_hip_modulate_bytes(mod, O.P(packed), O.P(sym_b), G, seed, 1, 1.0) == n else -1)

        t = {"rx_a": [], "rx_b": [], "tx_a": [], "tx_b": []}
        for k in range(warm + args.calls):
            for name, fn in (("rx_a", rx_a), ("rx_b", rx_b), ("tx_a", tx_a), ("tx_b", tx_b)):
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert rc == 0, (name, rc, capi.last_error())
                if k >= warm:
                    t[name].append(dt)
            assert res.crc_ok == 1 and crc.value and np.array_equal(out_a, payload) and np.array_equal(out_b, payload), (mod, n)
            assert abs(res.avg_iter - avg.value) < 1e-6 and np.array_equal(sym_a.view(np.uint32), sym_b.view(np.uint32)), (mod, n)
        row = dict(mod=mod, nof_re=n, tbs=tbs, nof_cb=int(cfg.C), Z=int(cfg.Z), calls=args.calls)
        for name in t:
            row[name + "_p50_us"], row[name + "_p90_us"] = round(pct(t[name], 0.5), 1), round(pct(t[name], 0.9), 1)
        rows_out.append(row)
        print("mod %d nof_re %5d tbs %5d (%d blocks, Z %3d)   receive: one call p50 %6.1f p90 %6.1f us | staged p50 %6.1f p90 %6.1f us   "
              "transmit: one call p50 %6.1f p90 %6.1f us | staged p50 %6.1f p90 %6.1f us" %
              (mod, n, tbs, cfg.C, cfg.Z, row["rx_a_p50_us"], row["rx_a_p90_us"], row["rx_b_p50_us"], row["rx_b_p90_us"], row["tx_a_p50_us"],
               row["tx_a_p90_us"], row["tx_b_p50_us"], row["tx_b_p90_us"]), flush=True)
    line = json.dumps({"tool": "nr_cw_time", "unit": "us, host to host", "rows": rows_out})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
