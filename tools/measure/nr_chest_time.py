#!/usr/bin/env python3
"""What an NR codeword costs from the slot grid (include/srsran_amd/phy_nr_chan_abi.h: srsran_hip_nr_cw_decode_grid).

    host   a STAND-IN for the route a caller took before the estimator and the de-mapper moved to the device: RE extraction by a precomputed index (the
           model's positions) and a vectorised float32 numpy estimator on the host (least squares, sync and CFO compensation, time average, a 5-tap FIR,
           linear interpolation -- the same passes as srsran_dmrs_sch_estimate, not its bits), then srsran_hip_nr_cw_decode with symbols, ce and the noise
           estimate.  The reference's own CPU time for srsran_dmrs_sch_estimate + srsran_pdsch_nr_get is not what this measures.
    grid   srsran_hip_nr_cw_decode_grid on the grid alone
on a full allocation of 25, 106 and 270 PRB (30 kHz), 256-QAM, 13 symbols behind one control symbol, two DMRS symbols.  The routes alternate call by call in
one loop after a warm-up of both; soft buffers are reset outside the timed region.  Median / p90 of the timed calls in microseconds, host to host.  One JSON
line at the end; the lines are appended to --out.

    python tools/measure/nr_chest_time.py [--calls 300] [--tag NAME] [--out profiles/nr_chest_time.txt]
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

import nr_chest_model as M
import oracle_api as O
from srslte_amd import capi
from test_gpu_nr_chest import _cfg, _channel, _prbs, _put_codeword, _rx
from test_gpu_nr_cw import Softbuffer
from test_nr_chest_abi import grid_of

SHAPES = [("25prb", 25), ("106prb", 106), ("270prb", 270)]
MOD, RATE, SNR_DB = 4, 0.6, 34.0


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


class HostEstimator:
    """the stand-in: everything that depends on the grant alone is prepared once, as a caller's tables would be"""

    def __init__(self, cfg):
        self.sym = M.dmrs_symbols(cfg)
        self.cols, _ = M.pilot_columns(cfg)
        a = np.float32(M.amplitude(cfg))
        self.conj_pilots = np.stack([np.conj(a * M.dmrs_signs(cfg, l)) for l in self.sym]).astype(np.complex64)
        self.idx, self.psym, self.pce = M.positions(cfg)
        self.stride = 2 if cfg["dmrs_type"] == 0 else 3
        self.f = M.smooth_filter()
        self.n = np.arange(self.cols.size, dtype=np.float32)
        self.m = np.arange(self.cols.size * self.stride, dtype=np.float32)
        self.td = [float(M.symbol_distance_s(self.sym[i], self.sym[i + 1], cfg["scs"])) for i in range(len(self.sym) - 1)]
        self.d0 = np.array([float(M.symbol_distance_s(0, l, cfg["scs"])) for l in range(14)], np.float32)

    def run(self, grid):
        """(symbols, ce, noise_estimate)"""
        flat = grid.reshape(-1)
        ls = grid[self.sym][:, self.cols] * self.conj_pilots
        P, n = ls.shape[1], ls.shape[0]
        sync = np.float32(np.mean(-np.angle(np.sum(ls[:, 1:] * np.conj(ls[:, :-1]), axis=1)) / (2 * np.pi)))
        ls = ls * np.exp(2j * np.pi * sync * self.n).astype(np.complex64)[None, :]
        corr = ls.sum(axis=1) / P
        epre = np.float32(np.mean(np.abs(ls) ** 2))
        rsrp = min(np.float32(np.mean(np.abs(corr) ** 2)), np.float32(epre - epre * 1e-7))
        cfo = sum(np.angle(corr[i + 1] * np.conj(corr[i])) / (2 * np.pi * self.td[i] * (n - 1)) for i in range(n - 1))
        arg0 = np.angle(corr[0]) - 2 * np.pi * self.d0[self.sym[0]] * cfo
        corr_l = np.exp(1j * (arg0 + 2 * np.pi * cfo * self.d0)).astype(np.complex64)
        avg = (ls * np.conj(corr_l[self.sym])[:, None]).sum(axis=0) / n
        ext = np.concatenate([[4 * avg[1] - 3 * avg[0], 3 * avg[1] - 2 * avg[0]], avg, [4 * avg[-1] - 3 * avg[-2], 5 * avg[-1] - 4 * avg[-2]]])
        sm = np.convolve(ext, self.f, "valid").astype(np.complex64)
        row = np.empty(P * self.stride, np.complex64)
        d = np.append(sm[1:] - sm[:-1], sm[-1] - sm[-2]) / self.stride
        for r in range(self.stride):
            row[r::self.stride] = sm + d * r
        row *= np.exp(-2j * np.pi * (sync / self.stride) * self.m).astype(np.complex64)
        return flat[self.idx], (row[self.pce] * corr_l[self.psym]).astype(np.complex64), float(epre - rsrp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nr_chest_time.txt"))
    args = ap.parse_args()
    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    assert lib.srsran_hip_set_device(0) == 0 and lib.srsran_hip_warmup(1) == 0
    warm = max(30, args.calls // 10)
    rows = []
    for name, nof_prb in SHAPES:
        rng = np.random.default_rng(nof_prb)
        cfg = _cfg(nof_prb, _prbs(nof_prb, (0, nof_prb)), S=1, L=13)
        grid = np.zeros((14, 12 * nof_prb), np.complex64)
        seed = lib.srsran_hip_sequence_nr_seed(0x4601, 0, 77)
        tb, ocfg, n, payload = _put_codeword(lib, capi, grid, cfg, MOD, RATE, seed, 3, _channel(cfg, rng, 0.03), SNR_DB, rng)
        g, host = grid_of(capi, cfg), HostEstimator(cfg)
        flat = grid.reshape(-1)
        sb, out, res, est = Softbuffer(ocfg.C + 1), np.zeros(tb.tbs // 8 + 16, np.uint8), capi.HipNrTbResult(), capi.HipNrChestRes()
        rx = _rx(capi, tb, n, seed)

        def route_host():
            sym, ce, ne = host.run(grid)
            rx.noise_estimate = ne
            return lib.srsran_hip_nr_cw_decode(C.byref(rx), O.P(sym), O.P(ce), C.byref(sb.c), O.P(out), C.byref(res))

        def route_grid():
            return lib.srsran_hip_nr_cw_decode_grid(C.byref(rx), C.byref(g), O.P(flat), C.byref(sb.c), O.P(out), C.byref(res), C.byref(est))

        tm = {"host": [], "grid": []}
        for it in range(warm + args.calls):
            for what, fn in (("host", route_host), ("grid", route_grid)):
                sb.flags[:] = False  # (outside the timed region: a fresh soft buffer; rv carries NEW_DATA, the rows are not read)
                out[:] = 0
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert rc == 0, (name, what, rc, capi.last_error())
                assert res.crc_ok == 1 and np.array_equal(out[:tb.tbs // 8], payload), (name, what, res.crc_ok, res.all_decoded)
                if it >= warm:
                    tm[what].append(dt)
        row = dict(shape=name, nof_re=n, tbs=int(tb.tbs), code_blocks=int(ocfg.C), calls=args.calls, host_p50_us=round(pct(tm["host"], 0.5), 1),
                   host_p90_us=round(pct(tm["host"], 0.9), 1), grid_p50_us=round(pct(tm["grid"], 0.5), 1), grid_p90_us=round(pct(tm["grid"], 0.9), 1))
        rows.append(row)
        print("%-6s %-7s nof_re %6d  host stand-in + _cw_decode p50 %7.1f p90 %7.1f us | _cw_decode_grid p50 %7.1f p90 %7.1f us" %
              (args.tag, name, n, row["host_p50_us"], row["host_p90_us"], row["grid_p50_us"], row["grid_p90_us"]), flush=True)
    line = json.dumps({"tool": "nr_chest_time", "tag": args.tag, "unit": "us, host to host", "mod": "256QAM", "host_route": "numpy stand-in, not the reference",
                       "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
