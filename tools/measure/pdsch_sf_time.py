#!/usr/bin/env python3
"""What RE de-mapping inside the PDSCH grant call costs (include/srsran_amd/phy_chan_abi.h: the _sf forms).

    twin    srsran_hip_pdsch_decode (one port, with the equaliser) / srsran_hip_pdsch_decode_mimo (2x2 large-delay CDD, two codewords) on PRE-EXTRACTED planes
    sf      srsran_hip_pdsch_decode_sf / srsran_hip_pdsch_decode_mimo_sf on the subframe grids the planes came from
on a full allocation of a 6-, a 25- and a 100-PRB cell (FDD subframe 1, normal CP, one control symbol, two on 6 PRB).  The symbols come from the library's own
transmit calls through a mild channel with noise 35 dB down and are put at the grant's REs of random-filled grids, so every call decodes in the minimum of
iterations.  The two routes alternate call by call in one loop after a warm-up of both; soft buffers are reset outside the timed region.  Median / p90 of the
timed calls in microseconds, host to host, and the median of the per-iteration difference: what de-mapping costs on this route (the host's row copies of whole
grids in place of plane copies, the table, one launch).  One JSON line at the end.

    python tools/measure/pdsch_sf_time.py [--calls 300] [--tag NAME] [--out FILE]
    python tools/measure/pdsch_sf_time.py --ref-cpu      no device needed: the reference's srsran_pdsch_get on the same planes, on this host's CPU (needs the
                                                         reference tree and oracle/_ref/libsrsran_ref.so; the wrapper of tools/gen_golden_pdsch_map.py)
The two modes usually run on different machines: the CPU figure is the cost the caller no longer pays, on whatever host measured it, not a like-for-like race.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import oracle_api as O
import pdsch_map_model as PM
import spmux_model as M
from grant_helpers import _matrix, _planes, _rx_softbuffer, _tx_softbuffer
from srslte_amd import capi

#         name    PRBs mod tbs    control symbols
CELLS = [("6prb", 6, 1, 600, 2), ("25prb", 25, 2, 6200, 1), ("100prb", 100, 3, 75376, 1)]
ROUTES = [("single", 1, 1), ("cdd", 2, 2)]  # name, ports, receive antennas
ITERS, SCALING = 10, 0.8
vp = C.c_void_p


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def description(nof_prb, ports, lstart):
    return PM.make(nof_prb, ports, 1, np.ones((2, nof_prb), np.uint8), sf_idx=1, lstart=lstart)


def ref_cpu(args):
    from gen_golden_pdsch_map import load_wrap, ref_args

    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_wrap(tmp)
        for name, nof_prb, _, _, lstart in CELLS:
            for route, ports, nrx in ROUTES:
                sfd = description(nof_prb, ports, lstart)
                n, planes = PM.indices(sfd).size, nrx * (1 + ports)
                rng = np.random.default_rng(nof_prb)
                grids = [np.ascontiguousarray(M.cn(rng, PM.grid_points(sfd)).astype(np.complex64)) for _ in range(planes)]
                outs = [np.zeros(n, np.complex64) for _ in range(planes)]
                a, _keep = ref_args((nof_prb, ports, 1, 7, 0, 1, lstart, 7, 7), sfd["prb"], grids, outs)
                tm = []
                for i in range(args.calls + 30):
                    t0 = time.perf_counter()
                    got = fn(*a)
                    tm.append((time.perf_counter() - t0) * 1e6)
                    assert got == n
                tm = tm[30:]
                rows.append(dict(cell=name, route=route, planes=planes, nof_re=n, p50_us=round(pct(tm, 0.5), 1), p90_us=round(pct(tm, 0.9), 1)))
                print("%-6s %-6s %-6s %2d x srsran_pdsch_get of %5d REs on the CPU: p50 %6.1f p90 %6.1f us" % (args.tag, name, route, planes, n, rows[-1]["p50_us"], rows[-1]["p90_us"]),
                      flush=True)
    return {"tool": "pdsch_sf_time", "mode": "ref-cpu", "tag": args.tag, "unit": "us, all planes of one call", "rows": rows}


def gpu(args):
    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
    assert lib.srsran_hip_set_device(0) == 0 and lib.srsran_hip_warmup(1) == 0
    warm = max(30, args.calls // 10)
    rows = []
    for name, nof_prb, mod, tbs, lstart in CELLS:
        for route, ports, nrx in ROUTES:
            sfd = description(nof_prb, ports, lstart)
            idx = PM.indices(sfd)
            n, ncw = idx.size, ports
            rng = np.random.default_rng(n)
            nb = O.cbsegm(tbs)["C"]
            seeds = [O.pdsch_seed(0x1234, k, 10, 301) for k in range(2)]
            pays = [rng.integers(0, 256, tbs // 8).astype(np.uint8) for _ in range(ncw)]
            sigma = 10 ** (-35 / 20) / np.sqrt(2)
            tb = lambda k, iters: capi.HipGrantTb(mod, tbs, 0, n, seeds[k], iters, 0, 1)  # noqa: E731
            p = np.zeros((ports, n), np.complex64)
            sbt = [_tx_softbuffer(capi, nb) for _ in range(ncw)]
            if route == "single":
                assert lib.srsran_hip_pdsch_encode(C.byref(capi.HipPdschTx(tb(0, 0), SCALING)), C.byref(sbt[0][0]), O.P(pays[0]), O.P(p[0])) == 0
                h = np.ascontiguousarray((0.9 + 0.1 * M.cn(rng, (1, 1, n))).astype(np.complex64))
            else:
                gt = capi.HipPdschMimoTx((capi.HipGrantTb * 2)(tb(0, 0), tb(1, 0)), 2, 2, capi.TXSCHEME_CDD, 0, SCALING)
                assert lib.srsran_hip_pdsch_encode_mimo(C.byref(gt), (C.POINTER(capi.SoftbufferTx) * 2)(*[C.pointer(s[0]) for s in sbt]),
                                                        (vp * 2)(*[a.ctypes.data for a in pays]), _planes(capi, list(p))) == 0
                h = M.channel(rng, n)
            y = np.einsum("krn,kn->rn", h.astype(np.complex128), p.astype(np.complex128))
            y = np.ascontiguousarray((y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))).astype(np.complex64))
            pts = PM.grid_points(sfd)
            gy = np.ascontiguousarray(M.cn(rng, (nrx, pts)).astype(np.complex64))
            gh = np.ascontiguousarray(M.cn(rng, (ports, nrx, pts)).astype(np.complex64))
            gy[:, idx], gh[:, :, idx] = y, h
            sf = PM.to_struct(capi, sfd, 0)
            sbs = [_rx_softbuffer(capi, nb, np.int16) for _ in range(ncw)]
            data, res = [np.zeros(tbs // 8 + 16, np.uint8) for _ in range(ncw)], (capi.HipGrantRes * 2)()
            if route == "single":
                g = capi.HipPdschRx(tb(0, ITERS), SCALING, 0.0)
                twin = lambda: lib.srsran_hip_pdsch_decode(C.byref(g), O.P(y[0]), O.P(h[0][0]), C.byref(sbs[0][0]), O.P(data[0]), res)  # noqa: E731
                sfc = lambda: lib.srsran_hip_pdsch_decode_sf(C.byref(g), C.byref(sf), O.P(gy[0]), O.P(gh[0][0]), C.byref(sbs[0][0]), O.P(data[0]), res)  # noqa: E731
            else:
                g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(tb(0, ITERS), tb(1, ITERS)), 2, 2, capi.TXSCHEME_CDD, 0, capi.MIMO_DECODER_MMSE, 2, SCALING, 0.0)
                py, ph, pgy, pgh = _planes(capi, list(y)), _matrix(capi, h), _planes(capi, list(gy)), _matrix(capi, gh)
                sbp, dp = (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbs]), (vp * 2)(*[a.ctypes.data for a in data])
                twin = lambda: lib.srsran_hip_pdsch_decode_mimo(C.byref(g), py, ph, sbp, dp, res)  # noqa: E731
                sfc = lambda: lib.srsran_hip_pdsch_decode_mimo_sf(C.byref(g), C.byref(sf), pgy, pgh, sbp, dp, res)  # noqa: E731
            tm = {"twin": [], "sf": []}
            for i in range(warm + args.calls):
                for what, fn in (("twin", twin), ("sf", sfc)):
                    for sb, rws, _, flags in sbs:  # (outside the timed region: a fresh soft buffer)
                        flags[:] = False
                        sb.tb_crc = False
                        for r in rws:
                            r[:] = 0
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = (time.perf_counter() - t0) * 1e6
                    assert rc == 0, (name, route, what, rc, capi.last_error())
                    for k in range(ncw):
                        assert res[k].crc_ok == 1 and np.array_equal(data[k][:tbs // 8], pays[k]), (name, route, what, k)
                    if i >= warm:
                        tm[what].append(dt)
            row = dict(cell=name, route=route, planes=nrx * (1 + ports), nof_re=n, nof_cb=nb * ncw, calls=args.calls, twin_p50_us=round(pct(tm["twin"], 0.5), 1),
                       twin_p90_us=round(pct(tm["twin"], 0.9), 1), sf_p50_us=round(pct(tm["sf"], 0.5), 1), sf_p90_us=round(pct(tm["sf"], 0.9), 1),
                       sf_minus_twin_p50_us=round(pct([b - a for a, b in zip(tm["twin"], tm["sf"])], 0.5), 1))
            rows.append(row)
            print("%-6s %-6s %-6s %2d planes nof_re %5d (%2d blocks)   twin p50 %6.1f p90 %6.1f us | _sf p50 %6.1f p90 %6.1f us | _sf - twin, call by call, p50 %+5.1f us" %
                  (args.tag, name, route, row["planes"], n, row["nof_cb"], row["twin_p50_us"], row["twin_p90_us"], row["sf_p50_us"], row["sf_p90_us"], row["sf_minus_twin_p50_us"]),
                  flush=True)
    return {"tool": "pdsch_sf_time", "mode": "gpu", "tag": args.tag, "unit": "us, host to host", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--ref-cpu", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    line = json.dumps(ref_cpu(args) if args.ref_cpu else gpu(args))
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
