#!/usr/bin/env python3
"""What the downlink channel estimator costs on the device, alone and inside the grant call (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_dl_estimate,
srsran_hip_pdsch_decode_txdiv_est), on cells of 25 and 100 PRB with 2 ports and 2 receive antennas (srsue's defaults: AVERAGE, Gauss taps of order 4, REFS):

    stage   srsran_hip_chest_dl_estimate with all four ce grids taken, and with ce == NULL (the measurements only)
    sf      srsran_hip_pdsch_decode_txdiv_sf with the ce grids ALREADY IN HAND (what the stage returned once, outside the timed region): the parent commit's
            route.  It does not include the estimator such a caller runs first on a CPU core
    est     srsran_hip_pdsch_decode_txdiv_est on the received grids alone
    ref     the reference's srsran_chest_dl_estimate_cfg on one CPU core of THIS machine, through the recording wrapper (tools/chest_dl_ref_wrap.c), where the
            reference tree is present; sf + ref is what the parent's route costs a stock UE.  --reference-only measures it where there is no device

The grant is an all-PRB QPSK grant of one code block, one decoder iteration, on random grids (it does not decode: both routes do the same work behind the
front end).  sf and est alternate call by call in one loop after a warm-up of both; soft buffers are reset outside the timed region.  Median / p90 of the
timed calls in microseconds, host to host, and the bytes the host stages per call.  One JSON line at the end.

    python tools/measure/chest_dl_time.py [--calls 300] [--tag NAME] [--out FILE] [--reference-only]
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

import chest_dl_model as M
import pdsch_map_model as PM

PORTS, NRX, CELL_ID, SF_IDX = 2, 2, 302, 1


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def scene(nof_prb):
    rng = np.random.default_rng(nof_prb)
    pts = 14 * 12 * nof_prb
    grids = [(0.7 * (rng.standard_normal(pts) + 1j * rng.standard_normal(pts))).astype(np.complex64) for _ in range(NRX)]
    pilots = [np.exp(2j * np.pi * rng.random(n * nof_prb)).astype(np.complex64) for n in (8, 4)]
    cfg = dict(nof_prb=nof_prb, nof_ports=PORTS, id=CELL_ID, cp_nsymb=7, nof_rx=NRX, sf_idx=SF_IDX, estimator_alg=M.ALG_AVERAGE, noise_alg=M.NOISE_REFS,
               filter_type=M.FILTER_GAUSS, filter_coef=np.array([4.0, 1.0], np.float32), rsrp_neighbour=0, cfo_estimate_enable=1, cfo_estimate_sf_mask=0x3FF)
    return cfg, grids, pilots


def time_reference(calls):
    """{nof_prb: (p50, p90)} of the reference's estimator on one core, or {} without the reference tree"""
    try:
        import gen_golden_chest_dl as G

        if not os.path.isdir(G.ref_flags()[0]):
            print("reference estimator not timed: no reference tree here")
            return {}
        tmp = tempfile.TemporaryDirectory()
        fn = G.load_wrapper(tmp.name)
    except Exception as e:  # noqa: BLE001
        print("reference estimator not timed: %s" % (str(e).splitlines()[0] if str(e) else type(e).__name__))
        return {}
    out = {}
    state = {"noise": np.zeros((4, 4), np.float32), "cfo": np.float32(0)}
    for nof_prb in (25, 100):
        cfg, grids, pilots = scene(nof_prb)
        t = []
        ref_args, keep = G.reference_args(cfg, state, grids, pilots, np.ones(62, np.complex64))
        for it in range(calls + 30):
            t0 = time.perf_counter()
            rc = fn(*ref_args)
            if it >= 30:
                t.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0
        out[nof_prb] = (round(pct(t, 0.5), 1), round(pct(t, 0.9), 1))
        print("ref    %3d PRB  srsran_chest_dl_estimate_cfg on one CPU core (the wrapper allocates its work buffers per call) p50 %7.1f p90 %7.1f us" % ((nof_prb,) + out[nof_prb]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--reference-only", action="store_true")
    args = ap.parse_args()
    ref = time_reference(args.calls)
    rows = []
    if not args.reference_only:
        import oracle_api as O
        from grant_helpers import _matrix, _planes, _rx_softbuffer
        from srslte_amd import capi
        from test_gpu_chest_dl import cfg_struct, state_struct

        lib = capi.lib()
        assert lib.srsran_hip_device_count() > 0, "no HIP device: nothing is measured without one"
        assert lib.srsran_hip_set_device(0) == 0 and lib.srsran_hip_warmup(1) == 0
        warm = max(30, args.calls // 10)
        for nof_prb in (25, 100):
            cfg, grids, pilots = scene(nof_prb)
            pts = grids[0].size
            c, keep = cfg_struct(capi, cfg, pilots, None)
            st = state_struct(capi, {"noise": np.zeros((4, 4)), "cfo": 0.0})
            ce = np.zeros((PORTS, NRX, pts), np.complex64)
            gp, cm = _planes(capi, grids), _matrix(capi, ce)
            eo = capi.HipChestDlRes()
            stage = lambda: lib.srsran_hip_chest_dl_estimate(C.byref(c), C.byref(st), gp, cm, C.byref(eo))  # noqa: E731
            stage0 = lambda: lib.srsran_hip_chest_dl_estimate(C.byref(c), C.byref(st), gp, None, C.byref(eo))  # noqa: E731
            assert stage() == 0, capi.last_error()
            sfd = PM.make(nof_prb, PORTS, CELL_ID, np.ones((2, nof_prb), np.uint8), sf_idx=SF_IDX, lstart=2)
            nof_re = PM.indices(sfd).size
            sf = PM.to_struct(capi, sfd, 0)
            tbs = 6144 - 24
            g = capi.HipPdschTxdivRx(capi.HipGrantTb(1, tbs, 0, nof_re, 12345, 1, 0, 2), PORTS, NRX, 1.0, 0)
            sb = _rx_softbuffer(capi, O.cbsegm(tbs)["C"], np.int16)
            data = np.zeros(tbs // 8 + 16, np.uint8)
            res = (capi.HipGrantRes * 1)()
            sf_call = lambda: lib.srsran_hip_pdsch_decode_txdiv_sf(C.byref(g), C.byref(sf), gp, cm, C.byref(sb[0]), O.P(data), res)  # noqa: E731
            est_call = lambda: lib.srsran_hip_pdsch_decode_txdiv_est(C.byref(g), C.byref(sf), C.byref(c), C.byref(st), gp, C.byref(sb[0]), O.P(data), res, C.byref(eo))  # noqa: E731
            tm = {"stage": [], "stage_null": [], "sf": [], "est": []}
            for it in range(warm + args.calls):
                for what, fn in (("stage", stage), ("stage_null", stage0), ("sf", sf_call), ("est", est_call)):
                    sbx, rws, _, flags = sb  # (outside the timed region: a fresh soft buffer)
                    flags[:] = False
                    sbx.tb_crc = False
                    for r in rws:
                        r[:] = 0
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = (time.perf_counter() - t0) * 1e6
                    assert rc == 0, (nof_prb, what, rc, capi.last_error())
                    if it >= warm:
                        tm[what].append(dt)
            rows_staged = 14 - 2  # the _sf call stages symbol lstart to the last
            staged_sf = (NRX + PORTS * NRX) * rows_staged * 12 * nof_prb * 8
            staged_est = NRX * pts * 8 + 8 * nof_prb * 8
            row = dict(nof_prb=nof_prb, ports=PORTS, nof_rx=NRX, calls=args.calls, nof_re=int(nof_re), staged_bytes_sf=staged_sf, staged_bytes_est=staged_est)
            for k in tm:
                row[k + "_p50_us"], row[k + "_p90_us"] = round(pct(tm[k], 0.5), 1), round(pct(tm[k], 0.9), 1)
            row["est_minus_sf_p50_us"] = round(pct([b - a for a, b in zip(tm["sf"], tm["est"])], 0.5), 1)
            if nof_prb in ref:
                row["ref_p50_us"], row["ref_p90_us"] = ref[nof_prb]
            rows.append(row)
            print("%-6s %3d PRB %dx%d  stage p50 %6.1f p90 %6.1f us (ce NULL: p50 %6.1f) | _txdiv_sf, ce in hand, p50 %6.1f p90 %6.1f us, %d bytes staged | _txdiv_est p50 %6.1f "
                  "p90 %6.1f us, %d bytes staged | est - sf, call by call, p50 %+6.1f us" %
                  (args.tag, nof_prb, PORTS, NRX, row["stage_p50_us"], row["stage_p90_us"], row["stage_null_p50_us"], row["sf_p50_us"], row["sf_p90_us"], staged_sf,
                   row["est_p50_us"], row["est_p90_us"], staged_est, row["est_minus_sf_p50_us"]), flush=True)
    line = json.dumps({"tool": "chest_dl_time", "tag": args.tag, "unit": "us, host to host", "rows": rows, "ref_us": {str(k): v for k, v in ref.items()}})
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
