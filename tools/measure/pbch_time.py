#!/usr/bin/env python3
"""What PBCH / MIB decoding costs in one device call (include/srsran_amd/phy_pbch_abi.h), on the recorded 6-PRB calls of tests/golden/pbch_ref.npz:

    est_f1_p0   srsran_hip_pbch_decode_est, frame_idx 1, nof_ports 0 (3 hypotheses x 4 combinations: 12 waves behind the estimator)
    est_f4_p0   frame_idx 4, nof_ports 0 (3 x 30: 90 waves)
    est_f1_p2   frame_idx 1, nof_ports 2 (4 waves)
    est_f4_p2   frame_idx 4, nof_ports 2 (30 waves)
    multi8      srsran_hip_pbch_decode_multi of 8 cells at frame_idx 4, nof_ports 0 (720 waves), estimates given
All four inputs are noise-only calls, so every hypothesis is tried by the reference too: its worst case.  Host to host around the C call, which ends in the
call's host wait, after a warm-up; the caller's state is put back before every call (a copy of 7.5 KB, inside the timed window on both sides); median / p90
of the timed calls in microseconds.  Next to each est_* line stands the reference's own time for srsran_chest_dl_estimate + srsran_pbch_decode on the same
input, taken by tools/gen_golden_pbch.py on the CPU named in the record -- another machine's CPU, so the two columns are a statement about the two paths as
users would run them, not a controlled comparison.  One JSON line at the end; the lines are appended to --out.

    python tools/measure/pbch_time.py [--calls 400] [--tag NAME] [--out profiles/pbch_time.txt]
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

import pbch_model as PB
from srslte_amd import capi
from test_gpu_pbch import Planes, cell_struct, est_struct, state_struct


def pct(t, q):
    t = sorted(t)
    return t[min(len(t) - 1, int(len(t) * q))]


def timed(fn, calls, warm=30):
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
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbch_time.txt"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.srsran_hip_device_count() > 0, "no HIP device"
    capi.check(L.srsran_hip_warmup(1), "warmup")
    d = np.load(os.path.join(ROOT, "tests", "golden", "pbch_ref.npz"))
    seqs = {s["name"]: s for s in PB.record_sequences(d)}
    ref_us = {str(k): float(v) for k, v in zip(d["ref_time_calls"], d["ref_time_us"])}
    cpu = str(d["ref_time_cpu"])
    result = {"tag": a.tag, "calls": a.calls, "ref_cpu": cpu}
    lines = []
    for name, sname, i in (("est_f1_p0", "noise4_told0", 0), ("est_f4_p0", "noise4_told0", 3), ("est_f1_p2", "noise6_then_2p", 0), ("est_f4_p2", "noise6_then_2p", 3)):
        s = seqs[sname]
        c, call = s["cell"], s["calls"][i]
        est, keep = est_struct(c, s["pilots"])
        start = state_struct(c, PB.state_before(c, s, i))
        state, cs, res, out, es = capi.HipPbchState(), cell_struct(c), capi.HipPbchRes(), capi.HipChestDlRes(), capi.HipChestDlState()
        rx = np.ascontiguousarray(call["rx"])
        y = (C.c_void_p * 4)(rx.ctypes.data, None, None, None)

        def one():
            C.memmove(C.byref(state), C.byref(start), C.sizeof(state))
            assert L.srsran_hip_pbch_decode_est(C.byref(cs), C.byref(est), C.byref(es), C.byref(state), y, C.byref(res), C.byref(out)) == 0

        p50, p90 = timed(one, a.calls)
        assert res.ret == int(call["ret"]) and state.frame_idx == int(call["f_out"])
        waves = len(PB.nant_list(c)) * len(PB.combos(int(call["f_in"]) + 1))
        ref = ref_us["%s/%d" % (sname, i)]
        result[name] = {"waves": waves, "p50_us": p50, "p90_us": p90, "ref_us": round(ref, 1)}
        lines.append("%-10s %3d waves  p50 %8.1f us  p90 %8.1f us   reference %8.1f us on %s: the %s is larger" %
                     (name, waves, p50, p90, ref, cpu, "reference's time" if ref > p50 else "device call's time"))
    s = seqs["noise4_told0"]
    c, call, n = s["cell"], s["calls"][3], 8
    cells = (capi.HipPbchCell * n)(*[cell_struct(c) for _ in range(n)])
    start = state_struct(c, PB.state_before(c, s, 3))
    states = [capi.HipPbchState() for _ in range(n)]
    sp = (C.POINTER(capi.HipPbchState) * n)(*[C.pointer(st) for st in states])
    pl = Planes(c, call)
    rx, ce, noise = (C.c_void_p * n)(*[pl.rx.ctypes.data] * n), ((C.c_void_p * 4) * n)(*[pl.ptr] * n), (C.c_float * n)(*[pl.noise] * n)
    res = (capi.HipPbchRes * n)()

    def multi():
        for st in states:
            C.memmove(C.byref(st), C.byref(start), C.sizeof(st))
        assert L.srsran_hip_pbch_decode_multi(n, cells, sp, rx, ce, noise, res) == 0

    p50, p90 = timed(multi, a.calls)
    result["multi8"] = {"waves": 720, "p50_us": p50, "p90_us": p90}
    lines.append("%-10s 720 waves  p50 %8.1f us  p90 %8.1f us   (%.1f us per cell; estimates given, no estimator in the call)" % ("multi8", p50, p90, p50 / n))
    text = "\n".join(["# pbch_time %s calls=%d" % (a.tag, a.calls)] + lines + [json.dumps(result)])
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
