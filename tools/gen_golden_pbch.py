#!/usr/bin/env python3
"""Record what the reference's PBCH receiver gives (srsran_pbch_get, decode_frame, srsran_pbch_decode: phch/pbch.c; srsran_chest_dl_estimate in front, as
srsran_ue_mib_decode runs them: ue/ue_mib.c:129-173): tests/golden/pbch_ref.npz.

    python tools/gen_golden_pbch.py          (needs the reference tree)

tools/pbch_ref_wrap.c and the reference files it binds into are compiled where they lie, with the REF_FLAGS of oracle/Makefile, into a temporary directory
(nothing compiled is kept); loaded lazily.  The record holds data only.

Map cases (m_*): 6, 15, 25 PRB x id % 3 in {0, 1, 2} x both prefixes: the indices srsran_pbch_get reads, off grids of slot 1 that hold their own indices.  The
model's table (tests/pbch_model.py) must equal them EXACTLY, which is asserted here.
Stage cases (t_*): for frame_idx 1 .. 4 (and one extended-prefix cell) a soft-bit buffer made by srsran_pbch_encode -- the QPSK symbols of the frames, read
back with srsran_pbch_get, as soft bits -- plus seeded noise; per (nb, dst, src) the reference's rm_f, q->data and verdict (one port's mask).
MIB cases (u_*): srsran_pbch_mib_unpack of every decoded payload and of one MIB per bandwidth.
Call sequences (c_*): srsran_pbch_encode on 1, 2 and 4 ports and srsran_refsignal_cs_put_sf fill subframe 0 of successive radio frames, which go through flat
per-port channels and noise; srsran_chest_dl_estimate (its zeroed configuration: AVERAGE, REFS noise, the Gauss filter made from the noise estimate) and
srsran_pbch_decode follow, the receiver's object carrying its state from call to call.  Per call: the slot-1 rows (4 x 72) of the received grid and of the
estimates, noise_estimate, the return, ports, offset, payload, the hit's (nb, dst, src) -- found again with decode_frame on q->llr --, frame_idx and the rows of
q->llr below it behind the call, and q->d (the last hypothesis tried).  The sequences marked `full` also hold the whole received grid and the pilot rows,
for the calls that estimate on the device.  SEQUENCES lists them with their SNRs; every draw comes from one generator seeded with SEED.

Asserted on the reference ALONE: a first-call hit for each port count with nof_ports given and with 0; a low-SNR sequence whose first hit combines >= 2 frames
with dst != src; a sequence that misses 6 calls, so that the shift at frame_idx 4 runs twice, and then hits; every transmitted MIB that decodes is decoded as
sent; no noise-only call hits.

The float tolerances of d and of the newest soft-bit row are MEASURED here: model against reference, max |a - b| / rms(b) per call; four times the worst
value is stored (the device may fuse a multiply-add where numpy rounds twice).  So that they hide no wrong decision, every recorded call is run again on the
reference's decode_frame with the newest row of every hypothesis (the reference's own, from a run told that port count) perturbed by seeded noise of 10 x that
tolerance x the row's rms: the return, ports, offset and payload must not change.

The time of srsran_chest_dl_estimate + srsran_pbch_decode on the calls tools/measure/pbch_time.py measures is taken here, on this CPU, and stored (ref_time_*)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_api as O  # noqa: E402
import pbch_model as PB  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402
from gen_golden_ctrl import REF_FILES as CTRL_FILES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pbch_ref.npz")
REF_FILES = CTRL_FILES + ["phch/pbch.c", "phch/prb_dl.c"]
SEED = 4021
F32 = np.float32

MAP_CASES = [PB.cell(prb, 0, cid, cp) for prb in (6, 15, 25) for cid in (150, 301, 2) for cp in (7, 6)]  # id % 3 = 0, 1, 2
STAGE_CASES = [("f1", PB.cell(6, 1, 150), 1, 0.9), ("f2", PB.cell(6, 1, 301), 2, 1.1), ("f3", PB.cell(15, 1, 2), 3, 1.4), ("f4", PB.cell(25, 1, 77), 4, 1.6),
               ("f4_ext", PB.cell(6, 1, 10, 6), 4, 1.6)]  # name, cell, frame_idx, noise per soft bit (against +-1/sqrt 2 symbols x -sqrt 2 = +-1)
# name, the receiver's cell, the transmitter's ports, noise per component (against channels of gain 0.6 .. 1.4), noise-only calls in front, the frame of the
# 40 ms the transmitted sequence starts at, calls at most behind the noise-only ones, full
SEQUENCES = [
    ("hi_1p_told1", PB.cell(6, 1, 1), 1, 0.05, 0, 0, 1, True),
    ("hi_1p_told0", PB.cell(6, 0, 1), 1, 0.05, 0, 0, 1, True),
    ("hi_2p_told2", PB.cell(6, 2, 150), 2, 0.05, 0, 0, 1, False),
    ("hi_2p_told0", PB.cell(6, 0, 150), 2, 0.05, 0, 0, 1, True),
    ("hi_4p_told4", PB.cell(6, 4, 33), 4, 0.05, 0, 0, 1, False),
    ("hi_4p_told0", PB.cell(6, 0, 33), 4, 0.05, 0, 0, 1, True),
    ("low_start1", PB.cell(6, 2, 61), 2, 2.1, 0, 1, 6, True),
    ("low_start2", PB.cell(6, 1, 62), 1, 1.8, 0, 2, 6, False),
    ("low_start3", PB.cell(6, 0, 63), 4, 1.3, 0, 3, 6, False),
    ("noise6_then_2p", PB.cell(6, 2, 150), 2, 0.3, 6, 0, 4, True),
    ("ext_1p", PB.cell(6, 1, 7, 6), 1, 0.05, 0, 0, 1, True),
    ("prb15_2p", PB.cell(15, 2, 301), 2, 0.05, 0, 0, 1, False),
    ("prb25_id2_1p", PB.cell(25, 1, 2), 1, 0.05, 0, 0, 1, False),
    ("noise4_told0", PB.cell(6, 0, 150), 2, 0.3, 4, 0, 0, True),
]
TIMED = [("noise4_told0", 0), ("noise4_told0", 3), ("noise6_then_2p", 0), ("noise6_then_2p", 3)]  # (sequence, call): frame_idx 1 and 4 with nof_ports 0 and 2


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libpbch_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_CHEST_DL_C="%s"' % os.path.join(phy, "ch_estimation", "chest_dl.c"),
                                             '-DREF_V37_C="%s"' % os.path.join(phy, "fec", "convolutional", "viterbi37_avx2_16bit.c"), "-shared",
                                             os.path.join(ROOT, "tools", "pbch_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    lib = C.CDLL(so, mode=os.RTLD_LAZY)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    lib.pbch_ref_open.argtypes = [vp, u32]
    lib.pbch_ref_close.restype = None
    lib.pbch_ref_get.argtypes = [vp, vp]
    lib.pbch_ref_encode.argtypes = [vp, vp, u32]
    lib.pbch_ref_cs_put.argtypes = [u32, vp]
    lib.pbch_ref_cs_pilots.argtypes = [vp, u32, vp, vp]
    lib.pbch_ref_set_state.argtypes = [u32, vp]
    lib.pbch_ref_set_state.restype = None
    lib.pbch_ref_get_state.argtypes = [vp, vp]
    lib.pbch_ref_get_state.restype = u32
    lib.pbch_ref_frame.argtypes = [u32, u32, u32, u32, vp, vp]
    lib.pbch_ref_decode.argtypes = [vp, vp, f32, vp, vp, vp]
    lib.pbch_ref_mib_unpack.argtypes = [vp, vp]
    lib.pbch_ref_mib_unpack.restype = None
    lib.pbch_ref_chest_open.argtypes = [vp, u32, vp, vp]
    lib.pbch_ref_chest_close.restype = None
    lib.pbch_ref_chest.argtypes = [vp, vp, vp]
    lib.pbch_ref_time.argtypes = [u32, u32, vp, vp, vp]
    lib.pbch_ref_time.restype = C.c_double
    lib.pbch_ref_told.argtypes = [u32]
    lib.pbch_ref_told.restype = None
    return lib


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def rms(v):
    return float(np.sqrt(np.mean(np.abs(np.asarray(v, np.complex128)) ** 2)))


def cnoise(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def map_case(lib, c):
    assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, 1) == PB.nof_re(c)
    try:
        grid = np.arange(c["cp_nsymb"] * 12 * c["nof_prb"]).astype(np.complex64)  # exact in float32 below 2^24
        out = np.zeros(PB.nof_re(c), np.complex64)
        assert lib.pbch_ref_get(grid.ctypes.data, out.ctypes.data) == PB.nof_re(c)
    finally:
        lib.pbch_ref_close()
    t = out.real.astype(np.uint32)
    assert np.array_equal(t, PB.table(c)), c
    return t


def frame_symbols(lib, c, payload, fr):
    """the QPSK symbols srsran_pbch_encode puts for frame fr of the 40 ms, in srsran_pbch_get's order (the transmitter has one port)"""
    n = 2 * c["cp_nsymb"] * 12 * c["nof_prb"]
    g = np.zeros(n, np.complex64)
    buf = np.array(payload, np.uint8)
    assert lib.pbch_ref_encode(buf.ctypes.data, ptrs([g]), fr) == 0
    return g[n // 2:][PB.table(c)]


def stage_case(lib, rng, name, c, f, sigma):
    nre, nof_bits = PB.nof_re(c), 2 * PB.nof_re(c)
    assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, 1) == nre
    try:
        payload = PB.mib_pack(c["nof_prb"], 0, 2, int(rng.integers(0, 256)) * 4)
        first = int(rng.integers(0, 5 - f))  # the frame of the 40 ms row 0 holds
        llr = np.zeros((4, nof_bits), F32)
        for r in range(f):
            llr[r] = PB.soft_bits(frame_symbols(lib, c, payload, first + r)) + (sigma * rng.standard_normal(nof_bits)).astype(F32)
        lib.pbch_ref_set_state(f, llr.ctypes.data)
        combos = PB.combos(f)
        rm_f, data, hit = np.zeros((len(combos), 120), F32), np.zeros((len(combos), 40), np.uint8), np.zeros(len(combos), np.uint8)
        for i, (nb, dst, src) in enumerate(combos):
            hit[i] = lib.pbch_ref_frame(src, dst, nb + 1, 1, rm_f[i].ctypes.data, data[i].ctypes.data) == 1
        model = PB.try_frames(c, llr, f)
        for i, m in enumerate(model):  # the model is integer-exact
            assert np.array_equal(m["rm_f"].view(np.uint32), rm_f[i].view(np.uint32)) and np.array_equal(m["bits"], data[i]) and PB.verdict(m, 1) == hit[i], (name, i)
        sent = [i for i in range(len(combos)) if hit[i]]
        assert sent and all(np.array_equal(data[i][:24], payload) for i in sent) and not hit.all(), (name, sent)
        print("T %-8s f %d  first frame %d  %2d combinations, %2d hits (all as sent)" % (name, f, first, len(combos), len(sent)))
        return dict(cell=PB.as_row(c), f=np.uint32(f), llr=llr, rm_f=rm_f, data=data, hit=hit, payload=payload)
    finally:
        lib.pbch_ref_close()


def ref_call(lib, c, f_in, llr_in, rx, ce, noise):
    """srsran_pbch_decode from the state given -> dict"""
    lib.pbch_ref_set_state(f_in, llr_in.ctypes.data)
    payload, ports, off = np.zeros(24, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    ret = lib.pbch_ref_decode(rx.ctypes.data, ptrs(ce), C.c_float(noise), payload.ctypes.data, ports.ctypes.data, off.ctypes.data)
    assert ret in (0, 1), ret
    llr, d = np.zeros_like(llr_in), np.zeros(PB.nof_re(c), np.complex64)
    f_out = lib.pbch_ref_get_state(llr.ctypes.data, d.ctypes.data)
    r = dict(ret=ret, ports=int(ports[0]) if ret else 0, off=int(off[0]) if ret else 0, payload=payload if ret else np.zeros(24, np.uint8), f_out=f_out, llr=llr, d=d,
             src=0, dst=0, nb=0)
    if ret:  # which combination it was: decode_frame again on q->llr, which holds the hit's rows
        found = [(nb, dst, src) for nb, dst, src in PB.combos(f_in + 1) if lib.pbch_ref_frame(src, dst, nb + 1, r["ports"], None, None) == 1]
        r["nb"], r["dst"], r["src"] = found[0]
        assert r["off"] == r["dst"] - r["src"] + f_in
    return r


def perturbed_call(lib, rng, c, f_in, llr_in, rx, ce, noise, tol):
    """the reference's decision with the newest row of every hypothesis moved by 10 tol rms(row): -> (ret, ports, off, payload)"""
    f = f_in + 1
    for nant in PB.nant_list(c):
        lib.pbch_ref_told(nant)
        own = ref_call(lib, c, f_in, llr_in, rx, ce, noise)  # told that count alone: q->llr's row f - 1 is this hypothesis's
        lib.pbch_ref_told(c["nof_ports"])
        llr = llr_in.copy()
        row = st_row(own, f_in)
        llr[f - 1] = row + (10 * tol * rms(row) * rng.standard_normal(row.size)).astype(F32)
        lib.pbch_ref_set_state(f, llr.ctypes.data)
        for nb, dst, src in PB.combos(f):
            data = np.zeros(40, np.uint8)
            if lib.pbch_ref_frame(src, dst, nb + 1, nant, None, data.ctypes.data) == 1:
                return 1, nant, dst - src + f - 1, data[:24].copy()
    return 0, 0, 0, np.zeros(24, np.uint8)


def estimate(lib, c, est_ports, pilots, rx):
    n = rx.size
    ce = [np.zeros(n, np.complex64) for _ in range(4)]
    noise = np.zeros(1, F32)
    assert lib.pbch_ref_chest(rx.ctypes.data, ptrs(ce), noise.ctypes.data) == 0
    return ce, float(noise[0])


def run_calls(lib, rng, name, c, grids, sent, full, pilots):
    """the reference's chain over the received grids of a sequence -> list of per-call records; stops behind the first hit"""
    est_ports = c["nof_ports"] or 4
    nof_bits = 2 * PB.nof_re(c)
    assert lib.pbch_ref_chest_open(PB.as_row(c).ctypes.data, est_ports, pilots[0].ctypes.data, pilots[1].ctypes.data) == 0
    recs, f_in, llr_in, dev = [], 0, np.zeros((4, nof_bits), F32), dict(d=0.0, llr=0.0)
    try:
        for i, rx in enumerate(grids):
            ce, noise = estimate(lib, c, est_ports, pilots, rx)
            r = ref_call(lib, c, f_in, llr_in, rx, ce, noise)
            rx_rows, ce_rows = PB.slot1_rows(c, rx), np.array([PB.slot1_rows(c, ce[p]) for p in range(est_ports)])
            # the model, from the reference's state
            res, st, dbg = PB.decode(c, dict(frame_idx=f_in, llr=llr_in), rx_rows, ce_rows, noise)
            assert (res["ret"], res["nof_tx_ports"], res["sfn_offset"], res["src"], res["dst"], res["nb"]) == (r["ret"], r["ports"], r["off"], r["src"], r["dst"], r["nb"]), \
                (name, i, res, r)
            assert np.array_equal(res["payload"], r["payload"]) and st["frame_idx"] == r["f_out"], (name, i)
            last = r["ports"] if r["ret"] else PB.nant_list(c)[-1]
            new_ref = st_row(r, f_in)
            if new_ref is not None:
                dev["llr"] = max(dev["llr"], float(np.abs(dbg["llr_new"][last].astype(np.float64) - new_ref).max()) / rms(new_ref))
            dev["d"] = max(dev["d"], float(np.abs(dbg["d"][last] - r["d"]).max()) / rms(r["d"]))
            if sent[i] is not None and r["ret"]:
                assert np.array_equal(r["payload"], sent[i]), (name, i, "decoded, but not as sent")
            assert sent[i] is not None or r["ret"] == 0, (name, i, "a noise-only call hit")
            rec = dict(rx_rows=rx_rows, ce_rows=ce_rows, noise=F32(noise), f_in=np.uint32(f_in), ret=np.int32(r["ret"]), ports=np.uint32(r["ports"]),
                       off=np.int32(r["off"]), payload=r["payload"], comb=np.array([r["nb"], r["dst"], r["src"]], np.uint32), f_out=np.uint32(r["f_out"]),
                       llr=r["llr"][:r["f_out"]].copy(), d=r["d"], d_nant=np.uint32(last), sent=np.int32(sent[i] is not None))
            if full:
                rec["rx"] = rx
            rec["_state"] = (f_in, llr_in, rx, ce, noise)
            recs.append(rec)
            print("C %-16s call %d  f %d -> %d  ret %d ports %d offset %d (nb %d dst %d src %d)  noise %.3g" %
                  (name, i, f_in, r["f_out"], r["ret"], r["ports"], r["off"], r["nb"], r["dst"], r["src"], noise))
            f_in, llr_in = r["f_out"], r["llr"]
            if r["ret"]:
                break
    finally:
        pass
    return recs, dev


def st_row(r, f_in):
    """the newest row as q->llr holds it behind the call, or None where the call left none to look at (a hit: the hit hypothesis's, which is there too)"""
    f = f_in + 1
    if r["ret"] == 0 and f == 4:
        return r["llr"][2]  # moved down by the shift
    return r["llr"][f - 1]


def sequence(lib, rng, spec):
    name, c, tx_ports, sigma, n_noise, start, n_calls, full = spec
    nre_sf = 2 * c["cp_nsymb"] * 12 * c["nof_prb"]
    assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, tx_ports) == PB.nof_re(c)
    try:
        est_ports = c["nof_ports"] or 4
        pilots = [np.zeros(8 * c["nof_prb"], np.complex64), np.zeros(4 * c["nof_prb"], np.complex64)]
        assert lib.pbch_ref_cs_pilots(PB.as_row(c).ctypes.data, est_ports, pilots[0].ctypes.data, pilots[1].ctypes.data) == 0
        h = np.exp(2j * np.pi * rng.uniform(0, 1, tx_ports)) * rng.uniform(0.6, 1.4, tx_ports)
        sfn0 = int(rng.integers(0, 200)) * 4
        grids, sent = [], []
        for i in range(n_noise):
            grids.append((sigma * cnoise(rng, nre_sf)).astype(np.complex64))
            sent.append(None)
        for i in range(n_calls):
            fr = start + i
            payload = PB.mib_pack(c["nof_prb"], 0, 2, sfn0 + 4 * (fr // 4))
            tx = [np.zeros(nre_sf, np.complex64) for _ in range(tx_ports)]
            for p in range(tx_ports):
                assert lib.pbch_ref_cs_put(p, tx[p].ctypes.data) == 0
            buf = payload.copy()
            assert lib.pbch_ref_encode(buf.ctypes.data, ptrs(tx), fr % 4) == 0
            y = sum(h[p] * tx[p].astype(np.complex128) for p in range(tx_ports)) + sigma * cnoise(rng, nre_sf)
            grids.append(y.astype(np.complex64))
            sent.append(payload)
        recs, dev = run_calls(lib, rng, name, c, grids, sent, full, pilots)
        return recs, dev, pilots
    finally:
        lib.pbch_ref_chest_close()
        lib.pbch_ref_close()


def capture_sequence(lib, rng, told):
    """the first subframe of the recorded capture pbch_1_92M through the reference's chain (pbch_file_test: cell 150, 6 PRB)"""
    cap = np.load(os.path.join(ROOT, "tests", "golden", "sync_captures.npz"))
    x = cap["pbch_1_92M_x"][:1920]
    c = PB.cell(6, told, 150)
    grid = np.ascontiguousarray(O.ofdm_rx(O.ofdm_cfg(6, 0, 0, 0), x[None, :])[0])
    assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, 2) == 240
    try:
        est_ports = told or 4
        pilots = [np.zeros(48, np.complex64), np.zeros(24, np.complex64)]
        assert lib.pbch_ref_cs_pilots(PB.as_row(c).ctypes.data, est_ports, pilots[0].ctypes.data, pilots[1].ctypes.data) == 0
        sent = np.array([int(ch) for ch in "011010000001110000000000"], np.uint8)  # pbch_file_test.c:45-46
        recs, dev = run_calls(lib, rng, "capture_told%d" % told, c, [grid], [sent], True, pilots)
        assert recs[0]["ret"] == 1 and recs[0]["ports"] == 2 and recs[0]["off"] == 0
        return recs, dev, pilots
    finally:
        lib.pbch_ref_chest_close()
        lib.pbch_ref_close()


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    rng = np.random.default_rng(SEED)
    d = {"m_cells": np.array([PB.as_row(c) for c in MAP_CASES]), "t_names": np.array([s[0] for s in STAGE_CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_wrapper(tmp)
        for i, c in enumerate(MAP_CASES):
            d["m_table_%d" % i] = map_case(lib, c)
        print("M %d map cases equal the model's table" % len(MAP_CASES))
        for i, (name, c, f, sigma) in enumerate(STAGE_CASES):
            for k, v in stage_case(lib, rng, name, c, f, sigma).items():
                d["t_%s_%d" % (k, i)] = v
        seqs, worst = [], dict(d=0.0, llr=0.0)
        for spec in SEQUENCES:
            recs, dev, pilots = sequence(lib, rng, spec)
            seqs.append((spec[0], spec[1], spec[7], recs, pilots, spec))
            worst = {k: max(worst[k], dev[k]) for k in worst}
        for told in (2, 0):
            recs, dev, pilots = capture_sequence(lib, rng, told)
            seqs.append(("capture_told%d" % told, PB.cell(6, told, 150), True, recs, pilots, None))
            worst = {k: max(worst[k], dev[k]) for k in worst}
        tol = {k: 4 * v for k, v in worst.items()}
        print("worst deviations of the model from the reference: %s -> tolerances %s" % (worst, tol))
        # the properties the sequences are there for, on the reference alone
        by = {s[0]: s[3] for s in seqs}
        for n in ("hi_1p_told1", "hi_1p_told0", "hi_2p_told2", "hi_2p_told0", "hi_4p_told4", "hi_4p_told0", "ext_1p", "prb15_2p", "prb25_id2_1p"):
            assert len(by[n]) == 1 and by[n][0]["ret"] == 1 and by[n][0]["ports"] == int(re.search(r"(\d)p", n).group(1)), n
        low = [by[n][-1] for n in ("low_start1", "low_start2", "low_start3")]
        assert all(r["ret"] == 1 for r in low) and any(r["comb"][0] >= 1 and r["comb"][1] != r["comb"][2] for r in low), [r["comb"] for r in low]
        n6 = by["noise6_then_2p"]
        assert [int(r["ret"]) for r in n6[:6]] == [0] * 6 and [int(r["f_out"]) for r in n6[:6]] == [1, 2, 3, 3, 3, 3] and n6[-1]["ret"] == 1 and len(n6) > 6
        assert all(r["ret"] == 0 for r in by["noise4_told0"]) and len(by["noise4_told0"]) == 4
        # the tolerances hide no wrong decision
        for name, c, full, recs, pilots, spec in seqs:
            tx_ports = spec[2] if spec else 2
            assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, tx_ports) == PB.nof_re(c)
            try:
                for i, rec in enumerate(recs):
                    f_in, llr_in, rx, ce, noise = rec["_state"]
                    got = perturbed_call(lib, rng, c, f_in, llr_in, rx, ce, noise, max(tol["llr"], 1e-7))
                    want = (int(rec["ret"]), int(rec["ports"]), int(rec["off"]))
                    assert got[:3] == want and np.array_equal(got[3], rec["payload"]), (name, i, got, want)
            finally:
                lib.pbch_ref_close()
        print("every call keeps its return, ports, offset and payload with the newest row moved by 10 x the tolerance")
        # srsran_pbch_mib_unpack on every decoded payload and on one MIB per bandwidth
        mibs = [r["payload"] for s in seqs for r in s[3] if r["ret"]] + \
            [PB.mib_pack(prb, pl, pr, sfn) for prb, pl, pr, sfn in ((6, 1, 0, 0), (15, 0, 1, 4), (25, 1, 2, 1020), (50, 0, 3, 512), (75, 1, 1, 8), (100, 0, 2, 1016))]
        unpacked = np.zeros((len(mibs), 4), np.uint32)
        for i, m in enumerate(mibs):
            buf = np.ascontiguousarray(m, np.uint8)
            lib.pbch_ref_mib_unpack(buf.ctypes.data, unpacked[i].ctypes.data)
            assert tuple(int(v) for v in unpacked[i]) == PB.mib_unpack(m), m
        d["u_payload"], d["u_out"] = np.array(mibs, np.uint8), unpacked
        # the reference's own time on the calls that are measured on the device
        times = []
        for sname, call in TIMED:
            name, c, full, recs, pilots, spec = [s for s in seqs if s[0] == sname][0]
            f_in, llr_in, rx, ce, noise = recs[call]["_state"]
            assert lib.pbch_ref_open(PB.as_row(c).ctypes.data, 2) == PB.nof_re(c)
            assert lib.pbch_ref_chest_open(PB.as_row(c).ctypes.data, c["nof_ports"] or 4, pilots[0].ctypes.data, pilots[1].ctypes.data) == 0
            try:
                lib.pbch_ref_time(20, f_in, llr_in.ctypes.data, rx.ctypes.data, ptrs(ce))
                t = min(lib.pbch_ref_time(200, f_in, llr_in.ctypes.data, rx.ctypes.data, ptrs(ce)) for _ in range(5))
            finally:
                lib.pbch_ref_chest_close()
                lib.pbch_ref_close()
            times.append(t * 1e6)
            print("reference: srsran_chest_dl_estimate + srsran_pbch_decode, %s call %d (frame_idx %d, nof_ports %d): %.1f us" % (sname, call, f_in + 1, c["nof_ports"], t * 1e6))
        d["ref_time_calls"] = np.array(["%s/%d" % t for t in TIMED])
        d["ref_time_us"] = np.array(times, np.float64)
        d["ref_time_cpu"] = np.array(cpu_name())
    d["c_names"] = np.array([s[0] for s in seqs])
    d["c_cells"] = np.array([PB.as_row(s[1]) for s in seqs])
    d["c_full"] = np.array([s[2] for s in seqs], np.uint8)
    d["c_ncalls"] = np.array([len(s[3]) for s in seqs], np.uint32)
    for si, (name, c, full, recs, pilots, spec) in enumerate(seqs):
        if full:
            d["c_pilots0_%d" % si], d["c_pilots1_%d" % si] = pilots
        for i, rec in enumerate(recs):
            for k, v in rec.items():
                if not k.startswith("_"):
                    d["c_%s_%d_%d" % (k, si, i)] = v
    d["d_tol"], d["llr_tol"] = np.float64(tol["d"]), np.float64(tol["llr"])
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(MAP_CASES), "map cases,", len(STAGE_CASES), "stage cases,", len(seqs), "sequences,", sum(len(s[3]) for s in seqs), "calls")


if __name__ == "__main__":
    main()
