#!/usr/bin/env python3
"""Record what the reference's PCFICH and PHICH give (regs_pcfich_init / regs_phich_init: phch/regs.c; srsran_pcfich_decode: phch/pcfich.c; srsran_phich_decode:
phch/phich.c) on seeded control regions that its own transmitters filled, and what its whole control chain gives on seeded subframes: tests/golden/ctrl_ref.npz.

    python tools/gen_golden_ctrl.py          (needs the reference tree)

tools/ctrl_ref_wrap.c and the reference files it binds into are compiled where they lie, with the REF_FLAGS of oracle/Makefile, into a temporary directory
(nothing compiled is kept); loaded lazily.  The record holds data only.

Map cases (m_*): a description, the 16 indices srsran_regs_pcfich_get reads, srsran_regs_phich_ngroups and per group the 12 indices srsran_regs_phich_get reads --
read off grids that hold their own indices.  The model's tables (tests/ctrl_model.py) must equal them EXACTLY, which is asserted here.
Signal cases (s_*): ports 1, 2 and 4 with 1 and 2 receive antennas, a one-port region with noise_estimate > 0 (it enters unhalved), an extended-prefix region,
each of CFI 1, 2 and 3, and one region whose PCFICH REs carry minus the sum of the three code words, so that all three correlations are negative: the reference
returns cfi 1, corr 0 there (asserted).  srsran_pcfich_encode and srsran_phich_encode fill the port grids: ACK and NACK on several sequences of one group at once,
a second group with two sequences at once, and two resources nobody transmitted; per-(port, antenna) channels (a random complex gain with a 5 % ripple per RE)
and noise follow.  Recorded per region: the description, the rows 0 .. 2 of the grids and estimates, the reference's cfi, corr, data_f and d, and per resource
its ack_value, distance, data_rx and z.
Subframe cases (e_*): srsran_refsignal_cs_put_sf, srsran_pcfich_encode, srsran_phich_encode and srsran_pdcch_encode fill whole subframes, which go through flat
per-pair channels and noise; the reference's own chain -- srsran_chest_dl_estimate_cfg, srsran_pcfich_decode, the TDD rule of ue_dl.c:331 where the case sets
cfi3_to_2, srsran_pdcch_extract_llr, srsran_pdcch_dci_decode, srsran_phich_decode -- gives the recorded CFI, payloads, CRC remainders and ACKs.  In the cfi3_to_2
case the PCFICH says 3 and the DCIs lie in the region of CFI 2.

The float tolerances are MEASURED here: the deviation of the model from the reference, max |a - b| / rms(b) per case, for data_f, corr (against |corr|), data_rx
and distance (each against the rms over the case's resources); four times the worst value is stored (the device may fuse a multiply-add where numpy rounds
twice).  So that they hide no wrong decision it is asserted ON THE REFERENCE ALONE that in every signal case but the non-positive one the best correlation leads the
second by more than 100 corr_tol |corr|, that every transmitted resource's |distance| exceeds 100 distance_tol times the case's rms (and that of a resource
nobody transmitted twice the tolerance, so that its ack_value cannot turn inside it either), that the reference decodes every transmitted CFI and ACK as sent, and that every DCI of the subframe cases decodes with crc_rem == rnti; the model's cfi and ack_value equal
the reference's in every case."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctrl_model as KM  # noqa: E402
import pdcch_map_model as PM  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ctrl_ref.npz")
REF_FILES = ["phch/regs.c", "phch/pcfich.c", "phch/phich.c", "phch/pdcch.c", "phch/dci.c", "phch/sequences.c", "common/sequence.c", "common/phy_common.c",
             "scrambling/scrambling.c", "modem/mod.c", "modem/demod_soft.c", "modem/modem_table.c", "modem/lte_tables.c", "mimo/precoding.c", "mimo/layermap.c",
             "utils/mat.c", "fec/convolutional/viterbi.c", "fec/convolutional/viterbi37_port.c", "fec/convolutional/viterbi37_sse.c",
             "fec/convolutional/viterbi37_avx2.c", "fec/convolutional/parity.c", "fec/convolutional/convcoder.c", "fec/turbo/rm_conv.c", "fec/crc.c",
             "ch_estimation/chest_common.c", "ch_estimation/refsignal_dl.c", "utils/convolution.c", "resampling/interp.c", "sync/pss.c",
             "utils/bit.c", "utils/vector.c", "utils/vector_simd.c", "utils/debug.c", "utils/phy_logger.c"]

D = PM.describe
MAP_CASES = [
    ("6prb_id10", D(6, 1, 10, 1)),  # 4 control symbols; the PCFICH's second REG wraps round the row
    ("15prb_id47", D(15, 2, 47, 2)),  # id above 2 nof_prb: k_hat wraps, and so do two of the REGs
    ("25prb_2p", D(25, 2, 11, 3)),
    ("6prb_ext", D(6, 1, 7, 3, cp_nsymb=6)),  # two groups per mapping unit
    ("15prb_ext_4p", D(15, 4, 77, 1, cp_nsymb=6, phich_resources=3)),
    ("25prb_phich_ext", D(25, 1, 101, 3, phich_length=1)),  # REG i of a unit on symbol i
    ("25prb_phich_ext_mbsfn", D(25, 1, 101, 2, phich_length=1, mbsfn=1)),  # symbols 0 / 1 alternating
    ("15prb_mi0", D(15, 1, 33, 2, phich_mi=0)),  # no PHICH
    ("15prb_mi2", D(15, 1, 33, 2, phich_mi=2)),
    ("25prb_ng16", D(25, 2, 11, 2, phich_resources=0)),
    ("25prb_ng2", D(25, 2, 11, 2, phich_resources=3)),
]
SIGNAL_CASES = [  # name, description, the CFI sent (0: minus the sum of the three code words), noise_estimate
    ("15prb_1p_1rx", D(15, 1, 1, 1, sf_idx=0, nof_rx=1), 1, 0.0),
    ("15prb_1p_2rx_noise", D(15, 1, 2, 2, sf_idx=3, nof_rx=2), 2, 0.05),
    ("25prb_2p_1rx", D(25, 2, 150, 3, sf_idx=5, nof_rx=1), 3, 0.0),
    ("15prb_2p_2rx", D(15, 2, 77, 1, sf_idx=9, nof_rx=2, phich_length=1), 1, 0.0),
    ("25prb_4p_1rx", D(25, 4, 2, 2, sf_idx=1, nof_rx=1, phich_resources=3), 2, 0.0),
    ("15prb_4p_2rx", D(15, 4, 400, 3, sf_idx=7, nof_rx=2), 3, 0.0),
    ("6prb_ext_1p_1rx", D(6, 1, 7, 2, cp_nsymb=6, sf_idx=4, nof_rx=1, phich_resources=3), 2, 0.0),
    ("15prb_1p_nonpos", D(15, 1, 30, 1, sf_idx=2, nof_rx=1), 0, 0.0),
]
EST_CASES = [  # name, description (cfi: what the PCFICH says), cfi3_to_2
    ("6prb_1p_1rx", D(6, 1, 5, 2, sf_idx=1, nof_rx=1, phich_resources=3), 0),
    ("15prb_2p_2rx_tdd", D(15, 2, 21, 3, sf_idx=6, nof_rx=2), 1),
    ("15prb_1p_2rx", D(15, 1, 300, 1, sf_idx=8, nof_rx=2), 0),
]
SIGMA = 0.03  # noise per component, against channels of unit gain


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libctrl_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_CHEST_DL_C="%s"' % os.path.join(phy, "ch_estimation", "chest_dl.c"),
                                             '-DREF_V37_C="%s"' % os.path.join(phy, "fec", "convolutional", "viterbi37_avx2_16bit.c"), "-shared",
                                             os.path.join(ROOT, "tools", "ctrl_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    lib = C.CDLL(so, mode=os.RTLD_LAZY)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    lib.ctrl_ref_open.argtypes = [vp]
    lib.ctrl_ref_close.restype = None
    lib.ctrl_ref_pdcch_nregs.argtypes = [u32]
    lib.ctrl_ref_pcfich_get.argtypes = [vp, vp]
    lib.ctrl_ref_phich_get.argtypes = [vp, vp, u32]
    lib.ctrl_ref_pcfich_encode.argtypes = [u32, u32, vp]
    lib.ctrl_ref_phich_encode.argtypes = [u32, u32, u32, u32, vp]
    lib.ctrl_ref_pdcch_encode.argtypes = [u32, u32, u32, u32, u32, C.c_uint16, vp, vp]
    lib.ctrl_ref_cs_put.argtypes = [u32, u32, vp]
    lib.ctrl_ref_cs_pilots.argtypes = [u32, vp, vp]
    lib.ctrl_ref_cs_pilots.restype = None
    lib.ctrl_ref_pcfich_decode.argtypes = [u32, u32, vp, vp, f32, vp, vp, vp, vp]
    lib.ctrl_ref_phich_decode.argtypes = [u32, u32, vp, vp, f32, u32, u32, vp, vp, vp, vp]
    lib.ctrl_ref_extract.argtypes = [u32, u32, u32, vp, vp, f32, vp]
    lib.ctrl_ref_dci_decode.argtypes = [vp, u32, u32, vp, vp]
    lib.ctrl_ref_chest.argtypes = [u32, u32, vp, vp, vp]
    return lib


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def rms(v):
    return float(np.sqrt(np.mean(np.abs(np.asarray(v, np.float64)) ** 2)))


def ref_tables(lib, sf, ngroups):
    """the indices srsran_regs_pcfich_get / _phich_get read, off a grid that holds its own indices (exact in float32 below 2^24)"""
    n = 4 * 12 * sf["cell_nof_prb"]
    grid = np.arange(n).astype(np.complex64)
    d = np.zeros(16, np.complex64)
    assert lib.ctrl_ref_pcfich_get(grid.ctypes.data, d.ctypes.data) == 16
    pcfich = d.real.astype(np.uint32)
    phich = np.zeros((ngroups, 12), np.uint32)
    for g in range(ngroups):
        d = np.zeros(12, np.complex64)
        assert lib.ctrl_ref_phich_get(grid.ctypes.data, d.ctypes.data, g) == 12
        phich[g] = d.real.astype(np.uint32)
    assert pcfich.max() < 12 * sf["cell_nof_prb"] and (ngroups == 0 or phich.max() < 3 * 12 * sf["cell_nof_prb"])
    return pcfich, phich


def check_tables(name, sf, ngroups, pcfich, phich):
    assert ngroups == KM.phich_ngroups(sf), name
    assert np.array_equal(pcfich, KM.pcfich_table(sf)), name
    for g in range(ngroups):
        assert np.array_equal(phich[g], KM.phich_table(sf, g)), (name, g)


def resources(sf, ngroups):
    """-> [(ngroup, nseq, ack or -1 when nobody transmits it)]"""
    last = ngroups - 1
    if sf["cp_nsymb"] == 6:  # four sequences; groups 2 k and 2 k + 1 share a mapping unit
        r = [(0, 0, 1), (0, 3, 0), (1, 1, 0), (1, 2, 1), (0, 2, -1), (last, 0, -1)]
    else:
        r = [(0, 0, 1), (0, 3, 0), (0, 5, 1), (0, 6, 0), (last, 2, 1), (last, 7, 0), (0, 1, -1), (last, 4, -1)]
    assert ngroups >= 2 and len(set(r)) == len(r)
    return r


def dot32(signs, v):
    acc = np.float32(0)
    for s, x in zip(signs, v):
        acc = np.float32(acc + x) if s else np.float32(acc - x)
    return acc


def channels(rng, ports, nof_rx, n, ripple):
    gain = (rng.standard_normal((ports, nof_rx, 1)) + 1j * rng.standard_normal((ports, nof_rx, 1))) / np.sqrt(2)
    gain = gain / np.abs(gain) * rng.uniform(0.6, 1.4, gain.shape)
    return (gain * (1 + ripple * (rng.standard_normal((ports, nof_rx, n)) + 1j * rng.standard_normal((ports, nof_rx, n))))).astype(np.complex64)


def receive(rng, h, tx):
    ports, nof_rx, n = h.shape
    rx = []
    for a in range(nof_rx):
        y = sum(h[p, a].astype(np.complex128) * tx[p] for p in range(ports))
        rx.append((y + SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
    return np.array(rx)


def ref_pcfich(lib, sf, rxs, ce, noise):
    cfi, corr, data_f, d = np.zeros(1, np.uint32), np.zeros(1, np.float32), np.zeros(32, np.float32), np.zeros(16, np.complex64)
    assert lib.ctrl_ref_pcfich_decode(sf["sf_idx"], sf["nof_rx"], ptrs(rxs), ptrs(ce), C.c_float(noise), cfi.ctypes.data, corr.ctypes.data, data_f.ctypes.data,
                                      d.ctypes.data) == 1
    return int(cfi[0]), corr[0], data_f, d


def ref_phich(lib, sf, rxs, ce, noise, res):
    n = len(res)
    ack, dist, bits, z = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.complex64)
    for i, (g, s, _) in enumerate(res):
        a, dd = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        assert lib.ctrl_ref_phich_decode(sf["sf_idx"], sf["nof_rx"], ptrs(rxs), ptrs(ce), C.c_float(noise), g, s, a.ctypes.data, dd.ctypes.data, bits[i].ctypes.data,
                                         z[i].ctypes.data) == 0
        ack[i], dist[i] = a[0], dd[0]
    return ack, dist, bits, z


def signal_case(lib, rng, name, sf, cfi_sent, noise_estimate):
    ngroups = lib.ctrl_ref_open(PM.as_row(sf).ctypes.data)
    assert ngroups >= 0, (name, ngroups)
    try:
        pcfich_t, phich_t = ref_tables(lib, sf, ngroups)
        check_tables(name, sf, ngroups, pcfich_t, phich_t)
        ports, nof_rx, nof_prb = sf["cell_nof_ports"], sf["nof_rx"], sf["cell_nof_prb"]
        full, npts = 4 * 12 * nof_prb, 3 * 12 * nof_prb
        tx = [np.zeros(full, np.complex64) for _ in range(ports)]
        if cfi_sent:
            assert lib.ctrl_ref_pcfich_encode(cfi_sent, sf["sf_idx"], ptrs(tx)) == 0
        else:  # minus the sum of the three code words: every soft bit comes out negative, every correlation too
            for c in (1, 2, 3):
                one = [np.zeros(full, np.complex64) for _ in range(ports)]
                assert lib.ctrl_ref_pcfich_encode(c, sf["sf_idx"], ptrs(one)) == 0
                for p in range(ports):
                    tx[p] -= one[p]
        res = resources(sf, ngroups)
        for g, s, ack in res:
            if ack >= 0:
                assert lib.ctrl_ref_phich_encode(sf["sf_idx"], g, s, ack, ptrs(tx)) == 0, (name, g, s)
        h = channels(rng, ports, nof_rx, full, 0.05)
        rx = receive(rng, h, tx)
        ce = [np.ascontiguousarray(h[p, a]) for p in range(ports) for a in range(nof_rx)]
        rxs = [np.ascontiguousarray(g) for g in rx]
        cfi, corr, data_f, d = ref_pcfich(lib, sf, rxs, ce, noise_estimate)
        ack, dist, bits, z = ref_phich(lib, sf, rxs, ce, noise_estimate, res)
        # the reference alone
        corr3 = np.array([dot32(KM.CFI_TABLE[k], data_f) for k in range(3)], np.float32)
        if cfi_sent:
            assert cfi == cfi_sent and corr == corr3.max() and corr > 0, (name, cfi, corr, corr3)
        else:
            assert cfi == 1 and corr == 0 and np.all(corr3 < 0), (name, cfi, corr, corr3)
        for i, (_, _, sent) in enumerate(res):
            assert sent < 0 or ack[i] == sent, (name, i)
        # the model
        m = KM.pcfich_decode(sf, rx, h, noise_estimate, pcfich_t)
        assert m["cfi"] == cfi, name
        mp = [KM.phich_decode(sf, rx, h, noise_estimate, g, s, phich_t[g]) for g, s, _ in res]
        assert [x["ack_value"] for x in mp] == list(ack), name
        dev = dict(data_f=float(np.abs(m["data_f"].astype(np.float64) - data_f).max()) / rms(data_f),
                   corr=abs(float(m["corr"]) - float(corr)) / abs(float(corr)) if corr != 0 else float(m["corr"] != 0),
                   bits=float(np.abs(np.array([x["bits"] for x in mp], np.float64) - bits).max()) / rms(bits),
                   distance=float(np.abs(np.array([x["distance"] for x in mp], np.float64) - dist).max()) / rms(dist))
        print("S %-20s cfi %d corr %8.4f  %d resources, %d groups  deviation of the model: %s" %
              (name, cfi, corr, len(res), ngroups, "  ".join("%s %.3g" % kv for kv in dev.items())))
        rec = dict(sf=PM.as_row(sf), pcfich_table=pcfich_t, phich_table=phich_t, rx=rx[:, :npts].copy(), ce=h[:, :, :npts].copy(), noise=np.float32(noise_estimate),
                   cfi_sent=np.uint32(cfi_sent), cfi=np.uint32(cfi), corr=np.float32(corr), corr3=corr3, data_f=data_f, d=d,
                   res=np.array([(g, s) for g, s, _ in res], np.uint32), sent=np.array([a for _, _, a in res], np.int32), ack=ack, distance=dist, bits=bits, z=z)
        return rec, dev
    finally:
        lib.ctrl_ref_close()


def est_layout(nof_cce):
    """the DCIs of a subframe case: (ncce, L, nof_bits)"""
    if nof_cce >= 7:
        return [(0, 2, 57), (4, 1, 43), (6, 0, 31)]
    return [(0, 1, 43), (2, 0, 31)] if nof_cce >= 3 else [(0, 0, 31), (1, 0, 27)]


def est_case(lib, rng, name, sf, cfi3_to_2):
    ngroups = lib.ctrl_ref_open(PM.as_row(sf).ctypes.data)
    assert ngroups >= 2, (name, ngroups)
    try:
        ports, nof_rx, nof_prb, sf_idx = sf["cell_nof_ports"], sf["nof_rx"], sf["cell_nof_prb"], sf["sf_idx"]
        full = 2 * sf["cp_nsymb"] * 12 * nof_prb
        cfi_pdcch = 2 if (cfi3_to_2 and sf["cfi"] == 3) else sf["cfi"]
        nof_cce = [lib.ctrl_ref_pdcch_nregs(c) // 9 for c in (1, 2, 3)]
        tx = [np.zeros(full, np.complex64) for _ in range(ports)]
        for p in range(ports):
            assert lib.ctrl_ref_cs_put(sf_idx, p, tx[p].ctypes.data) == 0
        assert lib.ctrl_ref_pcfich_encode(sf["cfi"], sf_idx, ptrs(tx)) == 0
        res = resources(sf, ngroups)
        for g, s, ack in res:
            if ack >= 0:
                assert lib.ctrl_ref_phich_encode(sf_idx, g, s, ack, ptrs(tx)) == 0
        dcis, sent = est_layout(nof_cce[cfi_pdcch - 1]), []
        for ncce, L, nof_bits in dcis:
            payload, rnti = rng.integers(0, 2, nof_bits).astype(np.uint8), int(rng.integers(1, 0xFFF0))
            buf = np.zeros(128, np.uint8)
            buf[:nof_bits] = payload
            assert lib.ctrl_ref_pdcch_encode(cfi_pdcch, sf_idx, ncce, L, nof_bits, rnti, buf.ctypes.data, ptrs(tx)) == 0, (name, ncce, L)
            sent.append((payload, rnti))
        h = channels(rng, ports, nof_rx, full, 0.0)  # flat: what an interpolating estimator follows
        rx = receive(rng, h, tx)
        rxs = [np.ascontiguousarray(g) for g in rx]
        pilots0, pilots1 = np.zeros(8 * nof_prb, np.complex64), np.zeros(4 * nof_prb, np.complex64)
        lib.ctrl_ref_cs_pilots(sf_idx, pilots0.ctypes.data, pilots1.ctypes.data)
        # the reference's chain (ue_dl.c:315-343)
        ce = [np.zeros(full, np.complex64) for _ in range(ports * nof_rx)]
        noise = np.zeros(1, np.float32)
        assert lib.ctrl_ref_chest(sf_idx, nof_rx, ptrs(rxs), ptrs(ce), noise.ctypes.data) == 0
        err = max(float(np.abs(ce[p * nof_rx + a] - h[p, a]).max()) for p in range(ports) for a in range(nof_rx))
        cfi, corr, _, _ = ref_pcfich(lib, sf, rxs, ce, float(noise[0]))
        assert cfi == sf["cfi"], (name, cfi)
        if cfi3_to_2 and cfi == 3:
            cfi = 2
        assert cfi == cfi_pdcch
        llr = np.zeros(72 * nof_cce[cfi - 1], np.float32)
        assert lib.ctrl_ref_extract(cfi, sf_idx, nof_rx, ptrs(rxs), ptrs(ce), C.c_float(noise[0]), llr.ctypes.data) == 0
        bits, crc = np.zeros((len(dcis), 144), np.uint8), np.zeros(len(dcis), np.uint16)
        for i, (ncce, L, nof_bits) in enumerate(dcis):
            e, b, r = np.ascontiguousarray(llr[72 * ncce:72 * ncce + (72 << L)]), np.zeros(nof_bits + 16, np.uint8), np.zeros(1, np.uint16)
            assert lib.ctrl_ref_dci_decode(e.ctypes.data, 72 << L, nof_bits, b.ctypes.data, r.ctypes.data) == 0
            assert r[0] == sent[i][1] and np.array_equal(b[:nof_bits], sent[i][0]), (name, i, "crc_rem != rnti")
            bits[i, :nof_bits + 16], crc[i] = b, r[0]
        ack, dist, _, _ = ref_phich(lib, sf, rxs, ce, float(noise[0]), res)
        for i, (_, _, a) in enumerate(res):
            assert a < 0 or ack[i] == a, (name, i)
        print("E %-20s cfi %d -> %d  nof_cce %s  %d DCIs  %d resources  noise_estimate %.3g  worst |ce - h| %.3g" %
              (name, sf["cfi"], cfi, nof_cce, len(dcis), len(res), noise[0], err))
        return dict(sf=PM.as_row(sf), cfi3_to_2=np.uint32(cfi3_to_2), rx=rx, pilots0=pilots0, pilots1=pilots1, cfi=np.uint32(cfi), corr=np.float32(corr),
                    noise=noise[0], nof_cce=np.array(nof_cce, np.uint32), cand=np.array(dcis, np.uint32), bits=bits, crc=crc,
                    res=np.array([(g, s) for g, s, _ in res], np.uint32), sent=np.array([a for _, _, a in res], np.int32), ack=ack, distance=dist)
    finally:
        lib.ctrl_ref_close()


def main():
    rng = np.random.default_rng(2507)
    d = {"m_names": np.array([n for n, _ in MAP_CASES]), "s_names": np.array([c[0] for c in SIGNAL_CASES]), "e_names": np.array([c[0] for c in EST_CASES]),
         "m_sf": np.array([PM.as_row(sf) for _, sf in MAP_CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_wrapper(tmp)
        for i, (name, sf) in enumerate(MAP_CASES):
            ngroups = lib.ctrl_ref_open(PM.as_row(sf).ctypes.data)
            assert ngroups >= 0, (name, ngroups)
            try:
                pcfich_t, phich_t = ref_tables(lib, sf, ngroups)
            finally:
                lib.ctrl_ref_close()
            check_tables(name, sf, ngroups, pcfich_t, phich_t)
            d["m_pcfich_%d" % i], d["m_phich_%d" % i] = pcfich_t, phich_t
            print("M %-22s PCFICH at %s  %2d PHICH groups on symbols %s" % (name, pcfich_t[::4], ngroups, sorted(set((phich_t // (12 * sf["cell_nof_prb"])).ravel()))))
        worst, recs = {}, []
        for name, sf, cfi_sent, noise in SIGNAL_CASES:
            rec, dev = signal_case(lib, rng, name, sf, cfi_sent, noise)
            recs.append(rec)
            for k, v in dev.items():
                worst[k] = max(worst.get(k, 0.0), v)
        tol = {k: 4 * v for k, v in worst.items()}
        for (name, _, cfi_sent, _), rec in zip(SIGNAL_CASES, recs):  # the conditions under which the tolerances hide no wrong decision: the reference alone
            if cfi_sent:
                best, second = np.sort(rec["corr3"].astype(np.float64))[::-1][:2]
                assert best - second > 100 * tol["corr"] * abs(best), (name, best, second)
            lead = np.abs(rec["distance"]) / (tol["distance"] * rms(rec["distance"]))
            assert np.all(lead[rec["sent"] >= 0] > 100) and np.all(lead > 2), (name, rec["distance"])
        for i, rec in enumerate(recs):
            for k, v in rec.items():
                d["s_%s_%d" % (k, i)] = v
        for k, v in tol.items():
            d["%s_tol" % k] = np.float64(v)
        print("worst deviations of the model from the reference: %s -> tolerances %s" % (worst, tol))
        for i, (name, sf, rule) in enumerate(EST_CASES):
            for k, v in est_case(lib, rng, name, sf, rule).items():
                d["e_%s_%d" % (k, i)] = v
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(MAP_CASES), "map cases,", len(SIGNAL_CASES), "signal cases,", len(EST_CASES), "subframe cases")


if __name__ == "__main__":
    main()
