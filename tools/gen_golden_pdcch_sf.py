#!/usr/bin/env python3
"""Record what the reference's REG map (srsran_regs_init_opts, srsran_regs_pdcch_get: phch/regs.c) and its PDCCH receiver (srsran_pdcch_extract_llr,
srsran_pdcch_dci_decode: phch/pdcch.c) give on seeded control regions that its own transmitter (srsran_pdcch_encode) filled: tests/golden/pdcch_sf_ref.npz.

    python tools/gen_golden_pdcch_sf.py          (needs the reference tree)

tools/pdcch_sf_ref_wrap.c and the reference files it binds into are compiled where they lie, with the REF_FLAGS of oracle/Makefile, into a temporary directory
(nothing compiled is kept); loaded lazily.  The record holds data only.

Map cases (m_*): a description and its index table -- 4 nregs grid indices, read off srsran_regs_pdcch_get on a grid that holds its own indices.  The model's
table (tests/pdcch_map_model.py) must equal it EXACTLY, which is asserted here.
Signal cases (s_*): ports 1, 2 and 4 with 1 and 2 receive antennas, a one-port region with noise_estimate > 0, an extended-prefix 6-PRB region, and a one-port region
with unit estimates in which one two-CCE candidate's REs span 40 binary orders (so that the double sum of the mean rule rounds and its order shows).  Every
region carries three or four DCIs of different lengths and levels put in by srsran_pdcch_encode, goes through per-(port, antenna) channels (a random complex
gain with a 5 % ripple per RE) and noise, has one CCE whose received REs are all zero and one that holds noise alone at signal level; the candidates are the
DCIs' own, the same locations with another length, an overlapping pair, the zero CCE, the noise CCE, an empty CCE and -- where the region has eight CCEs -- an
L = 3 candidate that ends at the last CCE.  Recorded per region: the description, the table, the control rows of the grids and estimates, the reference's
soft bits and equalised symbols, and per candidate the reference's payload, CRC remainder and mean.

The float tolerance is MEASURED here: the deviation of the model's soft bits from the reference's, max |a - b| / rms(b) per region; four times the worst value
is stored as llr_tol (the device may fuse a multiply-add where numpy rounds twice: about one more ulp per operation of a handful).  So that the comparison
hides nothing it is asserted that every DCI-carrying candidate decodes to the recorded payload from the MODEL's soft bits through conv_model, that the
reference decodes each with crc_rem == rnti, and that every signal case has at least three of them."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_model as CM  # noqa: E402
import pdcch_map_model as PM  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pdcch_sf_ref.npz")
REF_FILES = ["phch/regs.c", "phch/pdcch.c", "phch/dci.c", "phch/sequences.c", "common/sequence.c", "common/phy_common.c", "scrambling/scrambling.c", "modem/mod.c",
             "modem/demod_soft.c", "modem/modem_table.c", "modem/lte_tables.c", "mimo/precoding.c", "mimo/layermap.c", "utils/mat.c",
             "fec/convolutional/viterbi.c", "fec/convolutional/viterbi37_port.c", "fec/convolutional/viterbi37_sse.c", "fec/convolutional/viterbi37_avx2.c",
             "fec/convolutional/parity.c", "fec/convolutional/convcoder.c", "fec/turbo/rm_conv.c", "fec/crc.c",
             "utils/bit.c", "utils/vector.c", "utils/vector_simd.c", "utils/debug.c", "utils/phy_logger.c"]

D = PM.describe
MAP_CASES = [
    ("6prb_1p_cfi1", D(6, 1, 0, 1)),  # nof_prb <= 10: cfi + 1 symbols; 23 free REGs, 18 after the cut
    ("6prb_1p_cfi3", D(6, 1, 0, 3)),  # 4 control symbols
    ("15prb_2p_cfi1", D(15, 2, 1, 1)),
    ("25prb_4p_cfi3", D(25, 4, 2, 3)),  # symbol 1 has 2 REGs per PRB
    ("6prb_ext_cfi3", D(6, 1, 7, 3, cp_nsymb=6)),  # symbol 3 has 2 REGs per PRB
    ("6prb_id503_cfi1", D(6, 1, 503, 1)),  # an id above the region's REG count: the k < cell.id branch all the way
    ("15prb_id150_cfi2", D(15, 2, 150, 2)),  # both forms of the shift in one table
    ("25prb_ng16", D(25, 2, 11, 2, phich_resources=0)),
    ("25prb_ng2", D(25, 2, 11, 2, phich_resources=3)),
    ("25prb_phich_ext", D(25, 1, 101, 3, phich_length=1)),
    ("25prb_phich_ext_mbsfn", D(25, 1, 101, 2, phich_length=1, mbsfn=1)),
    ("15prb_mi0", D(15, 1, 33, 2, phich_mi=0)),
    ("15prb_mi2", D(15, 1, 33, 2, phich_mi=2)),
    ("50prb_mi2_ng2", D(50, 4, 301, 3, phich_resources=3, phich_mi=2)),
    ("100prb_2p_cfi3", D(100, 2, 257, 3)),
]
SIGNAL_CASES = [  # name, description, noise_estimate, kind
    ("15prb_1p_1rx", D(15, 1, 1, 3, sf_idx=0, nof_rx=1), 0.0, ""),
    ("15prb_1p_2rx_noise", D(15, 1, 2, 3, sf_idx=3, nof_rx=2), 0.05, ""),
    ("25prb_2p_1rx", D(25, 2, 150, 2, sf_idx=5, nof_rx=1), 0.0, ""),
    ("15prb_2p_2rx", D(15, 2, 77, 3, sf_idx=9, nof_rx=2, phich_length=1), 0.0, ""),
    ("25prb_4p_1rx", D(25, 4, 2, 3, sf_idx=1, nof_rx=1), 0.0, ""),
    ("15prb_4p_2rx", D(15, 4, 400, 3, sf_idx=7, nof_rx=2, phich_resources=0), 0.0, ""),
    ("6prb_ext_1p_1rx", D(6, 1, 7, 3, cp_nsymb=6, sf_idx=4, nof_rx=1, phich_mi=0), 0.0, ""),
    ("15prb_1p_wide", D(15, 1, 30, 3, sf_idx=2, nof_rx=1), 0.0, "wide"),
]
SIGMA = 0.03  # noise per component, against channels of unit gain


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libpdcch_sf_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_V37_C="%s"' % os.path.join(phy, "fec", "convolutional", "viterbi37_avx2_16bit.c"), "-shared",
                           os.path.join(ROOT, "tools", "pdcch_sf_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] +
                          ["-o", so, "-lm"])
    lib = C.CDLL(so, mode=os.RTLD_LAZY)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.pdcch_sf_ref_open.argtypes = [vp]
    lib.pdcch_sf_ref_get.argtypes = [u32, vp, vp]
    lib.pdcch_sf_ref_encode.argtypes = [u32, u32, u32, u32, u32, C.c_uint16, vp, vp]
    lib.pdcch_sf_ref_extract.argtypes = [u32, u32, u32, vp, vp, C.c_float, vp, vp]
    lib.pdcch_sf_ref_decode.argtypes = [vp, u32, u32, vp, vp]
    lib.pdcch_sf_ref_close.restype = None
    return lib


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def ref_open(lib, sf):
    row = PM.as_row(sf)
    nregs = lib.pdcch_sf_ref_open(row.ctypes.data)
    assert nregs > 0 and nregs % 9 == 0, (sf, nregs)
    return nregs


def ref_table(lib, sf, nregs):
    """the indices srsran_regs_pdcch_get reads, off a grid that holds its own indices (exact in float32 below 2^24)"""
    n = 4 * 12 * sf["cell_nof_prb"]
    grid = np.arange(n).astype(np.complex64)
    d = np.zeros(4 * nregs, np.complex64)
    assert lib.pdcch_sf_ref_get(sf["cfi"], grid.ctypes.data, d.ctypes.data) == 4 * nregs
    t = d.real.astype(np.uint32)
    assert np.all(d.imag == 0) and t.max() < PM.nof_ctrl_symbols(sf) * 12 * sf["cell_nof_prb"]
    return t


def layout(nof_cce):
    """where the DCIs, the zero CCE and the noise CCE go: -> dcis [(ncce, L, nof_bits)], zero, noise, empty"""
    if nof_cce >= 12:
        locs = [(0, 2, 57), (4, 1, 43), (6, 0, 31), (7, 0, 27)]
    elif nof_cce >= 9:
        locs = [(0, 1, 57), (2, 1, 43), (4, 0, 31), (5, 0, 27)]
    else:
        locs = [(0, 1, 43), (2, 0, 31), (3, 0, 27)]
    end = locs[-1][0] + 1
    assert end + 2 <= nof_cce
    return locs, end, end + 1, (end + 2 if end + 2 < nof_cce else None)


def signal_case(lib, rng, name, sf, noise_estimate, kind):
    nregs = ref_open(lib, sf)
    try:
        table = ref_table(lib, sf, nregs)
        assert np.array_equal(table, PM.reg_table(sf)), name
        nof_cce, ports, nof_rx, nof_prb = nregs // 9, sf["cell_nof_ports"], sf["nof_rx"], sf["cell_nof_prb"]
        rows, full = PM.nof_ctrl_symbols(sf), 4 * 12 * nof_prb
        npts = rows * 12 * nof_prb
        dcis, zero_cce, noise_cce, empty_cce = layout(nof_cce)
        wide_cce = None
        if kind == "wide":  # the two CCEs behind the noise CCE
            wide_cce = noise_cce + 1
            empty_cce = wide_cce + 2 if wide_cce + 2 < nof_cce else None
            assert wide_cce + 2 <= nof_cce
        tx = [np.zeros(full, np.complex64) for _ in range(ports)]
        sent = []
        for ncce, L, nof_bits in dcis:
            payload, rnti = rng.integers(0, 2, nof_bits).astype(np.uint8), int(rng.integers(1, 0xFFF0))
            buf = np.zeros(128, np.uint8)
            buf[:nof_bits] = payload
            assert lib.pdcch_sf_ref_encode(sf["cfi"], sf["sf_idx"], ncce, L, nof_bits, rnti, buf.ctypes.data, ptrs(tx)) == 0, (name, ncce, L)
            sent.append((payload, rnti))
        if kind == "wide":
            h = np.ones((ports, nof_rx, full), np.complex64)
        else:
            gain = (rng.standard_normal((ports, nof_rx, 1)) + 1j * rng.standard_normal((ports, nof_rx, 1))) / np.sqrt(2)
            gain = gain / np.abs(gain) * rng.uniform(0.6, 1.4, gain.shape)
            h = (gain * (1 + 0.05 * (rng.standard_normal((ports, nof_rx, full)) + 1j * rng.standard_normal((ports, nof_rx, full))))).astype(np.complex64)
        rx = []
        for a in range(nof_rx):
            y = sum(h[p, a].astype(np.complex128) * tx[p] for p in range(ports))
            y = y + SIGMA * (rng.standard_normal(full) + 1j * rng.standard_normal(full))
            y[table[36 * noise_cce:36 * noise_cce + 36]] = 0.7 * (rng.standard_normal(36) + 1j * rng.standard_normal(36))
            y[table[36 * zero_cce:36 * zero_cce + 36]] = 0
            if wide_cce is not None:  # magnitudes 2^-20 .. 2^20 with full random mantissas, random signs
                mag = lambda: np.exp2(rng.uniform(-20, 20, 72)) * rng.choice([-1.0, 1.0], 72)  # noqa: E731
                y[table[36 * wide_cce:36 * wide_cce + 72]] = mag() + 1j * mag()
            rx.append(y.astype(np.complex64))
        rx = np.array(rx)
        ce = [np.ascontiguousarray(h[p, a]) for p in range(ports) for a in range(nof_rx)]
        rxs = [np.ascontiguousarray(g) for g in rx]
        ref_llr, ref_d = np.zeros(72 * nof_cce, np.float32), np.zeros(36 * nof_cce, np.complex64)
        assert lib.pdcch_sf_ref_extract(sf["cfi"], sf["sf_idx"], nof_rx, ptrs(rxs), ptrs(ce), C.c_float(noise_estimate), ref_llr.ctypes.data,
                                        ref_d.ctypes.data) == 0, name
        m = PM.extract_llr(sf, rx, h, noise_estimate, table)
        dev = float(np.abs(m["llr"].astype(np.float64) - ref_llr).max() / np.sqrt(np.mean(ref_llr.astype(np.float64) ** 2)))
        # the candidates
        cands, carries = [], []
        for ncce, L, nof_bits in dcis:
            cands.append((ncce, L, nof_bits))
            carries.append(len(carries))
        n_dci = len(cands)
        cands.append((dcis[0][0], dcis[0][1], dcis[0][2] + 4))  # the same location, another length
        cands.append((dcis[1][0], dcis[1][1], 25))
        cands.append((0, max(dcis[0][1] - 1, 0), dcis[0][2]))  # inside the first DCI: overlaps its candidate
        cands.append((0, dcis[0][1] + 1, 41))  # over the first DCIs: overlaps again
        cands.append((zero_cce, 0, 27))
        cands.append((noise_cce, 0, 43))
        if empty_cce is not None:
            cands.append((empty_cce, 0, 27))
        if wide_cce is not None:
            cands.append((wide_cce, 1, 27))
        if nof_cce >= 8:
            cands.append((nof_cce - 8, 3, 57))  # ends at the last CCE
        cands = np.array(cands, np.uint32)
        n = len(cands)
        ref_bits, ref_crc, ref_mean, ref_dec = np.zeros((n, 144), np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.float64), np.zeros(n, np.uint8)
        for i, (ncce, L, nof_bits) in enumerate(cands):
            ncce, L, nof_bits = int(ncce), int(L), int(nof_bits)
            assert 72 * ncce + (72 << L) <= 72 * nof_cce, (name, ncce, L)
            ref_mean[i] = CM.pdcch_mean(ref_llr, ncce, L)  # the rule of srsran_pdcch_decode_msg on the reference's soft bits
            if ref_mean[i] > 0.3:
                e = np.ascontiguousarray(ref_llr[72 * ncce:72 * ncce + (72 << L)])
                bits, crc = np.zeros(nof_bits + 16, np.uint8), np.zeros(1, np.uint16)
                assert lib.pdcch_sf_ref_decode(e.ctypes.data, 72 << L, nof_bits, bits.ctypes.data, crc.ctypes.data) == 0
                ref_bits[i, :nof_bits + 16], ref_crc[i], ref_dec[i] = bits, crc[0], 1
        carry = np.zeros(n, np.uint8)
        for i in range(n_dci):
            payload, rnti = sent[i]
            nof_bits = int(cands[i][2])
            assert ref_dec[i] and ref_crc[i] == rnti and np.array_equal(ref_bits[i, :nof_bits], payload), (name, i)
            mm = CM.dci_decode(m["llr"][72 * int(cands[i][0]):72 * int(cands[i][0]) + (72 << int(cands[i][1]))], nof_bits)
            assert mm["crc_rem"] == rnti and np.array_equal(mm["bits"], ref_bits[i, :nof_bits + 16]), (name, i, "the model's soft bits")
            carry[i] = 1
        assert carry.sum() >= 3, name
        zi = n_dci + 4
        assert ref_mean[zi] == 0 and not ref_dec[zi] and ref_dec[zi + 1], name
        if wide_cce is not None:
            w = np.abs(ref_llr[72 * wide_cce:72 * wide_cce + 144])
            fwd, bwd = CM.pdcch_mean(ref_llr, wide_cce, 1), float(sum(float(v) for v in w[::-1])) / 144
            assert np.log2(w.max() / w.min()) > 38 and fwd != bwd, (name, "the order of the mean's sum does not show")
        print("S %-22s nof_cce %2d  candidates %2d (%d carry a DCI, %d decoded)  deviation of the model %.3g" % (name, nof_cce, n, carry.sum(), ref_dec.sum(), dev))
        rec = dict(sf=PM.as_row(sf), table=table, rx=rx[:, :npts].copy(), ce=h[:, :, :npts].copy(), noise=np.float32(noise_estimate), llr=ref_llr, d=ref_d,
                   cand=cands, carry=carry, bits=ref_bits, crc=ref_crc, mean=ref_mean, dec=ref_dec)
        return rec, dev
    finally:
        lib.pdcch_sf_ref_close()


def main():
    rng = np.random.default_rng(2406)
    d = {"m_names": np.array([n for n, _ in MAP_CASES]), "s_names": np.array([c[0] for c in SIGNAL_CASES]), "m_sf": np.array([PM.as_row(sf) for _, sf in MAP_CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_wrapper(tmp)
        for i, (name, sf) in enumerate(MAP_CASES):
            nregs = ref_open(lib, sf)
            try:
                t = ref_table(lib, sf, nregs)
            finally:
                lib.pdcch_sf_ref_close()
            assert np.array_equal(t, PM.reg_table(sf)), name
            d["m_table_%d" % i] = t
            print("M %-22s nregs %3d (%2d CCEs)" % (name, nregs, nregs // 9))
        assert d["m_table_0"].size == 4 * 18
        worst = 0.0
        for i, (name, sf, noise, kind) in enumerate(SIGNAL_CASES):
            rec, dev = signal_case(lib, rng, name, sf, noise, kind)
            worst = max(worst, dev)
            for k, v in rec.items():
                d["s_%s_%d" % (k, i)] = v
    d["llr_tol"] = np.float64(4 * worst)
    print("worst deviation of the model's soft bits from the reference's: %.4g of the region's rms -> llr_tol %.4g" % (worst, 4 * worst))
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(MAP_CASES), "map cases,", len(SIGNAL_CASES), "signal cases")


if __name__ == "__main__":
    main()
