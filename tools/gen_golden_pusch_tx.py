#!/usr/bin/env python3
"""Record what the reference's srsran_ulsch_encode (lib/src/phy/phch/sch.c:1194-1337) gives on seeded grants with control information:
tests/golden/pusch_tx_ref.npz.

    python tools/gen_golden_pusch_tx.py          (needs the reference tree and oracle/_ref/libsrsran_ref.so, built by `make -C oracle ref`)

tools/pusch_tx_ref_wrap.c includes the reference's sch.c where it lies and exports one wrapper; it is compiled together with the reference's FFT-free sources
the call needs and libsrsran_ref.so lacks (uci.c, cqi.c, the block and convolutional coders, rm_conv.c, softbuffer.c), where they lie, with the REF_FLAGS of
oracle/Makefile, into a temporary directory (nothing compiled is kept), and loaded lazily behind libsrsran_ref.so, which is loaded globally.  The sources that
include the umbrella header get its list of headers force-included, as tests/ref_link/Makefile does.

The record stops at the bits.  The rest of srsran_pusch_encode (pusch.c:259-354) cannot be built here: pusch.c needs the transform precoder, which needs
FFTW, which this image lacks.  What is recorded per grant: the packed q_bits srsran_ulsch_encode leaves, srsran_sequence_pusch_apply_pack of them (the
scrambled bits BEFORE the fix-up of pusch.c:315-331), the ack_ri_bits list (positions and types, RI first), the three Q' counts, the coded CQI bits (packed)
and the payload.  tests/test_pusch_tx_golden.py holds tests/pusch_tx_model.py to it, tests/test_gpu_pusch_tx.py the library.

Cases: a 1-bit ACK, a 2-bit ACK, a 4-bit ACK (block code), a 1-bit RI, a 4-bit CQI (block code), a 14-bit CQI (CRC + convolutional code), everything together on
two code blocks, a TDD-bundled ACK (N_bundle = 2) and a retransmission (rv 2); normal and extended cyclic prefix, with and without the SRS symbol; 1, 2, 3 and
12 PRB."""
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
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pusch_tx_ref.npz")
QM = {1: 2, 2: 4, 3: 6}
RNTI, TTI, CELL_ID = 0x46, 7, 211
EXTRA_SRC = ["phch/uci.c", "phch/cqi.c", "fec/block/block.c", "fec/convolutional/convcoder.c", "fec/convolutional/viterbi.c", "fec/convolutional/viterbi37_port.c",
             "fec/convolutional/viterbi37_sse.c", "fec/convolutional/viterbi37_avx2.c", "fec/convolutional/viterbi37_avx2_16bit.c", "fec/convolutional/parity.c",
             "fec/turbo/rm_conv.c", "fec/softbuffer.c"]

# name, mod, tbs, rv, L_prb, nof_symb, ACK bits, N_bundle, ri_len, ri, cqi_kind, (I_offset_ack, I_offset_ri, I_offset_cqi)
CASES = [
    ("ack1_qpsk_L1", 1, 40, 0, 1, 12, [1], 0, 0, 0, 0, (4, 3, 6)),
    ("ack2_16qam_L1", 2, 40, 0, 1, 12, [1, 0], 0, 0, 0, 0, (4, 3, 6)),
    ("ack4_64qam_L2_srs", 3, 40, 0, 2, 11, [1, 0, 1, 1], 0, 0, 0, 0, (2, 3, 6)),
    ("ri1_16qam_L1_ext", 2, 40, 0, 1, 10, [], 0, 1, 1, 0, (4, 5, 6)),
    ("cqi4_qpsk_L1", 1, 40, 0, 1, 12, [], 0, 0, 0, 1, (4, 3, 4)),
    ("cqi14_16qam_L3_ext_srs", 2, 40, 0, 3, 9, [], 0, 0, 0, 2, (4, 3, 6)),
    ("ack2_ri1_cqi14_64qam_L12_tbs6200", 3, 6200, 0, 12, 12, [0, 1], 0, 1, 0, 2, (9, 6, 6)),
    ("ack1_bundle2_16qam_L1", 2, 40, 0, 1, 12, [1], 2, 0, 0, 0, (6, 3, 6)),
    ("ack1_ri1_cqi4_qpsk_L2_rv2", 1, 40, 2, 2, 12, [0], 0, 1, 1, 1, (4, 3, 6)),
]


def umbrella_flags(rlib):
    """-include for every header the umbrella srsran/srsran.h lists (it is skipped itself: it wants a cmake-generated header)"""
    text = open(os.path.join(rlib, "include", "srsran", "srsran.h")).read()
    out = ["-include", "complex.h", "-include", "math.h", "-include", "srsran/config.h"]
    for h in re.findall(r'^#include "(srsran/phy/[^"]*)"', text, re.M):
        out += ["-include", h]
    return out


def main():
    rlib, flags = ref_flags()
    C.CDLL(O.REF_LIB, mode=os.RTLD_GLOBAL | os.RTLD_NOW)
    phy = os.path.join(rlib, "src", "phy")
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for src in EXTRA_SRC:
            path = os.path.join(phy, src)
            obj = os.path.join(tmp, src.replace("/", "_") + ".o")
            umb = umbrella_flags(rlib) if "srsran/srsran.h" in open(path).read() else []
            subprocess.check_call(["gcc"] + flags + umb + ["-c", path, "-o", obj])
            objs.append(obj)
        so = os.path.join(tmp, "libpusch_tx_ref_wrap.so")
        subprocess.check_call(["gcc"] + flags + umbrella_flags(rlib) + ['-DREF_SCH_C="%s"' % os.path.join(phy, "phch", "sch.c"), "-shared",
                               os.path.join(ROOT, "tools", "pusch_tx_ref_wrap.c")] + objs + ["-o", so, "-lm"])
        wrap = C.CDLL(so, mode=os.RTLD_LAZY)
        fn = wrap.pusch_tx_ref
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        fn.argtypes = [i, i, i, u, u, u, vp, u, u, u, i, u, u, u, u, u, u, u, vp, vp, vp, vp, vp, vp, vp]
        fn.restype = C.c_int
        rng = np.random.default_rng(36212)
        d = {"names": np.array([c[0] for c in CASES]), "seeds": np.full(len(CASES), O.pusch_seed(RNTI, 2 * (TTI % 10), CELL_ID), np.uint32)}
        rows = []
        for k, (name, mod, tbs, rv, L_prb, nof_symb, ack, N_bundle, ri_len, ri, cqi_kind, (I_ack, I_ri, I_cqi)) in enumerate(CASES):
            Qm = QM[mod]
            H = nof_symb * 12 * L_prb
            pay = rng.integers(0, 256, tbs // 8 + 8).astype(np.uint8)
            ackv = np.array(ack + [0], np.uint8)
            q, scr = np.zeros(H * Qm // 8 + 64, np.uint8), np.zeros(H * Qm // 8 + 64, np.uint8)
            pos, typ, counts, cqi = np.zeros(57600, np.uint32), np.zeros(57600, np.uint8), np.zeros(3, np.uint32), np.zeros(H * Qm + 64, np.uint8)
            n = fn(mod, tbs, rv, L_prb, nof_symb, len(ack), O.P(ackv), N_bundle, ri_len, ri, cqi_kind, int(rng.integers(1 << 14)), I_ack, I_ri, I_cqi, RNTI, TTI, CELL_ID,
                   O.P(pay), O.P(q), O.P(scr), O.P(pos), O.P(typ), O.P(counts), O.P(cqi))
            assert n >= 0, (name, n)
            Qa, Qr, Qc = (int(x) for x in counts)
            assert n == (Qa + Qr) * Qm and not q[H * Qm // 8:].any(), name
            assert (Qa > 0) == (len(ack) > 0) and (Qr > 0) == (ri_len > 0) and (Qc > 0) == (cqi_kind > 0), (name, Qa, Qr, Qc)
            rows.append((mod, tbs, rv, L_prb, nof_symb, Qa, Qr, Qc))
            d["q_%d" % k], d["scr_%d" % k] = q[:H * Qm // 8].copy(), scr[:H * Qm // 8].copy()
            d["pos_%d" % k], d["type_%d" % k] = pos[:n].copy(), typ[:n].copy()
            d["cqi_%d" % k], d["pay_%d" % k] = np.packbits(cqi[:Qc * Qm]), pay[:tbs // 8].copy()
            print("%-36s Q'ack %3d Q'ri %3d Q'cqi %3d  types %s" % (name, Qa, Qr, Qc, np.bincount(typ[:n], minlength=4).tolist()))
        d["cases"] = np.array(rows, np.int32)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
