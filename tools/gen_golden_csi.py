#!/usr/bin/env python3
"""Record what the reference's csi_correction (lib/src/phy/phch/pdsch.c:523-618) gives on seeded inputs: tests/golden/csi_ref.npz.

    python tools/gen_golden_csi.py          (needs the reference tree and oracle/_ref/libsrsran_ref.so, built by `make -C oracle ref`)

The function is static: tools/csi_ref_wrap.c includes the reference's pdsch.c where it lies and exports one wrapper.  It is compiled with the REF_FLAGS of
oracle/Makefile into a temporary directory (nothing compiled is kept) and loaded lazily behind libsrsran_ref.so, which is loaded globally: the call binds
srsran_mod_bits_x_symbol and srsran_vec_max_fi only, both in that library; the other undefined functions of pdsch.c are never bound.

Cases: every modulation (BPSK .. 256-QAM) x both soft-bit widths x nof_re in {2, 3, 8, 301, 516} with CSI random positive and its maximum at a random place
("rand"); at nof_re = 75 an all-equal row ("equal"), a row whose largest and smallest entry are 1e4 apart ("ratio") and one 1e6 apart ("tiny": 16-bit weights
that round to 0 and 1).  Soft bits are uniform over the full range of their width with 0, +-1 and the extremes placed in.  Rows are 64-byte aligned.
tests/test_csi_golden.py holds tests/csi_model.py to this record, element by element."""
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
from gen_golden_spmux import aligned  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "csi_ref.npz")
QM = {0: 1, 1: 2, 2: 4, 3: 6, 4: 8}
SIZES = [2, 3, 8, 301, 516]
EXTRA_N = 75


def ref_flags():
    """REF, RLIB and REF_FLAGS as oracle/Makefile states them"""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    ref = os.environ.get("REF", var["REF"])
    rlib = var["RLIB"].replace("$(REF)", ref)
    return rlib, var["REF_FLAGS"].replace("$(RLIB)", rlib).split()


def soft_bits(rng, nbits, llr8):
    dt = np.int8 if llr8 else np.int16
    info = np.iinfo(dt)
    e = rng.integers(info.min, info.max + 1, nbits).astype(dt)
    special = np.array([0, 1, -1, info.max, info.min, 3, -3], dt)[:nbits]
    e[rng.permutation(nbits)[:special.size]] = special
    return e


def csi_row(rng, n, kind):
    if kind == "equal":
        return np.full(n, 0.73, np.float32)
    if kind in ("ratio", "tiny"):
        span = 4.0 if kind == "ratio" else 6.0
        c = (10.0 ** rng.uniform(-span, 0.0, n)).astype(np.float32) * np.float32(2.5)
        lo, hi = rng.permutation(n)[:2]
        c[hi], c[lo] = np.float32(2.5), np.float32(2.5 * 10.0 ** -span)
        return c
    c = rng.uniform(0.05, 3.0, n).astype(np.float32)
    c[rng.integers(n)] = np.float32(3.25)  # the maximum, somewhere
    return c


def main():
    rlib, flags = ref_flags()
    C.CDLL(O.REF_LIB, mode=os.RTLD_GLOBAL | os.RTLD_NOW)
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libcsi_ref_wrap.so")
        subprocess.check_call(["gcc"] + flags + ['-DREF_PDSCH_C="%s"' % os.path.join(rlib, "src", "phy", "phch", "pdsch.c"), "-shared",
                               os.path.join(ROOT, "tools", "csi_ref_wrap.c"), "-o", so])
        wrap = C.CDLL(so, mode=os.RTLD_LAZY)
        fn = wrap.csi_ref_correction
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_int]
        fn.restype = None
        rng = np.random.default_rng(20)
        cases = [(mod, llr8, n, "rand") for mod in range(5) for llr8 in (0, 1) for n in SIZES]
        cases += [(mod, llr8, EXTRA_N, kind) for mod in range(5) for llr8 in (0, 1) for kind in ("equal", "ratio", "tiny")]
        d = {"cases": np.array([(m, w, n) for m, w, n, _ in cases], np.int32), "kinds": np.array([k for _, _, _, k in cases])}
        for i, (mod, llr8, n, kind) in enumerate(cases):
            e = soft_bits(rng, n * QM[mod], llr8)
            c = csi_row(rng, n, kind)
            ev, eraw = aligned((1, e.size), e.dtype)
            cv, craw = aligned((1, n), np.float32)
            ev[0], cv[0] = e, c
            fn(cv[0].ctypes.data, ev[0].ctypes.data, mod, n * QM[mod], llr8)
            assert np.array_equal(cv[0], c)  # the row is only read
            d["e_%d" % i], d["csi_%d" % i], d["out_%d" % i] = e, c, np.array(ev[0])
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
