#!/usr/bin/env python3
"""Record what the reference's srsran_chest_ul_estimate_pusch (lib/src/phy/ch_estimation/chest_ul.c:370-404) gives on seeded inputs:
tests/golden/chest_ul_ref.npz.

    python tools/gen_golden_chest_ul.py          (needs the reference tree)

tools/chest_ul_ref_wrap.c includes the reference's chest_ul.c where it lies and exports one wrapper.  It is compiled with the REF_FLAGS of oracle/Makefile,
together with the reference files the call binds into (chest_common.c, convolution.c, refsignal_ul.c, dft_precoding.c, vector.c, vector_simd.c, debug.c,
phy_logger.c, where they lie), into a temporary directory (nothing compiled is kept) and loaded lazily: convolution.c needs no FFTW header and the FFT
symbols it and dft_precoding.c leave undefined are never bound.

Cases: L_prb in {1, 2, 6, 25, 100} on cells of 6, 6, 15, 25 and 100 PRB, with a non-zero first PRB where one fits (1: twelve references, both end rules
inside one quarter wave; 6: more than one wave; 25: 300 references are more than one stride of 256 lanes, with a ragged tail; 100: the largest LDS use
in practice); normal and extended cyclic prefix; SNR 0, 10 and 30 dB on a frequency-selective channel with a delay of 0 to 2.6 us and a carrier offset
within +-300 Hz; smoothing on, and off at one point per size; time alignment measured, with one case where it is not.  Two 100-PRB cases.  r is random
unit-modulus: the estimator never looks inside it.  The grid outside the two reference rows is random; the ce grid is full of a sentinel.

A case is drawn again unless (a) each phasor sum (CFO, both time-alignment sums) has a magnitude of at least 0.1 of the sum of its terms' magnitudes and
(b) the unrounded ta_us lies at least 0.01 us from a rounding boundary (9e-4 rad of phasor angle, far above any summation-order effect).

Per case the record holds rx (the two received reference rows), r, the reference's two ce rows, its six outputs, whether it left everything outside the
grant's columns untouched and wrote the slot's row to every symbol of the slot, and its own distance to the float64 model (tests/chest_ul_model.py):
rows relative to max |ce|, noise_estimate and snr relative, cfo_hz in Hz, ta_us in steps of 0.1 us."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chest_ul_model as M  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "chest_ul_ref.npz")
W = np.float32(0.3333)
FILTER = np.array([W, np.float32(1) - np.float32(2) * W, W], np.float32)
SENTINEL = np.complex64(-7.5 + 3.25j)
REF_FILES = ["ch_estimation/chest_common.c", "utils/convolution.c", "ch_estimation/refsignal_ul.c", "dft/dft_precoding.c", "utils/vector.c",
             "utils/vector_simd.c", "utils/debug.c", "utils/phy_logger.c"]
SHAPES = [(1, 6, 3), (2, 6, 2), (6, 15, 4), (25, 25, 0), (100, 100, 0)]  # L_prb, cell PRBs, first PRB


def cases():
    """(L_prb, nof_prb, n_prb, cp_nsymb, snr_db, filter_on, meas_ta_en)"""
    out = []
    for L_prb, nof_prb, n_prb in SHAPES:
        if L_prb == 100:
            out += [(L_prb, nof_prb, n_prb, 7, 10.0, 1, 1), (L_prb, nof_prb, n_prb, 6, 30.0, 1, 1)]
            continue
        out += [(L_prb, nof_prb, n_prb, cp, snr, 1, 1) for cp in (7, 6) for snr in (0.0, 10.0, 30.0)]
        out.append((L_prb, nof_prb, n_prb, 7, 10.0, 0, 1))
    out.append((6, 15, 4, 7, 10.0, 1, 0))
    return out


def draw(rng, L_prb, nof_prb, n_prb, cp_nsymb, snr_db):
    """(grid, r): unit-modulus r through a three-path channel behind a bulk delay, a carrier offset between the slots, noise"""
    n = 12 * L_prb
    r = np.exp(2j * np.pi * rng.random(2 * n)).astype(np.complex64)
    k = np.arange(12 * n_prb, 12 * n_prb + n)
    tau0 = rng.uniform(0.0, 2.0e-6)
    taus = tau0 + np.array([0.0, rng.uniform(0.1e-6, 0.3e-6), rng.uniform(0.3e-6, 0.6e-6)])
    amps = np.array([1.0, 0.5, 0.3]) * np.exp(2j * np.pi * rng.random(3))
    h = (amps[None, :] * np.exp(-2j * np.pi * 15e3 * k[:, None] * taus[None, :])).sum(axis=1)
    h /= np.sqrt(np.mean(np.abs(h) ** 2))
    cfo = rng.uniform(-300.0, 300.0)
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    grid = (0.7 * (rng.standard_normal((2 * cp_nsymb, 12 * nof_prb)) + 1j * rng.standard_normal((2 * cp_nsymb, 12 * nof_prb)))).astype(np.complex64)
    for s in range(2):
        y = h * r[s * n:(s + 1) * n] * np.exp(2j * np.pi * cfo * 0.0005 * s) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        grid[M.ref_symbol(s, cp_nsymb), 12 * n_prb:12 * n_prb + n] = y.astype(np.complex64)
    return np.ascontiguousarray(grid.reshape(-1)), r


def well_conditioned(rx, ls, sm, meas_ta_en):
    _, _, cfo, ta = M.sums(rx, ls, sm)
    if abs(cfo) < 0.1 * np.sum(np.abs(ls[0] * np.conj(ls[1]))):
        return False
    for s in range(2):
        if abs(ta[s]) < 0.1 * np.sum(np.abs(ls[s, 1:] * np.conj(ls[s, :-1]))):
            return False
    if meas_ta_en:
        x = M.ta_unrounded(ta) * 10.0
        if abs((x - np.floor(x)) - 0.5) * 0.1 < 0.01:
            return False
    return True


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libchest_ul_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_CHEST_UL_C="%s"' % os.path.join(phy, "ch_estimation", "chest_ul.c"), "-shared",
                           os.path.join(ROOT, "tools", "chest_ul_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    fn = C.CDLL(so, mode=os.RTLD_LAZY).chest_ul_ref
    fn.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def run_reference(fn, grid, r, nof_prb, cp_nsymb, n_prb, L_prb, filter_on, meas_ta_en):
    """(ce grid [2 cp_nsymb, 12 nof_prb], six outputs)"""
    ce = np.full(2 * cp_nsymb * 12 * nof_prb, SENTINEL, np.complex64)
    out6 = np.zeros(6, np.float32)
    g, rr = np.array(grid), np.array(r)
    rc = fn(nof_prb, 1 if cp_nsymb == 6 else 0, n_prb, L_prb, 3 if filter_on else 0, FILTER.ctypes.data, meas_ta_en, rr.ctypes.data, g.ctypes.data, ce.ctypes.data,
            out6.ctypes.data)
    assert rc == 0 and np.array_equal(g, grid) and np.array_equal(rr, r)  # both are only read
    return ce.reshape(2 * cp_nsymb, 12 * nof_prb), out6


def distances(sm, m, rows, out6):
    """the reference's distance to the float64 model: rows / max |ce|, noise and snr relative, cfo in Hz, ta in steps of 0.1 us"""
    rel = lambda a, b: 0.0 if (a == b or (np.isnan(a) and np.isnan(b))) else abs(float(a) - float(b)) / abs(float(b))  # noqa: E731
    return np.array([np.max(np.abs(rows.astype(np.complex128) - sm)) / np.max(np.abs(sm)), rel(out6[0], m["noise_estimate"]), rel(out6[2], m["snr"]),
                     abs(float(out6[4]) - float(m["cfo_hz"])), round(abs(float(out6[5]) - float(m["ta_us"])) * 10.0)], np.float64)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_wrapper(tmp)
        rng = np.random.default_rng(31)
        cs = cases()
        d = {"cases": np.array([(L, p, a, cp, f, t) for L, p, a, cp, _, f, t in cs], np.int32), "snr_db": np.array([c[4] for c in cs], np.float32),
             "filter": FILTER, "sentinel": np.array([SENTINEL])}
        worst = np.zeros(5)
        for i, (L_prb, nof_prb, n_prb, cp_nsymb, snr_db, filter_on, meas_ta_en) in enumerate(cs):
            filt = FILTER if filter_on else None
            while True:
                grid, r = draw(rng, L_prb, nof_prb, n_prb, cp_nsymb, snr_db)
                rx, ls, sm = M.rows(grid, r, nof_prb, cp_nsymb, (n_prb, n_prb), L_prb, filt)
                if well_conditioned(rx, ls, sm, meas_ta_en):
                    break
            ce, out6 = run_reference(fn, grid, r, nof_prb, cp_nsymb, n_prb, L_prb, filter_on, meas_ta_en)
            n, a = 12 * L_prb, 12 * n_prb
            rows = np.stack([ce[M.ref_symbol(s, cp_nsymb), a:a + n] for s in range(2)])
            inside = np.zeros(ce.shape, bool)
            inside[:, a:a + n] = True
            untouched = bool(np.all(ce[~inside] == SENTINEL))
            copied = all(np.array_equal(ce[l, a:a + n], rows[l // cp_nsymb]) for l in range(2 * cp_nsymb))
            m = M.measurements(*M.sums(rx, ls, sm), filt, meas_ta_en)
            dist = distances(sm, m, rows, out6)
            worst = np.maximum(worst, dist)
            d["rx_%d" % i], d["r_%d" % i], d["ce_%d" % i], d["out_%d" % i] = rx.astype(np.complex64), r, rows, out6
            d["flags_%d" % i], d["dist_%d" % i] = np.array([untouched, copied]), dist
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(cs), "cases; the reference's worst distance to the model (rows, noise, snr, cfo Hz, ta steps):", worst)


if __name__ == "__main__":
    main()
