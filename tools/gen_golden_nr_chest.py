#!/usr/bin/env python3
"""Record what the reference's srsran_dmrs_sch_estimate (lib/src/phy/ch_estimation/dmrs_sch.c:763-986) and srsran_dmrs_sch_get_symbols_idx (:395-435) give
on seeded inputs: tests/golden/nr_chest_ref.npz.

    python tools/gen_golden_nr_chest.py          (needs the reference tree)

tools/nr_chest_ref_wrap.c includes the reference's dmrs_sch.c where it lies and exports one wrapper.  It is compiled with the REF_FLAGS of oracle/Makefile,
together with the reference files the calls bind into, into a temporary directory (nothing compiled is kept) and loaded lazily.

Cases (CASES below): the smallest shapes at which the estimator's kernel can go wrong -- type 1 on 1 of 6 PRB (6 pilots: both filter end rules inside one
wave), 2 non-adjacent of 6, 11 of 25 with a hole, 25 of 25 (150 pilots: a ragged third wave), 52 of 106 with a hole, 106 of 106, 275 of 275; type 2 on 1,
25 and 106 PRB; 1, 2, 3 and 4 DMRS symbols through additional_pos and S + L, one double-length case (and the 275-PRB one); typeA_pos 2 and 3; S > 0 with a
last symbol that is not 13; 1 and 2 (and 3) CDM groups without data; beta_dmrs != 1; n_scid = 1; a reserved pattern with a stride and a case with two
patterns; SNR 0 / 10 / 30 dB on a three-path channel behind a bulk delay with a carrier offset; and a noiseless flat-channel case on which sync_err and the CFO
are exactly zero, so that both isnormal branches are skipped.  The grants of the large cases are short (few symbols) to keep the record small.

A case is drawn again unless each phasor sum (the lag-1 sums, the corr[i+1] conj(corr[i]) products) has a magnitude of at least 0.1 of the sum of its terms'
magnitudes.  The reference's own ce must lie within 2.5e-5 of max |ce| from the model (tests/nr_chest_model.py) on every case: asserted here.

Per case the record holds the configuration, the received DMRS rows and the seed that regenerates the rest of the grid (fill_grid), the reference's extracted
ce, its eight outputs, what srsran_dmrs_sch_get_symbols_idx returned, and the reference's own distance to the float64 model: ce relative to max |ce|,
noise_estimate, rsrp and sync_error relative, cfo in Hz."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nr_chest_model as M  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nr_chest_ref.npz")
REF_FILES = ["ch_estimation/chest_common.c", "utils/convolution.c", "resampling/interp.c", "utils/vector.c", "utils/vector_simd.c", "utils/re_pattern.c",
             "common/sequence.c", "common/phy_common_nr.c", "utils/debug.c", "utils/phy_logger.c"]
CFG_KEYS = ["nof_prb", "scs", "slot_idx", "S", "L", "dmrs_type", "typeA_pos", "additional_pos", "length", "n_id", "n_scid", "cdm"]


def prbs(nof_prb, *spans):
    p = np.zeros(nof_prb, np.uint8)
    for a, b in spans:
        p[a:b] = 1
    return p


def case(name, nof_prb, prb, snr_db, dmrs_type=0, S=0, L=14, typeA_pos=2, additional_pos=0, length=1, cdm=2, beta=1.0, n_scid=0, rvd=(), scs=0, flat=False,
         delay=1.0):
    return dict(name=name, nof_prb=nof_prb, prb=prb, snr_db=snr_db, dmrs_type=dmrs_type, S=S, L=L, typeA_pos=typeA_pos, additional_pos=additional_pos,
                length=length, cdm=cdm, beta=beta, n_scid=n_scid, rvd=list(rvd), scs=scs, flat=flat, delay=delay, slot_idx=3 + nof_prb % 7, n_id=41 + nof_prb)


CASES = [
    case("t1_1of6", 6, prbs(6, (3, 4)), 30.0, cdm=1),
    case("t1_2of6", 6, prbs(6, (1, 2), (4, 5)), 10.0, additional_pos=1),
    case("t1_11of25_hole", 25, prbs(25, (3, 9), (14, 19)), 0.0, S=2, L=10, typeA_pos=3, additional_pos=2),
    case("t1_25of25", 25, prbs(25, (0, 25)), 10.0, additional_pos=3, beta=1.4125, rvd=[(1, 25, 3, 0x249, 0x0003)]),
    case("t1_52of106_hole", 106, prbs(106, (10, 36), (50, 76)), 10.0, additional_pos=1, n_scid=1, scs=1, S=1, L=11,
         rvd=[(0, 106, 2, 0x00f, 0x0010), (40, 60, 1, 0xf00, 0x0820)]),
    case("t1_106of106", 106, prbs(106, (0, 106)), 30.0, L=7, scs=1, delay=0.5),
    case("t1_275of275", 275, prbs(275, (0, 275)), 10.0, L=4, length=2, scs=1, delay=0.25),
    case("t2_1of6", 6, prbs(6, (2, 3)), 30.0, dmrs_type=1, cdm=1),
    case("t2_25of25", 25, prbs(25, (0, 25)), 10.0, dmrs_type=1, additional_pos=2),
    case("t2_106of106", 106, prbs(106, (0, 106)), 0.0, dmrs_type=1, L=9, additional_pos=1, cdm=3, scs=1, delay=0.5),
    case("t1_double_25", 25, prbs(25, (0, 25)), 10.0, length=2, additional_pos=1),
    case("t1_flat_6", 6, prbs(6, (0, 6)), None, additional_pos=1, flat=True),
]


def fill_grid(seed, nof_prb):
    """the grid outside the DMRS rows: what the tests regenerate from the recorded seed"""
    rng = np.random.default_rng(int(seed))
    return (0.7 * (rng.standard_normal((14, 12 * nof_prb)) + 1j * rng.standard_normal((14, 12 * nof_prb)))).astype(np.complex64)


def draw(rng, c, gseed):
    """the received grid of a case: DMRS through the channel on the DMRS symbols, random points everywhere else"""
    grid = fill_grid(gseed, c["nof_prb"])
    tx = np.zeros((14, 12 * c["nof_prb"]), np.complex128)
    M.put_dmrs(tx, c)
    cols, _ = M.pilot_columns(c)
    if c["flat"]:  # +-0.5 +-0.5j: every product with the pilots' amplitude is exact in float32, contracted or not, and every phasor sum is real
        for l in M.dmrs_symbols(c):
            grid[l, cols] = (0.5 * M.dmrs_signs(c, l)).astype(np.complex64)
        return grid
    k = np.arange(12 * c["nof_prb"])
    scs_hz = 15e3 * (1 << c["scs"])
    tau0 = rng.uniform(0.2e-6, 1.0e-6) * c["delay"] / (1 << c["scs"])
    taus = tau0 + np.array([0.0, rng.uniform(0.05e-6, 0.15e-6), rng.uniform(0.15e-6, 0.3e-6)]) * c["delay"] / (1 << c["scs"])
    amps = np.array([1.0, 0.5, 0.3]) * np.exp(2j * np.pi * rng.random(3))
    h = (amps[None, :] * np.exp(-2j * np.pi * scs_hz * k[:, None] * taus[None, :])).sum(axis=1)
    h /= np.sqrt(np.mean(np.abs(h) ** 2))
    cfo = rng.uniform(-300.0, 300.0)
    sigma = 10 ** (-c["snr_db"] / 20) / np.sqrt(2)
    for l in M.dmrs_symbols(c):
        t = l * 2192.0 / (15000.0 * 2048.0) / (1 << c["scs"])
        y = h[cols] * tx[l, cols] * np.exp(2j * np.pi * cfo * t) + sigma * (rng.standard_normal(cols.size) + 1j * rng.standard_normal(cols.size))
        grid[l, cols] = y.astype(np.complex64)
    return grid


def well_conditioned(m):
    return bool(np.all(np.abs(m["lag1"]) >= 0.1 * m["lag1_abs"]) and np.all(np.abs(m["cross"]) >= 0.1 * m["cross_abs"]))


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libnr_chest_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_DMRS_SCH_C="%s"' % os.path.join(phy, "ch_estimation", "dmrs_sch.c"), "-shared",
                           os.path.join(ROOT, "tools", "nr_chest_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    fn = C.CDLL(so, mode=os.RTLD_LAZY).nr_chest_ref
    fn.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    return fn


def cfg_array(c):
    return np.array([c[k] for k in CFG_KEYS] + [len(c["rvd"])], np.uint32)


def run_reference(fn, c, grid):
    cfg, rvd = cfg_array(c), np.array(c["rvd"], np.uint32).reshape(-1, 5)
    rvd = np.ascontiguousarray(rvd) if rvd.size else np.zeros((1, 5), np.uint32)
    g = np.array(grid.reshape(-1), np.complex64)
    ce = np.zeros(14 * 12 * c["nof_prb"], np.complex64)
    out8, sym5 = np.zeros(8, np.float32), np.zeros(5, np.int32)
    prb = np.ascontiguousarray(c["prb"], np.uint8)
    rc = fn(cfg.ctypes.data, C.c_float(c["beta"]), rvd.ctypes.data, prb.ctypes.data, g.ctypes.data, ce.ctypes.data, out8.ctypes.data, sym5.ctypes.data)
    assert rc == 0 and np.array_equal(g, grid.reshape(-1))  # the grid is only read
    return ce[:int(out8[7])].copy(), out8, sym5


def distances(m, ce, out8):
    rel = lambda a, b: 0.0 if a == b else (np.inf if b == 0 else abs(float(a) - float(b)) / abs(float(b)))  # noqa: E731
    return np.array([np.max(np.abs(ce.astype(np.complex128) - m["ce"])) / np.max(np.abs(m["ce"])), rel(out8[0], m["noise_estimate"]), rel(out8[2], m["rsrp"]),
                     abs(float(out8[5]) - float(m["cfo"])), rel(out8[6], m["sync_error"])], np.float64)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_wrapper(tmp)
        rng = np.random.default_rng(47)
        d = {"names": np.array([c["name"] for c in CASES]), "snr_db": np.array([np.nan if c["snr_db"] is None else c["snr_db"] for c in CASES], np.float32)}
        worst = np.zeros(5)
        for i, c in enumerate(CASES):
            while True:
                gseed = int(rng.integers(1, 2 ** 31))
                grid = draw(rng, c, gseed)
                m = M.estimate(grid, c)
                if c["flat"] or well_conditioned(m):
                    break
            ce, out8, sym5 = run_reference(fn, c, grid)
            sym = M.dmrs_symbols(c)
            assert sym5[0] == len(sym) and list(sym5[1:1 + len(sym)]) == sym, (c["name"], sym5, sym)
            assert int(out8[7]) == m["nof_re"] == M.nof_re(c), (c["name"], out8[7], m["nof_re"])
            dist = distances(m, ce, out8)
            print("%-18s nof_re %6d  dist (ce, noise, rsrp, cfo Hz, sync)" % (c["name"], m["nof_re"]), dist)
            assert dist[0] <= 2.5e-5, (c["name"], dist)
            if c["flat"]:
                assert out8[5] == 0 and out8[6] == 0, out8
            worst = np.maximum(worst, dist)
            d["cfg_%d" % i], d["beta_%d" % i], d["prb_%d" % i] = cfg_array(c), np.float32(c["beta"]), np.asarray(c["prb"], np.uint8)
            d["rvd_%d" % i] = np.array(c["rvd"], np.uint32).reshape(-1, 5)
            d["gseed_%d" % i], d["rows_%d" % i] = np.int64(gseed), grid[sym].astype(np.complex64)
            d["ce_%d" % i], d["out_%d" % i], d["sym_%d" % i], d["dist_%d" % i] = ce, out8, sym5, dist
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases; the reference's worst distance to the model (ce, noise, rsrp, cfo Hz, sync):", worst)


if __name__ == "__main__":
    main()
