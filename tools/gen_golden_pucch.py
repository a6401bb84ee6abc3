#!/usr/bin/env python3
"""Record what the reference's PUCCH receive side gives on seeded inputs: tests/golden/pucch_ref.npz.

    python tools/gen_golden_pucch.py          (needs the reference tree)

tools/pucch_ref_wrap.c includes the reference's pucch.c where it lies and is compiled with the REF_FLAGS of oracle/Makefile, together with the reference
files the calls bind into (where they lie), into a temporary directory (nothing compiled is kept) and loaded lazily.

A case is one job: a cell (6 PRB normal prefix, 6 PRB extended prefix, 25 PRB normal prefix with group hopping), a subframe (tti 0 or 7, shortened or not),
a resource and its settings.  The UE's signal is the reference's own (encode_signal and pucch_put, what srsran_pucch_encode runs behind encode_bits, plus
srsran_refsignal_dmrs_pucch_gen / _put), through a two-tap channel behind a delay of 0 to 1 us with an independent phase per slot, plus noise at 10 or
30 dB; one case per family is noise alone.  Only the two column blocks of the resource are stored: the rest of the grid is seeded noise that the tests
regenerate (pucch_model.full_grid).  The record also holds the two tables the library takes from its caller, and n_cs_cell / f_gh of each cell, as the
running reference reported them.

Conditions, asserted on the reference alone; a case that fails one is drawn again, and after 20 draws the generator fails:
  every correlation and dmrs_correlation lies more than 100 tolerances from each threshold it is compared with; the winning 1A / 1B candidate and the winning
  DRS hypothesis lead the runner-up by more than 100 tolerances (candidates and hypothesis sums from the float64 model, whose decisions equal the
  reference's); the best CQI word leads by at least 2; every unquantised soft bit lies more than 100 of z's tolerances from an integer, and |llr| < 16384
  (the int16 product of srsran_vec_dot_prod_sss does not wrap); ta_us unrounded is at least 0.01 us from a rounding boundary and each phasor sum is at
  least 0.1 of its terms' magnitudes (tools/gen_golden_chest_ul.py's rule).
Tolerances: per float quantity the worst deviation of the model from the reference over all cases, times four.  The draws use a provisional value; the
conditions are asserted again with the stored one."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pucch_ref.npz")
REF_FILES = ["ch_estimation/chest_ul.c", "ch_estimation/chest_common.c", "ch_estimation/refsignal_ul.c", "utils/convolution.c", "utils/vector.c", "utils/vector_simd.c",
             "utils/debug.c", "utils/phy_logger.c", "utils/bit.c", "utils/primes.c", "common/phy_common.c", "common/sequence.c", "common/zc_sequence.c",
             "phch/sequences.c", "phch/uci.c", "phch/cqi.c", "modem/mod.c", "modem/demod_soft.c", "modem/modem_table.c", "modem/lte_tables.c", "scrambling/scrambling.c",
             "mimo/precoding.c", "dft/dft_precoding.c", "fec/block/block.c"]
W = np.float32(0.3333)
FILTER = np.array([W, np.float32(1) - np.float32(2) * W, W], np.float32)
CELLS = {"A": (6, 0, 1), "B": (6, 1, 77), "C": (25, 0, 150)}
TH = (0.5, 0.5, 0.5)
PROVISIONAL = {"z": 1.2e-6, "other": 6e-6}


def cases():
    """(cell, tti, shortened, format, n_pucch, N_cs, delta, n_rb_2, nof_uci_bits, bits, drs, snr_db or None, filter_on, meas_ta_en, th_dmrs)"""
    out = []
    F1, F1A, F1B, F2, F2A, F2B = range(6)
    # formats 1x: delta 1, 2, 3; N_cs 0 and not; n_pucch on both sides of c N_cs / delta; every n_oc with both parities of n'; shortened on and off
    f1 = [("A", 0, 0, F1, 0, 0, 1, 0), ("A", 0, 1, F1A, 1, 0, 1, 0), ("A", 7, 0, F1B, 13, 0, 1, 0), ("A", 7, 1, F1A, 26, 0, 1, 0), ("A", 0, 0, F1B, 35, 0, 1, 0),
          ("A", 0, 0, F1A, 2, 4, 2, 1), ("A", 7, 1, F1B, 5, 4, 2, 1), ("A", 7, 0, F1A, 7, 4, 2, 1), ("A", 0, 1, F1B, 20, 4, 2, 1), ("A", 0, 0, F1, 3, 6, 3, 0),
          ("A", 7, 1, F1A, 8, 6, 3, 1), ("A", 7, 0, F1B, 11, 3, 3, 1), ("B", 0, 0, F1, 0, 0, 1, 0), ("B", 0, 1, F1A, 5, 0, 1, 0), ("B", 7, 0, F1B, 14, 0, 1, 0),
          ("B", 7, 1, F1A, 1, 4, 2, 1), ("B", 0, 0, F1B, 9, 4, 2, 1), ("B", 0, 0, F1A, 17, 6, 3, 0), ("C", 0, 0, F1, 4, 0, 1, 2), ("C", 0, 1, F1A, 40, 0, 2, 2),
          ("C", 7, 0, F1B, 3, 6, 2, 2), ("C", 7, 1, F1B, 30, 6, 2, 2), ("C", 0, 0, F1A, 77, 3, 3, 1), ("C", 7, 0, F1A, 101, 0, 1, 3)]
    for i, (cell, tti, short, fmt, n_pucch, N_cs, delta, n_rb_2) in enumerate(f1):
        bits = {F1: (0, 0), F1A: (i % 2, 0), F1B: ((i // 2) % 2, i % 2)}[fmt]
        out.append((cell, tti, short, fmt, n_pucch, N_cs, delta, n_rb_2, 0, bits, (0, 0), 30.0 if i % 3 == 0 else 10.0, 1, 1, 0.0))
    # every bit value of 1A and 1B on one resource
    for b in range(2):
        out.append(("A", 0, 0, F1A, 6, 0, 2, 0, 0, (b, 0), (0, 0), 10.0, 1, 1, 0.0))
    for b in range(4):
        out.append(("C", 7, 1, F1B, 9, 4, 2, 2, 0, (b >> 1, b & 1), (0, 0), 10.0, 1, 1, 0.0))
    # format 2 with 1, 4, 11, 12 bits, n_pucch on both sides of 12 n_rb_2
    f2 = [("A", 0, F2, 3, 0, 1, 1, 1), ("A", 7, F2, 17, 4, 2, 1, 4), ("A", 0, F2, 7, 0, 1, 2, 11), ("A", 7, F2, 30, 2, 2, 2, 12), ("B", 0, F2, 5, 0, 1, 1, 4),
          ("B", 7, F2, 14, 4, 2, 1, 11), ("C", 0, F2, 20, 6, 3, 2, 12), ("C", 7, F2, 29, 0, 1, 2, 1), ("C", 0, F2, 2, 0, 2, 1, 11)]
    rng = np.random.default_rng(5)
    for i, (cell, tti, fmt, n_pucch, N_cs, delta, n_rb_2, nbits) in enumerate(f2):
        out.append((cell, tti, 0, fmt, n_pucch, N_cs, delta, n_rb_2, nbits, tuple(int(v) for v in rng.integers(0, 2, nbits)), (0, 0), 30.0 if i % 2 else 10.0, 1, 1, 0.0))
    for b in range(2):
        out.append(("A", 0, 0, F2A, 4, 0, 1, 1, 4, tuple(int(v) for v in rng.integers(0, 2, 4)), (b, 0), 10.0, 1, 1, 0.0))
    for b in range(4):
        out.append(("C", 7, 0, F2B, 15, 4, 2, 2, 11, tuple(int(v) for v in rng.integers(0, 2, 11)), (b & 1, b >> 1), 30.0 if b % 2 else 10.0, 1, 1, 0.0))
    # noise alone, one per family; smoothing off; time alignment not measured; DMRS detection on, with a noise-only case that returns early
    out.append(("A", 0, 0, F1A, 1, 0, 1, 0, 0, (0, 0), (0, 0), None, 1, 1, 0.0))
    out.append(("A", 7, 0, F2, 3, 0, 1, 1, 1, (1,), (0, 0), None, 1, 1, 0.0))
    out.append(("A", 0, 0, F1B, 13, 0, 1, 0, 0, (1, 0), (0, 0), 10.0, 0, 1, 0.0))
    out.append(("C", 7, 0, F2, 29, 0, 1, 2, 11, tuple(int(v) for v in rng.integers(0, 2, 11)), (0, 0), 30.0, 0, 1, 0.0))
    out.append(("B", 0, 1, F1A, 5, 0, 1, 0, 0, (1, 0), (0, 0), 10.0, 1, 0, 0.0))
    out.append(("A", 0, 0, F1A, 1, 0, 1, 0, 0, (1, 0), (0, 0), 10.0, 1, 1, 0.4))
    out.append(("C", 0, 0, F2, 20, 6, 3, 2, 4, (1, 0, 1, 1), (0, 0), 30.0, 1, 1, 0.4))
    out.append(("B", 7, 0, F1B, 14, 0, 1, 0, 0, (0, 1), (0, 0), 10.0, 1, 1, 0.4))
    out.append(("A", 7, 0, F1A, 7, 4, 2, 1, 0, (0, 0), (0, 0), None, 1, 1, 0.4))
    return out


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libpucch_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_PUCCH_C="%s"' % os.path.join(phy, "phch", "pucch.c"), "-shared", os.path.join(ROOT, "tools", "pucch_ref_wrap.c")] +
                          [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    L = C.CDLL(so, mode=os.RTLD_LAZY)
    vp, u32 = C.c_void_p, C.c_uint32
    L.pucch_ref_open.argtypes = [u32, u32, u32]
    L.pucch_ref_tables.argtypes = [vp, vp, vp, vp]
    L.pucch_ref_plan.argtypes = [vp, vp]
    L.pucch_ref_encode.argtypes = [vp, vp, vp, vp]
    L.pucch_ref_decode.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


def words(M, j, sf):
    return np.array([j[k] for k in M.JOB_FIELDS[:9]] + [sf["tti"], sf["shortened"]], np.uint32)


def run_reference(L, M, cell, sf, j, grid):
    nsymb = 6 if cell["cp"] else 7
    d = words(M, j, sf)
    ce = np.zeros(2 * nsymb * 12 * cell["nof_prb"], np.complex64)
    outf, outb, z, llr, pe = np.zeros(13, np.float32), np.zeros(15, np.uint8), np.zeros(120, np.complex64), np.zeros(20, np.int16), np.zeros(72, np.complex64)
    mc = np.zeros(1, np.int32)
    th = np.array([j[k] for k in M.TH_FIELDS], np.float32)
    g = np.array(grid)
    flen, filt = (3, FILTER) if j["filter_len"] == 3 else (1, np.ones(1, np.float32))
    rc = L.pucch_ref_decode(d.ctypes.data, flen, filt.ctypes.data, th.ctypes.data, g.ctypes.data, ce.ctypes.data, outf.ctypes.data, outb.ctypes.data, z.ctypes.data,
                            llr.ctypes.data, pe.ctypes.data, mc.ctypes.data)
    assert rc == 0 and np.array_equal(g, grid)
    return dict(ce=ce.reshape(2 * nsymb, -1), outf=outf, outb=outb, z=z, llr=llr, pe=pe, max_corr=int(mc[0]))


def rel(a, b):
    a, b = float(a), float(b)
    if a == b or (np.isnan(a) and np.isnan(b)):
        return 0.0
    return abs(a - b) / abs(b)


OUTF = ("detected", "correlation", "dmrs_correlation", "ack_valid", "noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "rsrp", "rsrp_dBfs", "epre", "epre_dBfs", "ta_us")


def distances(M, p, j, ref, m):
    """the reference's distance to the model: ce and z relative to the row maximum, the rest relative"""
    n_rs, nsymb = int(p["n_rs"]), ref["ce"].shape[0] // 2
    rows = np.stack([ref["ce"][s * nsymb, 12 * p["n_prb"][s]:12 * p["n_prb"][s] + 12] for s in range(2)])
    d = {"ce": float(np.max(np.abs(rows.astype(np.complex128) - m["ce"])) / np.max(np.abs(m["ce"]))),
         "pe": float(np.max(np.abs(ref["pe"][:2 * n_rs * 12].reshape(-1, 12).astype(np.complex128) - m["pe"])) / np.max(np.abs(m["pe"])))}
    nof_re = 12 * int(p["N_sf"].sum())
    lo = 10 if j["format"] >= M.F2 and not m["early"] else 0  # formats 2x: the reference overwrites z[0 .. 9] with the symbol averages
    zm = m["z"].reshape(-1)
    d["z"] = float(np.max(np.abs(ref["z"][lo:nof_re].astype(np.complex128) - zm[lo:])) / np.max(np.abs(zm)))
    for k in M.FLOATS:
        d[k] = rel(ref["outf"][OUTF.index(k)], m[k])
    return d


def conditions(M, j, m, tol):
    """None, or which condition the case fails"""
    if j["meas_ta_en"]:
        if np.any(np.abs(m["ta_sums"]) < 0.1 * m["ta_mags"]):
            return "ta phasor sum"
        x = m["ta_unrounded"] * 10.0
        if abs((x - np.floor(x)) - 0.5) * 0.1 < 0.01:
            return "ta rounding"
    if M._isnormal(np.float32(j["threshold_dmrs_detection"])) and abs(m["dmrs_correlation"] - j["threshold_dmrs_detection"]) <= 100 * tol["dmrs_correlation"]:
        return "dmrs threshold"
    if j["format"] >= M.F2A:
        a = sorted(m["drs_abs"])
        if a[-1] - a[-2] <= 100 * tol["pe"] * a[-1]:
            return "drs hypothesis"
    if m["early"]:
        return None
    c = float(m["correlation"])
    ths = {M.F1: ("threshold_format1",), M.F1A: ("threshold_format1", "threshold_data_valid_format1a"), M.F1B: ("threshold_format1", "threshold_data_valid_format1a")}
    for k in ths.get(j["format"], ("threshold_data_valid_format2",)):
        if abs(c - j[k]) <= 100 * tol["correlation"] * max(abs(c), 1e-3):
            return "correlation threshold"
    if j["format"] in (M.F1A, M.F1B):
        a = sorted(float(v) for v in m["cands"])
        if a[-1] - a[-2] <= 100 * tol["correlation"]:
            return "candidate lead"
    if j["format"] >= M.F2:
        if m["runner_up"] is not None and m["max_corr"] - m["runner_up"] < 2:
            return "word lead"
        if np.max(np.abs(m["llr"].astype(np.int64))) >= 16384:
            return "llr range"
        zmax = float(np.max(np.abs(m["z"])))
        if np.min(np.abs(m["soft"] - np.rint(m["soft"]))) <= 100 * tol["z"] * zmax * 100 * np.sqrt(2.0):
            return "soft bit boundary"
    return None


def draw(L, M, rng, cell, sf, j, p, bits, drs, snr_db):
    """the job's two column blocks [2, 7, 12]: the reference's UE signal through the channel, plus noise (or noise alone)"""
    nsymb, nof_prb = (6 if cell["cp"] else 7), cell["nof_prb"]
    cols = np.zeros((2, 7, 12), np.complex64)
    tx = np.zeros(2 * nsymb * 12 * nof_prb, np.complex64)
    if snr_db is not None:
        d = words(M, j, sf)
        b, dr = np.array(list(bits) + [0, 0], np.uint8), np.array(drs, np.uint8)
        assert L.pucch_ref_encode(d.ctypes.data, b.ctypes.data, dr.ctypes.data, tx.ctypes.data) == 0
    tx = tx.reshape(2 * nsymb, -1)
    tau = rng.uniform(0.0, 1.0e-6)
    sigma = (10 ** (-(snr_db if snr_db is not None else 0.0) / 20)) / np.sqrt(2)
    for s in range(2):
        k = np.arange(12 * p["n_prb"][s], 12 * p["n_prb"][s] + 12)
        taps = np.array([1.0, rng.uniform(0.0, 0.25)]) * np.exp(2j * np.pi * rng.random(2))
        h = taps[0] * np.exp(-2j * np.pi * 15e3 * k * tau) + taps[1] * np.exp(-2j * np.pi * 15e3 * k * (tau + rng.uniform(0.1e-6, 0.4e-6)))
        h /= np.sqrt(np.mean(np.abs(h) ** 2))
        y = tx[s * nsymb:(s + 1) * nsymb, k] * h[None, :] + sigma * (rng.standard_normal((nsymb, 12)) + 1j * rng.standard_normal((nsymb, 12)))
        cols[s, :nsymb] = y.astype(np.complex64)
    return cols


def main():
    import pucch_model as M

    with tempfile.TemporaryDirectory() as tmp:
        L = load_wrapper(tmp)
        # the tables first: the model reads them from the record being built
        assert L.pucch_ref_open(6, 0, 1) == 0
        base, basis = np.zeros((30, 12), np.complex64), np.zeros((13, 20), np.uint8)
        rec = {"cell_names": np.array(sorted(CELLS)), "n_cs_cell": np.zeros((3, 20, 7), np.uint32), "f_gh": np.zeros((3, 20), np.uint32)}
        for i, name in enumerate(sorted(CELLS)):
            assert L.pucch_ref_open(*CELLS[name]) == 0
            L.pucch_ref_tables(base.ctypes.data, basis.ctypes.data, rec["n_cs_cell"][i].ctypes.data, rec["f_gh"][i].ctypes.data)
        rec.update(base=base, basis=basis, cells=np.array([CELLS[k] for k in sorted(CELLS)], np.uint32))
        M._rec = rec
        tol = {k: PROVISIONAL.get(k, PROVISIONAL["other"]) for k in M.FLOATS + ("ce", "z", "pe")}
        kept, worst = [], {k: 0.0 for k in tol}
        for c, (cn, tti, short, fmt, n_pucch, N_cs, delta, n_rb_2, nbits, bits, drs, snr, filter_on, meas_ta, th_dmrs) in enumerate(cases()):
            cell = dict(zip(M.CELL_FIELDS, CELLS[cn]))
            sf = {"tti": tti, "shortened": short}
            j = dict(zip(M.JOB_FIELDS, (fmt, n_pucch, N_cs, delta, n_rb_2, 1 if cn == "C" else 0, 0x1234 + c, nbits, meas_ta, 3 if filter_on else 0)))
            j["filter"] = [float(v) for v in FILTER] if filter_on else [0.0, 0.0, 0.0]
            j.update(zip(M.TH_FIELDS, (float(np.float32(v)) for v in TH + (th_dmrs,))))
            assert L.pucch_ref_open(*CELLS[cn]) == 0
            p = M.plan(cell, sf, j)
            pw = np.zeros(65, np.uint32)
            assert p is not None and L.pucch_ref_plan(words(M, j, sf).ctypes.data, pw.ctypes.data) == 0
            mw = M.plan_words(p)
            if fmt >= M.F2:
                mw[37:47] = 0  # n_prime of formats 2x is not exposed by the reference
            assert np.array_equal(mw, pw), (c, mw, pw)
            why = "never drawn"
            for attempt in range(20):
                rng = np.random.default_rng(7000 + 100 * c + attempt)
                cols = draw(L, M, rng, cell, sf, j, p, bits, drs, snr)
                grid = M.full_grid(c, cell["nof_prb"], 6 if cell["cp"] else 7, p["n_prb"], cols[:, :6 if cell["cp"] else 7])
                ref = run_reference(L, M, cell, sf, j, grid)
                m = M.decode(grid, cell, sf, j, p)
                why = conditions(M, j, m, tol)
                if why is None and snr is None and ref["outf"][0]:
                    why = "noise alone was detected"
                if why is None:
                    break
            assert why is None, (c, why)
            # the model's decisions are the reference's
            o = ref["outf"]
            assert bool(o[0]) == m["detected"] and bool(o[3]) == m["ack_valid"] and np.array_equal(ref["outb"][:13], m["pucch_bits"]), (c, o, m["pucch_bits"], ref["outb"], m["correlation"], m["cands"], m["detected"], m["ack_valid"])
            assert list(ref["outb"][13:]) == [m["drs"] % 2, m["drs"] // 2] and np.array_equal(ref["llr"], m["llr"]) and ref["max_corr"] == m["max_corr"], c
            assert abs(float(o[12]) - float(m["ta_us"])) < 0.01, (c, o[12], m["ta_us"])
            if snr is not None and not m["early"]:
                want = list(bits[:nbits]) if fmt >= M.F2 else list(bits[:{M.F1: 0, M.F1A: 1, M.F1B: 2}[fmt]])
                got = list(m["pucch_bits"][:len(want)])
                assert got == want and m["detected"], (c, got, want)
                assert [m["drs"] % 2, m["drs"] // 2] == list(drs), c
            dist = distances(M, p, j, ref, m)
            for k in worst:
                worst[k] = max(worst[k], dist[k])
            kept.append(dict(cell=[cell[k] for k in M.CELL_FIELDS], sf=[tti, short], job=[j[k] for k in M.JOB_FIELDS], filter=j["filter"], th=[j[k] for k in M.TH_FIELDS],
                             plan=pw, cols=cols, ce=np.stack([ref["ce"][s * (6 if cell["cp"] else 7), 12 * p["n_prb"][s]:12 * p["n_prb"][s] + 12] for s in range(2)]),
                             pe=ref["pe"], z=ref["z"], llr=ref["llr"], outf=o, outb=ref["outb"], max_corr=ref["max_corr"], early=int(m["early"]),
                             noise_only=int(snr is None), sent=np.array(list(bits) + [0] * (13 - len(bits)), np.uint8), sent_drs=np.array(drs, np.uint8),
                             ref_ce_elsewhere_untouched=int(np.count_nonzero(ref["ce"]) == 2 * (6 if cell["cp"] else 7) * 12)))
            print("case %2d %s fmt %d n_pucch %3d: draw %d, corr %.4f dmrs %.4f" % (c, cn, fmt, n_pucch, attempt, o[1], o[2]))
        final = {k: 4.0 * v for k, v in worst.items()}
        print("tolerances:", {k: "%.3g" % v for k, v in final.items()})
        assert all(v <= tol[k] for k, v in final.items()), "a stored tolerance is above the provisional value the draws used"
        rec.update({k: np.array([e[k] for e in kept]) for k in kept[0]})
        rec["tol_names"] = np.array(sorted(final))
        rec["tol"] = np.array([final[k] for k in sorted(final)], np.float64)
        rec["job"] = rec["job"].astype(np.uint32)
        np.savez_compressed(OUT, **rec)
        # with the record in place: every case again through the public loader, conditions under the stored tolerances
        M._rec = None
        for c in range(M.n_cases()):
            cell, sf, j, grid = M.case(c)
            assert conditions(M, j, M.decode(grid, cell, sf, j), final) is None, c
    print("wrote %s (%d cases, %d bytes)" % (OUT, len(kept), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
