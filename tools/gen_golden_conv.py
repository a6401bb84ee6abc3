#!/usr/bin/env python3
"""Record what the reference's 16-bit tail-biting Viterbi decoder (srsran_viterbi_decode_f / _s / _us on an AVX2 host: viterbi.c:548-617,
viterbi37_avx2_16bit.c) and srsran_pdcch_dci_decode (pdcch.c:335-368: srsran_rm_conv_rx, the decoder, the 16-bit CRC) give on seeded inputs:
tests/golden/conv_ref.npz.

    python tools/gen_golden_conv.py          (needs the reference tree)
    python tools/gen_golden_conv.py --sweep  (the length sweep, tests/golden/conv_sweep_ref.npz: main_sweep(); conv_ref.npz is left alone)

tools/conv_ref_wrap.c includes the reference's viterbi37_avx2_16bit.c where it lies (struct v37 is read) and is compiled with the REF_FLAGS of oracle/Makefile,
together with viterbi.c, rm_conv.c, pdcch.c and the reference files they bind into, into a temporary directory (nothing compiled is kept); loaded lazily.

The model (tests/conv_model.py) must equal the reference EXACTLY on every case -- de-matched floats, quantised symbols, decoded bits, best state, the 64 final
metrics, crc_rem -- which is asserted here; so is that the quantiser's sum is contracted the way the model says, that the case meant to wrap its metrics did,
and that the chain-back through the six zeroed words makes the best state moot on every tail-biting case.

Handle cases (V_*): frame lengths 40 (PBCH), 32, 33, 64, 65, 144 with a codeword at an SNR from clean downwards and with no codeword at all (random soft bits:
ties, the best-state rule and the wrap decide), a 1000-bit frame, a 40-bit frame on a 144-bit handle, an all-zero frame (the 1e-9 floor), a gain that hits both
clamps, a frame on which the quantiser's sum rounds differently when it is contracted, int16 input at +-32767, uint16 input straight in (uniform over the whole range: the metrics wrap), one frame without tail biting per input kind.
PDCCH cases (P_*): E of 72, 144, 288, 576 against every one of those lengths (nrows 1, 2, 2, 3, 5; ndummy 0, 31, 0, 31, 16; puncturing and up to 6 contributions
per position), SNR rotating from clean to none, soft bits that are or sum to SRSRAN_RX_NULL, an all-zero region and one whose mean is below 0.3."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_model as M  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_ref.npz")
OUT_SWEEP = os.path.join(ROOT, "tests", "golden", "conv_sweep_ref.npz")
REF_FILES = ["fec/convolutional/viterbi.c", "fec/convolutional/viterbi37_port.c", "fec/convolutional/viterbi37_sse.c", "fec/convolutional/viterbi37_avx2.c",
             "fec/convolutional/parity.c", "fec/turbo/rm_conv.c", "phch/pdcch.c", "fec/crc.c", "utils/bit.c", "utils/vector.c", "utils/vector_simd.c",
             "utils/debug.c", "utils/phy_logger.c"]
LENGTHS = [40, 32, 33, 64, 65, 144]
SNRS = [None, 6.0, 0.0, -6.0]  # None: clean
KIND_F, KIND_S, KIND_US = 0, 1, 2


def soft(rng, coded, snr_db, amp=2.0):
    """soft bits of a coded sequence: positive is 1.  snr_db None: clean; 'none': no codeword behind them"""
    if isinstance(snr_db, str):
        return (amp * rng.standard_normal(coded.size)).astype(np.float32)
    x = 2.0 * coded.astype(np.float64) - 1.0
    if snr_db is not None:
        x = x + 10 ** (-snr_db / 20) * rng.standard_normal(coded.size)
    return (amp * x).astype(np.float32)


def v_cases(rng):
    cases = []

    def add(name, kind, tb, framebits, L, vin, gain=0.0):
        cases.append(dict(name=name, kind=kind, tb=tb, framebits=framebits, L=L, vin=vin, gain=gain))

    for n, L in enumerate(LENGTHS):
        snr = SNRS[n % len(SNRS)]
        add("f_%d_snr_%s" % (L, "clean" if snr is None else "%g" % snr), KIND_F, 1, L, L, soft(rng, M.encode(rng.integers(0, 2, L), True), snr))
        add("f_%d_none" % L, KIND_F, 1, L, L, soft(rng, np.zeros(3 * L), "none"))
    add("f_1000_snr_0", KIND_F, 1, 1000, 1000, soft(rng, M.encode(rng.integers(0, 2, 1000), True), 0.0))
    add("f_40_on_144", KIND_F, 1, 144, 40, soft(rng, M.encode(rng.integers(0, 2, 40), True), 3.0))
    add("f_65_zero", KIND_F, 1, 65, 65, np.zeros(3 * 65, np.float32))
    add("f_64_clamps", KIND_F, 1, 64, 64, soft(rng, M.encode(rng.integers(0, 2, 64), True), 0.0), gain=1.0e6)
    s = rng.integers(-32767, 32768, 3 * 65).astype(np.int16)
    s[rng.permutation(s.size)[:60]] = np.tile(np.array([32767, -32767], np.int16), 30)
    add("s_65_extremes", KIND_S, 1, 65, 65, s)
    add("s_40_codeword", KIND_S, 1, 40, 40, np.clip(3000.0 * soft(rng, M.encode(rng.integers(0, 2, 40), True), 0.0), -32767, 32767).astype(np.int16))
    add("us_144_hard", KIND_US, 1, 144, 144, rng.integers(0, 65536, 3 * 144).astype(np.uint16))
    add("us_33_none", KIND_US, 1, 33, 33, rng.integers(0, 65536, 3 * 33).astype(np.uint16))
    add("f_40_tailed", KIND_F, 0, 40, 40, soft(rng, M.encode(rng.integers(0, 2, 40), False), 3.0))
    add("us_65_tailed", KIND_US, 0, 65, 65, rng.integers(0, 65536, 3 * 71).astype(np.uint16))
    add("s_33_tailed_on_64", KIND_S, 0, 64, 33, rng.integers(-32767, 32768, 3 * 39).astype(np.int16))
    add("f_32_contraction", KIND_F, 1, 32, 32, contraction_frame(rng, 3 * 32))
    return cases


def contraction_frame(rng, n):
    """soft bits on which the quantiser's sum gives another integer as one fused multiply-add than as a product and a sum: the case that lets the record say
    how the reference's sum was compiled (they are rare: about 3 in 100000 uniform draws)"""
    found = [np.array([3.0], np.float32)]  # the maximum: a gain of 1000 / 3
    while sum(f.size for f in found) < n:
        x = np.append(rng.uniform(-3.0, 3.0, 1 << 20).astype(np.float32), np.float32(3.0))
        found.append(x[M.quant_f(x, contracted=True) != M.quant_f(x, contracted=False)])
    return np.concatenate(found)[:n]


def p_cases(rng):
    cases = []
    snrs = SNRS + ["none"]
    n = 0
    for E in (72, 144, 288, 576):
        for L in LENGTHS:
            nof_bits, snr = L - 16, snrs[n % len(snrs)]
            n += 1
            rnti = int(rng.integers(1, 0xFFF0))
            tx = M.dci_encode(rng.integers(0, 2, nof_bits), rnti, E)
            cases.append(dict(name="E%d_L%d_%s" % (E, L, "clean" if snr is None else snr), E=E, nof_bits=nof_bits, llr=soft(rng, tx, snr), rnti=rnti))
    llr = soft(rng, M.dci_encode(rng.integers(0, 2, 16), 77, 288), 6.0)
    llr[[0, 5, 96 + 7, 192 + 9]] = M.RX_NULL  # a first contribution that reads as empty, later ones that are skipped
    llr[11], llr[96 + 11] = 4000.0, 6000.0  # a sum that reads as empty when the third contribution arrives
    cases.append(dict(name="E288_L32_rx_null", E=288, nof_bits=16, llr=llr, rnti=77))
    cases.append(dict(name="E144_L40_zero", E=144, nof_bits=24, llr=np.zeros(144, np.float32), rnti=0))
    cases.append(dict(name="E72_L33_mean_0.25", E=72, nof_bits=17, llr=(0.125 * soft(rng, M.dci_encode(rng.integers(0, 2, 17), 5, 72), None)).astype(np.float32),
                      rnti=5))
    return cases


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libconv_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_V37_C="%s"' % os.path.join(phy, "fec", "convolutional", "viterbi37_avx2_16bit.c"), "-shared",
                           os.path.join(ROOT, "tools", "conv_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    lib = C.CDLL(so, mode=os.RTLD_LAZY)
    vp = C.c_void_p
    lib.conv_ref_viterbi.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, vp]
    lib.conv_ref_dci.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    return lib


def ref_viterbi(lib, c):
    L, nsym = c["L"], 3 * (c["L"] + (0 if c["tb"] else 6))
    vin = np.ascontiguousarray(c["vin"])
    assert vin.size == nsym, (c["name"], vin.size, nsym)
    bits, sym, best, met = np.full(L, 9, np.uint8), np.zeros(nsym, np.uint16), np.zeros(1, np.uint32), np.zeros(64, np.uint16)
    keep = vin.copy()
    rc = lib.conv_ref_viterbi(c["kind"], c["tb"], c["framebits"], L, C.c_float(c["gain"]), vin.ctypes.data, bits.ctypes.data, sym.ctypes.data, best.ctypes.data,
                              met.ctypes.data)
    assert rc == c["framebits"], (c["name"], rc)  # the functions return q->framebits
    assert np.array_equal(vin, keep)
    if c["kind"] == KIND_US:
        sym = vin.copy()
    return bits, sym, int(best[0]), met


def ref_dci(lib, c):
    n = 3 * (c["nof_bits"] + 16)
    llr = np.ascontiguousarray(c["llr"], np.float32)
    rm, sym, bits = np.zeros(n, np.float32), np.zeros(n, np.uint16), np.full(c["nof_bits"] + 16, 9, np.uint8)
    crc, best, met = np.zeros(1, np.uint16), np.zeros(1, np.uint32), np.zeros(64, np.uint16)
    rc = lib.conv_ref_dci(llr.ctypes.data, c["E"], c["nof_bits"], rm.ctypes.data, sym.ctypes.data, bits.ctypes.data, crc.ctypes.data, best.ctypes.data,
                          met.ctypes.data)
    assert rc == 0, (c["name"], rc)
    return rm, sym, bits, int(crc[0]), int(best[0]), met


def model_sym(c):
    if c["kind"] == KIND_F:
        return M.quant_f(c["vin"], c["gain"] if c["gain"] > 0 else M.DEFAULT_GAIN_16)
    return M.quant_s(c["vin"]) if c["kind"] == KIND_S else np.asarray(c["vin"], np.uint16)


def main():
    rng = np.random.default_rng(2311)
    V, P = v_cases(rng), p_cases(rng)
    d = {"v_names": np.array([c["name"] for c in V]), "p_names": np.array([c["name"] for c in P]),
         "v_cfg": np.array([[c["kind"], c["tb"], c["framebits"], c["L"]] for c in V], np.uint32), "v_gain": np.array([c["gain"] for c in V], np.float32),
         "p_cfg": np.array([[c["E"], c["nof_bits"], c["rnti"]] for c in P], np.uint32)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_wrapper(tmp)
        clamps = set()
        for i, c in enumerate(V):
            bits, sym, best, met = ref_viterbi(lib, c)
            msym = model_sym(c)
            if c["kind"] == KIND_F and not np.array_equal(msym, sym):  # which way the quantiser's sum was compiled: told once, then asserted
                other = M.quant_f(c["vin"], c["gain"] if c["gain"] > 0 else M.DEFAULT_GAIN_16, contracted=not M.QUANT_CONTRACTED)
                raise AssertionError("%s: quantiser differs; the other contraction %s" % (c["name"], "matches" if np.array_equal(other, sym) else "differs too"))
            assert np.array_equal(msym, sym), c["name"]
            m = M.decode(sym, c["L"], bool(c["tb"]))
            assert np.array_equal(m["bits"], bits) and m["best_state"] == best and np.array_equal(m["metrics"], met) and m["best_moot"], c["name"]
            if c["name"] == "us_144_hard":
                assert m["wrapped"], "the metrics of the hard case did not wrap"
            if c["name"] == "f_64_clamps":
                clamps = {int(sym.min()), int(sym.max())}
            if c["name"] == "f_65_zero":
                assert np.all(sym == 32767)
            if c["name"] == "f_32_contraction":
                assert np.count_nonzero(M.quant_f(c["vin"], contracted=not M.QUANT_CONTRACTED) != sym) >= c["vin"].size - 1
            print("V %-22s best %2d  wrapped %d  ones %d / %d" % (c["name"], best, m["wrapped"], int(bits.sum()), bits.size))
            d["v_in_%d" % i], d["v_sym_%d" % i], d["v_bits_%d" % i], d["v_best_%d" % i], d["v_met_%d" % i] = np.asarray(c["vin"]), sym, bits, np.uint32(best), met
        assert clamps == {0, 65535}, clamps
        for i, c in enumerate(P):
            rm, sym, bits, crc, best, met = ref_dci(lib, c)
            m = M.dci_decode(c["llr"], c["nof_bits"])
            assert rm.tobytes() == m["rm"].tobytes() and rm.tobytes() == M.rm_rx_owner(c["llr"], rm.size).tobytes(), c["name"]
            assert np.array_equal(sym, m["sym"]) and np.array_equal(bits, m["bits"]) and crc == m["crc_rem"] and best == m["best_state"], c["name"]
            assert np.array_equal(met, m["metrics"]) and m["best_moot"], c["name"]
            mean = M.pdcch_mean(c["llr"], 0, {72: 0, 144: 1, 288: 2, 576: 3}[c["E"]])
            print("P %-22s crc_rem %04x (rnti %04x)  mean %.4f  wrapped %d" % (c["name"], crc, c["rnti"], mean, m["wrapped"]))
            d["p_llr_%d" % i], d["p_rm_%d" % i], d["p_sym_%d" % i], d["p_bits_%d" % i] = np.asarray(c["llr"], np.float32), rm, sym, bits
            d["p_crc_%d" % i], d["p_best_%d" % i], d["p_met_%d" % i], d["p_mean_%d" % i] = np.uint16(crc), np.uint32(best), met, np.float64(mean)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(V), "handle cases,", len(P), "PDCCH cases")


# ---------------------------------------------------------------------------------------------------------------- the length sweep
SWEEP_TAILED = [1, 2, 5, 6, 7, 58, 62, 63, 64, 65, 66, 127, 128, 129]
SWEEP_E = (72, 144, 288, 576)


def sweep_E(L):
    """every one of the 128 pairs (ndummy, E) once over L = 17 .. 144"""
    return SWEEP_E[((L - 17) // 32 + L % 32) % 4]


def sweep_v_cases(rng):
    cases = []
    snrs = SNRS + ["none"]

    def label(snr):
        return "clean" if snr is None else snr if isinstance(snr, str) else "snr_%g" % snr

    for L in range(1, 145):  # tail biting, float soft bits, default gain: every length
        snr = snrs[(L - 1) % len(snrs)] if L >= 7 else "none"  # M.encode needs six bits in front of the first with tail biting
        coded = np.zeros(3 * L) if isinstance(snr, str) else M.encode(rng.integers(0, 2, L), True)
        cases.append(dict(name="f_%d_%s" % (L, label(snr)), kind=KIND_F, tb=1, framebits=L, L=L, vin=soft(rng, coded, snr), gain=0.0))
    for L in SWEEP_TAILED:  # tailed, uint16 straight in, uniform over the whole range: the metrics wrap
        cases.append(dict(name="us_%d_tailed" % L, kind=KIND_US, tb=0, framebits=L, L=L, vin=rng.integers(0, 65536, 3 * (L + 6)).astype(np.uint16), gain=0.0))
    for L, tb in ((2048, 1), (2047, 0)):  # the frames that size the LDS at its limit: symbols of a noisy codeword
        sym = M.quant_f(soft(rng, M.encode(rng.integers(0, 2, L), bool(tb)), 0.0))
        cases.append(dict(name="us_%d_%s" % (L, "snr_0" if tb else "tailed_on_2048"), kind=KIND_US, tb=tb, framebits=2048, L=L, vin=sym, gain=0.0))
    return cases


def sweep_p_cases(rng):
    cases = []
    snrs = SNRS + ["none"]
    for L in range(17, 145):
        nof_bits, E, snr = L - 16, sweep_E(L), snrs[(L - 17) % len(snrs)]
        rnti = int(rng.integers(1, 0xFFF0))
        tx = M.dci_encode(rng.integers(0, 2, nof_bits), rnti, E)
        cases.append(dict(name="L%d_E%d_%s" % (L, E, "clean" if snr is None else snr), E=E, nof_bits=nof_bits, llr=soft(rng, tx, snr, amp=2.0), rnti=rnti))
    return cases


def pack_table(rows):
    """arrays of one type one behind the other -> (the whole, the offset of each)"""
    off = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint32)
    return np.concatenate(rows), off[:-1]


def main_sweep():
    """tests/golden/conv_sweep_ref.npz: every frame length 1 .. 144 with tail biting, the tailed lengths around the chain-back's 64-word blocks, the two frames at
    the LDS limit, and every DCI length 17 .. 144 (every ndummy with every E once).  Inputs and what the reference gave (bits packed, crc_rem, best state, final
    metrics), a few concatenated arrays and an offset table; the model is asserted against the reference on every case, exactly as in main()."""
    rng = np.random.default_rng(2412)
    V, P = sweep_v_cases(rng), sweep_p_cases(rng)
    assert len({(rm_geometry_ndummy(c["nof_bits"] + 16), c["E"]) for c in P}) == 128
    v_bits, v_best, v_met, p_bits, p_crc, p_best, p_met = [], [], [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_wrapper(tmp)
        for c in V:
            bits, sym, best, met = ref_viterbi(lib, c)
            assert np.array_equal(model_sym(c), sym), c["name"]
            m = M.decode(sym, c["L"], bool(c["tb"]))
            assert np.array_equal(m["bits"], bits) and m["best_state"] == best and np.array_equal(m["metrics"], met) and m["best_moot"], c["name"]
            if c["kind"] == KIND_US and c["L"] >= 58:
                assert m["wrapped"], c["name"]
            print("V %-22s best %2d  wrapped %d  ones %d / %d" % (c["name"], best, m["wrapped"], int(bits.sum()), bits.size))
            v_bits.append(bits), v_best.append(best), v_met.append(met)
        for c in P:
            rm, sym, bits, crc, best, met = ref_dci(lib, c)
            m = M.dci_decode(c["llr"], c["nof_bits"])
            assert rm.tobytes() == m["rm"].tobytes() and rm.tobytes() == M.rm_rx_owner(c["llr"], rm.size).tobytes(), c["name"]
            assert np.array_equal(sym, m["sym"]) and np.array_equal(bits, m["bits"]) and crc == m["crc_rem"] and best == m["best_state"], c["name"]
            assert np.array_equal(met, m["metrics"]) and m["best_moot"], c["name"]
            mean = M.pdcch_mean(c["llr"], 0, SWEEP_E.index(c["E"]))
            assert mean > 0.3, (c["name"], mean)
            print("P %-22s crc_rem %04x (rnti %04x)  mean %.4f  wrapped %d" % (c["name"], crc, c["rnti"], mean, m["wrapped"]))
            p_bits.append(bits), p_crc.append(crc), p_best.append(best), p_met.append(met)
    d = {"v_names": np.array([c["name"] for c in V]), "p_names": np.array([c["name"] for c in P])}
    in_f, off_f = pack_table([c["vin"] for c in V if c["kind"] == KIND_F])
    in_us, off_us = pack_table([c["vin"] for c in V if c["kind"] == KIND_US])
    off_in = {KIND_F: iter(off_f), KIND_US: iter(off_us)}
    allbits, off_bits = pack_table(v_bits)
    d["v_in_f"], d["v_in_us"], d["v_bits"] = in_f.astype(np.float32), in_us.astype(np.uint16), np.packbits(allbits)
    # per frame: kind, tail biting, framebits, L, where its input starts in v_in_f / v_in_us, where its bits start in the unpacked v_bits
    d["v_cfg"] = np.array([[c["kind"], c["tb"], c["framebits"], c["L"], next(off_in[c["kind"]]), off_bits[i]] for i, c in enumerate(V)], np.uint32)
    d["v_best"], d["v_met"] = np.array(v_best, np.uint8), np.array(v_met, np.uint16)
    llr, off_llr = pack_table([c["llr"] for c in P])
    allbits, off_bits = pack_table(p_bits)
    d["p_llr"], d["p_bits"] = llr.astype(np.float32), np.packbits(allbits)
    # per candidate: E, nof_bits, rnti, where its soft bits start in p_llr, where its nof_bits + 16 bits start in the unpacked p_bits
    d["p_cfg"] = np.array([[c["E"], c["nof_bits"], c["rnti"], off_llr[i], off_bits[i]] for i, c in enumerate(P)], np.uint32)
    d["p_crc"], d["p_best"], d["p_met"] = np.array(p_crc, np.uint16), np.array(p_best, np.uint8), np.array(p_met, np.uint16)
    np.savez_compressed(OUT_SWEEP, **d)
    size = os.path.getsize(OUT_SWEEP)
    print(OUT_SWEEP, size, "bytes,", len(V), "frames,", len(P), "PDCCH cases")
    assert size < 400 * 1024, size


def rm_geometry_ndummy(L):
    return M.rm_geometry(3 * L)[2]


if __name__ == "__main__":
    if "--sweep" in sys.argv[1:]:
        main_sweep()
    else:
        main()
