"""The model of the convolutional-code receive chain (tests/conv_model.py) against what the reference gave (tests/golden/conv_ref.npz, written by
tools/gen_golden_conv.py from the reference's own viterbi37_avx2_16bit.c, viterbi.c, rm_conv.c and pdcch.c): exact on every case -- quantised symbols, decoded
bits, best state, the 64 final metrics, de-matched floats, crc_rem.  The same on the length sweep (tests/golden/conv_sweep_ref.npz, the generator's --sweep: every
tail-biting frame length 1 .. 144, the tailed lengths around the chain-back's 64-word blocks, 2048 bits, every DCI length 17 .. 144).  And the model against itself: the intrinsic-by-intrinsic step is the plain step the kernel
runs (metrics and decision layout), the lane-owner form of the rate de-matcher gives the reference's sums, clean codewords come back.  No device."""
import os

import numpy as np
import pytest

import conv_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_ref.npz")
SWEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_sweep_ref.npz")  # tools/gen_golden_conv.py --sweep
KIND_F, KIND_S, KIND_US = 0, 1, 2
_rec = _sweep = _sweep_model = None


def record():
    global _rec
    if _rec is None:
        with np.load(GOLDEN) as z:
            _rec = {k: z[k] for k in z.files}
    return _rec


def v_cases():
    """the handle cases: dict(name, kind, tb, framebits, L, gain, vin, sym, bits, best, met)"""
    d = record()
    out = []
    for i, name in enumerate(d["v_names"]):
        kind, tb, framebits, L = (int(v) for v in d["v_cfg"][i])
        out.append(dict(name=str(name), kind=kind, tb=tb, framebits=framebits, L=L, gain=float(d["v_gain"][i]), vin=d["v_in_%d" % i], sym=d["v_sym_%d" % i],
                        bits=d["v_bits_%d" % i], best=int(d["v_best_%d" % i]), met=d["v_met_%d" % i]))
    return out


def p_cases():
    """the PDCCH cases: dict(name, E, nof_bits, rnti, llr, rm, sym, bits, crc, best, met, mean)"""
    d = record()
    out = []
    for i, name in enumerate(d["p_names"]):
        E, nof_bits, rnti = (int(v) for v in d["p_cfg"][i])
        out.append(dict(name=str(name), E=E, nof_bits=nof_bits, rnti=rnti, llr=d["p_llr_%d" % i], rm=d["p_rm_%d" % i], sym=d["p_sym_%d" % i], bits=d["p_bits_%d" % i],
                        crc=int(d["p_crc_%d" % i]), best=int(d["p_best_%d" % i]), met=d["p_met_%d" % i], mean=float(d["p_mean_%d" % i])))
    return out


def sweep_record():
    global _sweep
    if _sweep is None:
        with np.load(SWEEP) as z:
            _sweep = {k: z[k] for k in z.files}
        _sweep["v_bits"], _sweep["p_bits"] = np.unpackbits(_sweep["v_bits"]), np.unpackbits(_sweep["p_bits"])
    return _sweep


def sweep_v_cases():
    """the frames of the length sweep: dict(name, kind, tb, framebits, L, gain, vin, bits, best, met) -- no symbols: the model's are the reference's (asserted by
    the generator)"""
    d = sweep_record()
    out = []
    for i, name in enumerate(d["v_names"]):
        kind, tb, framebits, L, o_in, o_bits = (int(v) for v in d["v_cfg"][i])
        vin = d["v_in_f" if kind == KIND_F else "v_in_us"][o_in:o_in + 3 * (L + (0 if tb else 6))]
        out.append(dict(name=str(name), kind=kind, tb=tb, framebits=framebits, L=L, gain=0.0, vin=vin, bits=d["v_bits"][o_bits:o_bits + L], best=int(d["v_best"][i]),
                        met=d["v_met"][i]))
    return out


def sweep_p_cases():
    """the PDCCH cases of the length sweep: dict(name, E, nof_bits, rnti, llr, bits, crc, best, met)"""
    d = sweep_record()
    out = []
    for i, name in enumerate(d["p_names"]):
        E, nof_bits, rnti, o_llr, o_bits = (int(v) for v in d["p_cfg"][i])
        out.append(dict(name=str(name), E=E, nof_bits=nof_bits, rnti=rnti, llr=d["p_llr"][o_llr:o_llr + E], bits=d["p_bits"][o_bits:o_bits + nof_bits + 16],
                        crc=int(d["p_crc"][i]), best=int(d["p_best"][i]), met=d["p_met"][i]))
    return out


def sweep_model():
    """what the model gives on every case of the sweep, computed once (about ten seconds) and shared, the GPU tests included: (frames, PDCCH cases) in the order of
    sweep_v_cases() / sweep_p_cases(); a frame's entry is M.decode's dict with its symbols added as "sym", a PDCCH case's is M.dci_decode's"""
    global _sweep_model
    if _sweep_model is None:
        V, P = [], []
        for c in sweep_v_cases():
            sym = M.quant_f(c["vin"]) if c["kind"] == KIND_F else c["vin"]
            V.append(dict(M.decode(sym, c["L"], bool(c["tb"])), sym=sym))
        for c in sweep_p_cases():
            P.append(M.dci_decode(c["llr"], c["nof_bits"]))
        _sweep_model = (V, P)
    return _sweep_model


def nw_of(L, tb):
    """decision words the kernel keeps (conv_device.h: nof_words)"""
    return max(2 * L - 6, 0) if tb else L


def test_sweep_record_holds_every_length():
    V, P = sweep_v_cases(), sweep_p_cases()
    tb = [c for c in V if c["tb"] and c["kind"] == KIND_F]
    assert sorted(c["L"] for c in tb) == list(range(1, 145)) and all(c["framebits"] == c["L"] and c["vin"].dtype == np.float32 for c in tb)
    assert {nw_of(c["L"], True) % 64 for c in tb} >= {0, 2, 62}  # the chain-back's last block exactly full, just begun, nearly full
    assert any(nw_of(c["L"], True) < c["L"] for c in tb)  # fewer words than bits: L <= 5
    tailed = [c for c in V if not c["tb"]]
    assert {c["L"] for c in tailed} >= {63, 64, 65, 127, 128} and all(c["kind"] == KIND_US and c["vin"].size == 3 * (c["L"] + 6) for c in tailed)
    assert any(c["L"] == 2048 and c["tb"] for c in V) and all(c["L"] <= c["framebits"] <= 2048 for c in V)
    assert sorted(c["nof_bits"] + 16 for c in P) == list(range(17, 145))
    assert len({(M.rm_geometry(3 * (c["nof_bits"] + 16))[2], c["E"]) for c in P}) == 128 == len(P)  # every ndummy with every E
    assert all(c["llr"].size == c["E"] and M.pdcch_mean(c["llr"], 0, {72: 0, 144: 1, 288: 2, 576: 3}[c["E"]]) > 0.3 for c in P)
    assert os.path.getsize(SWEEP) < 400 * 1024


def test_sweep_frames_model_is_the_reference():
    """every frame of the sweep: decoded bits, best state and the 64 final metrics exact; the best state moot on every tail-biting frame.  The record holds no
    symbol rows (the generator asserted the quantiser against the reference's); the final metrics are sums over every symbol, so they hold the quantiser too"""
    V = sweep_v_cases()
    for c, m in zip(V, sweep_model()[0]):
        assert m["sym"].dtype == np.uint16 and m["sym"].size == c["vin"].size, c["name"]
        assert np.array_equal(m["bits"], c["bits"]) and m["best_state"] == c["best"] and np.array_equal(m["metrics"], c["met"]) and m["best_moot"], c["name"]
        if c["kind"] == KIND_US and not c["tb"] and c["L"] >= 58:
            assert m["wrapped"], c["name"]


def test_sweep_pdcch_cases_model_is_the_reference():
    """every DCI length of the sweep: bits, crc_rem, best state and final metrics exact, and the kernel's form of the de-matcher gives dci_decode's floats"""
    P = sweep_p_cases()
    for c, m in zip(P, sweep_model()[1]):
        assert np.array_equal(m["bits"], c["bits"]) and m["crc_rem"] == c["crc"] and m["best_state"] == c["best"], c["name"]
        assert np.array_equal(m["metrics"], c["met"]) and m["best_moot"], c["name"]
        assert M.rm_rx_owner(c["llr"], 3 * (c["nof_bits"] + 16)).tobytes() == m["rm"].tobytes(), c["name"]
        if c["name"].endswith("clean") and c["E"] >= 3 * (c["nof_bits"] + 16) // 2:
            assert c["crc"] == c["rnti"], c["name"]


def test_record_holds_the_cases_the_kernel_can_go_wrong_on():
    V, P = v_cases(), p_cases()
    assert {c["L"] for c in V} >= {32, 33, 40, 64, 65, 144, 1000} and {c["kind"] for c in V} == {KIND_F, KIND_S, KIND_US}
    assert any(not c["tb"] for c in V) and any(c["L"] < c["framebits"] for c in V) and any(c["gain"] > 1000 for c in V)
    assert any(c["kind"] == KIND_F and not c["vin"].any() for c in V) and any(c["kind"] == KIND_S and {32767, -32767} <= set(c["vin"].tolist()) for c in V)
    assert {(c["E"], c["nof_bits"] + 16) for c in P} >= {(E, L) for E in (72, 144, 288, 576) for L in (40, 32, 33, 64, 65, 144)}
    assert any(c["mean"] == 0 for c in P) and any(0 < c["mean"] <= 0.3 for c in P) and any((c["llr"] == M.RX_NULL).any() for c in P)
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("c", v_cases(), ids=lambda c: c["name"])
def test_handle_cases_model_is_the_reference(c):
    if c["kind"] == KIND_F:
        sym = M.quant_f(c["vin"], c["gain"] if c["gain"] > 0 else M.DEFAULT_GAIN_16)
    else:
        sym = M.quant_s(c["vin"]) if c["kind"] == KIND_S else c["vin"]
    assert np.array_equal(sym, c["sym"])
    m = M.decode(sym, c["L"], bool(c["tb"]))
    assert np.array_equal(m["bits"], c["bits"]) and m["best_state"] == c["best"] and np.array_equal(m["metrics"], c["met"])
    assert m["best_moot"]  # the six zeroed words in front of the chain-back: the best state never reaches a bit
    if c["name"] == "us_144_hard":
        assert m["wrapped"]
    if c["name"] == "f_64_clamps":
        assert sym.min() == 0 and sym.max() == 65535
    if c["name"] == "f_65_zero":
        assert np.all(sym == 32767)


@pytest.mark.parametrize("c", p_cases(), ids=lambda c: c["name"])
def test_pdcch_cases_model_is_the_reference(c):
    m = M.dci_decode(c["llr"], c["nof_bits"])
    assert m["rm"].tobytes() == c["rm"].tobytes() and np.array_equal(m["sym"], c["sym"]) and np.array_equal(m["bits"], c["bits"])
    assert m["crc_rem"] == c["crc"] and m["best_state"] == c["best"] and np.array_equal(m["metrics"], c["met"]) and m["best_moot"]
    assert M.rm_rx_owner(c["llr"], 3 * (c["nof_bits"] + 16)).tobytes() == c["rm"].tobytes()  # the kernel's form: the same sums in the same order
    assert M.pdcch_mean(c["llr"], 0, {72: 0, 144: 1, 288: 2, 576: 3}[c["E"]]) == c["mean"]
    if c["name"].endswith("clean") and c["E"] >= 3 * (c["nof_bits"] + 16) // 2:
        assert c["crc"] == c["rnti"]


def test_quantiser_sum_is_contracted():
    """on the record, the fused form is the reference's and the two-rounding form is not"""
    differs = 0
    for c in v_cases():
        if c["kind"] == KIND_F:
            g = c["gain"] if c["gain"] > 0 else M.DEFAULT_GAIN_16
            assert np.array_equal(M.quant_f(c["vin"], g, contracted=True), c["sym"])
            differs += int(not np.array_equal(M.quant_f(c["vin"], g, contracted=False), c["sym"]))
    assert M.QUANT_CONTRACTED and differs > 0


def test_plain_step_is_the_intrinsics():
    """new metrics, decision layout (pack, movemask, byte swap against 'bit s is state s') and the normalisation block that never subtracts"""
    rng = np.random.default_rng(5)
    for n in range(200):
        old = rng.integers(0, 65536, 64).astype(np.uint16)
        if n % 3 == 0:
            old = (old >> 4).astype(np.uint16) + np.uint16(20000)  # every metric above the 12288 threshold: the block runs and changes nothing
        s = [int(v) for v in rng.integers(0, 65536, 3)]
        if n % 7 == 0:
            s[n % 3] = (0, 65535)[n % 2]
        new, word, _ = M.step(old, *s)
        new_i, dbytes = M.step_intrinsics(old, *s)
        assert np.array_equal(new, new_i)
        assert [M.decision_bit(dbytes, st) for st in range(64)] == [(word >> st) & 1 for st in range(64)]


def test_decode_by_intrinsics_is_decode():
    c = [c for c in v_cases() if c["name"] == "f_33_none"][0]
    a, b = M.decode(c["sym"], 33, True), M.decode(c["sym"], 33, True, stepper=M.step_intrinsics)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["metrics"], b["metrics"]) and a["best_state"] == b["best_state"]
    assert np.array_equal(a["bits"], c["bits"])


def test_rank_of_every_position_is_a_permutation():
    for L in (17, 32, 33, 40, 64, 65, 96, 97, 144):
        ranks = sorted(M.rm_rank(o, 3 * L) for o in range(3 * L))
        assert ranks == list(range(3 * L)), L


def test_clean_codewords_come_back():
    rng = np.random.default_rng(9)
    for L in (32, 33, 40, 65):
        bits = rng.integers(0, 2, L).astype(np.uint8)
        for tb in (True, False):
            sym = M.quant_f(2.0 * M.encode(bits, tb).astype(np.float32) - 1.0)
            assert np.array_equal(M.decode(sym, L, tb)["bits"], bits), (L, tb)
    payload = rng.integers(0, 2, 27).astype(np.uint8)
    for E in (144, 288, 576):
        m = M.dci_decode((2.0 * M.dci_encode(payload, 0x1234, E).astype(np.float32) - 1.0) * 3.0, 27)
        assert m["crc_rem"] == 0x1234 and np.array_equal(m["bits"][:27], payload), E
