"""One device call per grant (include/srsran_amd/phy_chan_abi.h): srsran_hip_pusch_decode{,_multi}, srsran_hip_pdsch_decode, srsran_hip_pdsch_encode,
srsran_hip_ulsch_encode, srsran_hip_modulate_bytes.

Receive side: the test signal comes from the ORACLE's transmit chain (payload -> CRC / segmentation / turbo code / rate matching -> [UL channel
interleaver] -> scrambling -> constellation -> [transform precoding] -> grid, a frequency-selective channel and noise on top).  What the fused call
returns is held to the oracle's decode_tb (orc_sch_decode_tb: verdict, payload bytes, half iterations per block, soft-buffer rows of failed blocks)
run on the soft bits the SAME stages produce one call at a time through the reference-named entry points (srsran_predecoding_single ->
srsran_dft_precoding -> srsran_demod_soft_demodulate_{s,b} -> srsran_sequence_pusch_apply_{s,c}; each of them is held to the oracle in
test_gpu_modem.py / test_gpu_dft.py) and the oracle's channel de-interleaver.  Transmit side: bit-exact against the oracle's chain, which
tests/test_oracle_golden.py pins to the reference's modulator output.

Which test holds what to what:
  test_pusch_grant_in_one_call, test_pdsch_codeword_in_one_call   verdict, payload, iteration average (PUSCH: EPRE; PDSCH: the _dbg call's symbols and soft bits) to the
                                                                  oracle, on grants that DECODE: a data soft bit in the wrong slot can decode to the same payload
  test_pusch_grant_harq_and_failure                               the rows of failed blocks to the oracle over three transmissions, at one shape (20 PRB, 16-QAM)
  test_pusch_grants_of_a_tti_in_one_call, *_from_worker_threads   the _multi call to the SINGLE call, not to the oracle
  test_*_encode_*, test_modulator_*                               the transmit side bit for bit to the oracle's chain / the reference's tables
  tests/test_gpu_chan_softbits.py                                 the PLACEMENT of every transport-block soft bit to the oracle: grants of random bits, where no block
                                                                  decodes and all rows come back -- every modulation, store width and column count, small and
                                                                  tile-crossing allocations, with control information, single and _multi calls, PDSCH
_pusch_signal = a code word's bits + _pusch_grid (bits -> grid), which that module feeds with random bits."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_api as O
from grant_helpers import SB, _rx_softbuffer, _tx_softbuffer

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _oracle_tx_bits(tbs, Qm, nof_bits, rv, payload_bits):
    """e bits of the transport block (transmit-side block order, sch.c:284) as uint8 [nof_bits]"""
    e, _ = O.tb_coded_bits(tbs, Qm, nof_bits, rv, None, payload=payload_bits, tx_order=True)
    assert e.size == nof_bits
    return e


def _pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, rv, rnti, tti, cell_id, snr_db, payload_bits):
    """the subframe grid a UE's PUSCH leaves at the eNB (pusch.c:258-350 srsran_pusch_encode without UCI) through a channel: returns (grid, ce, seed)"""
    Qm = O.QM[mod]
    nsymb = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    nof_re = nsymb * 12 * L_prb
    g = _oracle_tx_bits(tbs, Qm, nof_re * Qm, rv, payload_bits)
    lut = O.ulsch_interleaver_lut(nof_re, Qm, nsymb)
    q = g[lut]  # q[position] = g[lut[position]] (sch.c:995-1018: the de-interleaver reads q through the same table)
    return _pusch_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, q, rnti, tti, cell_id, snr_db)


def _pusch_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, q, rnti, tti, cell_id, snr_db):
    """the "bits -> grid" half of the signal path: the interleaved bits q (uint8 [nof_re Qm], a code word or anything else) -> scrambling -> constellation ->
    transform precoding -> the allocation's REs of the subframe grid, a frequency-selective channel with per-symbol phase and noise: (grid, ce, seed)"""
    Qm = O.QM[mod]
    nsymb = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    nsc = 12 * L_prb
    nof_re = nsymb * nsc
    assert q.size == nof_re * Qm
    seed = O.pusch_seed(rnti, 2 * (tti % 10), cell_id)
    d = O.modulate_bytes(mod, np.packbits(q), nof_re * Qm, seed=seed, scramble=True)
    z = (np.fft.fft(d.reshape(nsymb, nsc).astype(np.complex128), axis=1) / np.sqrt(nsc)).astype(np.complex64)  # srsran_dft_precoding, tx: forward, normalised
    grid = np.zeros((2 * cp_nsymb, 12 * nof_prb), np.complex64)
    ce = np.zeros_like(grid)
    # a frequency-selective channel over the whole grid + per-symbol phase drift
    k = np.arange(12 * nof_prb)
    h = (0.9 + 0.2 * np.exp(2j * np.pi * k / 97.0) + 0.1 * np.exp(-2j * np.pi * k / 31.0))
    L_ref = 3 if cp_nsymb == 7 else 2
    row = 0
    for slot in range(2):
        nl = cp_nsymb - (1 if (shortened and slot == 1) else 0)
        for l in range(nl):
            sym = l + slot * cp_nsymb
            hs = (h * np.exp(1j * 0.03 * sym)).astype(np.complex64)
            ce[sym] = hs
            if l == L_ref:
                continue
            a = 12 * n_prb[slot]
            grid[sym, a:a + nsc] = z[row] * hs[a:a + nsc]
            row += 1
    assert row == nsymb
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    grid = (grid + sigma * (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape))).astype(np.complex64)
    # unused symbols of ce stay zero (nothing may read them)
    return np.ascontiguousarray(grid.reshape(-1)), np.ascontiguousarray(ce.reshape(-1)), seed


def _per_stage_pusch_llrs(lib, capi, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, rnti, tti, cell_id, noise, llr8, symbols_out=None):
    """pusch.c:383-443 one reference-named call at a time on the library (four device round trips): returns the q soft bits.  symbols_out: a list that gets the
    symbols the demodulator was given"""
    nsymb = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    nsc = 12 * L_prb
    nof_re = nsymb * nsc
    L_ref = 3 if cp_nsymb == 7 else 2
    y, h = [], []
    for slot in range(2):
        nl = cp_nsymb - (1 if (shortened and slot == 1) else 0)
        for l in range(nl):
            if l == L_ref:
                continue
            a = ((l + slot * cp_nsymb) * nof_prb + n_prb[slot]) * 12
            y.append(grid[a:a + nsc])
            h.append(ce[a:a + nsc])
    y, h = np.ascontiguousarray(np.concatenate(y)), np.ascontiguousarray(np.concatenate(h))
    x = np.zeros(nof_re, np.complex64)
    assert lib.srsran_predecoding_single(O.P(y), O.P(h), O.P(x), None, nof_re, 1.0, noise) == nof_re
    pre = capi.DftPrecoding()
    assert lib.srsran_dft_precoding_init(C.byref(pre), L_prb, False) == 0
    d = np.zeros(nof_re, np.complex64)
    assert lib.srsran_dft_precoding(C.byref(pre), O.P(x), O.P(d), L_prb, nsymb) == 0
    lib.srsran_dft_precoding_free(C.byref(pre))
    Qm = O.QM[mod]
    dt = np.int8 if llr8 else np.int16
    llr = np.zeros(nof_re * Qm, dt)
    assert (lib.srsran_demod_soft_demodulate_b if llr8 else lib.srsran_demod_soft_demodulate_s)(mod, O.P(d), O.P(llr), nof_re) == 0
    assert np.array_equal(llr, O.demod_soft(mod, d, "b" if llr8 else "s"))  # the demodulator against the oracle on the device's own symbols
    if symbols_out is not None:
        symbols_out.append(d)
    out = np.zeros_like(llr)
    (lib.srsran_sequence_pusch_apply_c if llr8 else lib.srsran_sequence_pusch_apply_s)(O.P(llr), O.P(out), rnti, 2 * (tti % 10), cell_id, llr.size)
    return out, avg_power(y)


def avg_power(y):
    return float(np.mean(np.abs(y.astype(np.complex128)) ** 2))


PUSCH_CASES = [
    # nof_prb, cp_nsymb, n_prb_tilde, L_prb, shortened, mod, tbs, snr_db, llr8
    (100, 7, (0, 0), 100, 0, 3, 75376, 29.0, False),  # configs[1]'s grant: 13 code blocks of 6144
    (100, 7, (10, 40), 50, 0, 3, 36696, 29.0, False),  # hopping between the slots
    (25, 7, (0, 0), 25, 1, 2, 6200, 17.0, False),  # SRS in the last symbol: 11 columns
    (6, 7, (1, 1), 4, 0, 1, 328, 8.0, False),  # one scalar-decoder block (K = 352)
    (50, 6, (3, 3), 45, 0, 2, 11448, 17.0, False),  # extended cyclic prefix: 10 columns
    (100, 7, (0, 0), 100, 0, 3, 75376, 29.0, True),  # 8-bit soft bits (what srsenb runs)
    (15, 7, (2, 5), 9, 0, 1, 1544, 11.0, True),
]


@pytest.mark.parametrize("case", PUSCH_CASES, ids=lambda c: "prb%d_L%d_mod%d_tbs%d%s" % (c[0], c[3], c[5], c[6], "_8bit" if c[8] else ""))
def test_pusch_grant_in_one_call(hiplib, case):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, snr_db, llr8 = case
    rng = np.random.default_rng(1000 + tbs + L_prb)
    rnti, tti, cell_id, noise, iters = 0x46, 7, 211, 0.01, 8
    Qm = O.QM[mod]
    nsymb = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    nof_re = nsymb * 12 * L_prb
    dt = np.int8 if llr8 else np.int16
    seg = O.cbsegm(tbs)
    payload_bits = rng.integers(0, 2, tbs).astype(np.uint8)
    grid, ce, seed = _pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, rnti, tti, cell_id, snr_db, payload_bits)
    g = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, iters, 1 if llr8 else 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened,
                        noise, 1)
    sb, rows, keep, flags = _rx_softbuffer(capi, seg["C"] + 1, dt)
    data = np.zeros(tbs // 8 + 16, np.uint8)
    res = capi.HipGrantRes()
    assert lib.srsran_hip_pusch_decode(C.byref(g), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res)) == 0, capi.last_error()
    # ---- the same stages one call at a time + the oracle's de-interleaver and decode_tb
    q, epre = _per_stage_pusch_llrs(lib, capi, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, rnti, tti, cell_id, noise, llr8)
    lut = O.ulsch_interleaver_lut(nof_re, Qm, nsymb)
    e = np.zeros_like(q)
    e[lut] = q  # srsran_vec_lut_sis(q_bits, lut, g_bits, n): g[lut[i]] = q[i]
    soft = np.zeros((seg["C"], SB), dt)
    crc = np.zeros(seg["C"], np.uint8)
    ret, want, avg = O.sch_decode_tb(tbs, Qm, 0, e, soft, crc, iters)
    assert res.crc_ok == (1 if ret == 0 else 0)
    assert abs(res.avg_iterations_block - avg) < 1e-6
    assert abs(res.epre - epre) <= 1e-5 * epre
    if ret == 0:
        assert np.array_equal(data[:tbs // 8], want[:tbs // 8]) and np.array_equal(np.unpackbits(data[:tbs // 8]), payload_bits)
        assert sb.tb_crc and flags[:seg["C"]].all()
    assert ret == 0, "the case is meant to decode (snr %.1f dB)" % snr_db
    assert not data[tbs // 8 + 6:].any()  # nothing behind the block's last code block


def test_pusch_grant_harq_and_failure(hiplib):
    """a first transmission that cannot decode (the rows that come back are the oracle's combined soft bits), then rv 2 on the same soft buffer"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb, n_prb, L_prb, mod, tbs = 50, 7, (4, 4), 20, 2, 12960
    rnti, tti, cell_id, noise, iters = 0x51, 3, 17, 0.05, 6
    rng = np.random.default_rng(5)
    Qm, nsymb = O.QM[mod], 12
    nof_re = nsymb * 12 * L_prb
    seg = O.cbsegm(tbs)
    payload_bits = rng.integers(0, 2, tbs).astype(np.uint8)
    sb, rows, keep, flags = _rx_softbuffer(capi, seg["C"], np.int16)
    soft = np.zeros((seg["C"], SB), np.int16)
    crc = np.zeros(seg["C"], np.uint8)
    cb_data = np.zeros((seg["C"], 768), np.uint8)
    lut = O.ulsch_interleaver_lut(nof_re, Qm, nsymb)
    outcomes = []
    for rv, snr in ((0, 9.0), (2, 13.0), (3, 15.0)):
        grid, ce, seed = _pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, rv, rnti, tti, cell_id, snr, payload_bits)
        g = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, rv, nof_re, seed, iters, 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, 0, noise, 0)
        data = np.zeros(tbs // 8 + 16, np.uint8)
        res = capi.HipGrantRes()
        assert lib.srsran_hip_pusch_decode(C.byref(g), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res)) == 0, capi.last_error()
        q, _ = _per_stage_pusch_llrs(lib, capi, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, rnti, tti, cell_id, noise, False)
        e = np.zeros_like(q)
        e[lut] = q
        ret, want, avg = O.sch_decode_tb(tbs, Qm, rv, e, soft, crc, iters, cb_data=cb_data)
        assert res.crc_ok == (1 if ret == 0 else 0) and abs(res.avg_iterations_block - avg) < 1e-6, (rv, ret, res.crc_ok, avg, res.avg_iterations_block)
        assert np.isnan(res.epre)
        assert np.array_equal(flags[:seg["C"]].astype(np.uint8), crc)
        for i in range(seg["C"]):
            if not crc[i]:  # undecoded: the combined soft bits are the HARQ state
                K = seg["K1"] if i < seg["C1"] else seg["K2"]
                span = 3 * (K + 32) + 12
                assert np.array_equal(rows[i][:span], soft[i][:span]), (rv, i)
        if ret == 0:
            assert np.array_equal(np.unpackbits(data[:tbs // 8]), payload_bits)
        outcomes.append(ret)
        if ret == 0:
            break
    assert outcomes[0] != 0 and outcomes[-1] == 0, outcomes  # the draw does exercise a failure and a combining success


def test_pusch_grants_of_a_tti_in_one_call(hiplib):
    """srsran_hip_pusch_decode_multi: the grants of one TTI (different allocations, modulations, block sizes, one of them 8-bit) decoded in one call give
    what the single-grant call gives for each"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(99)
    nof_prb, cp_nsymb = 100, 7
    ues = [  # n_prb, L_prb, mod, tbs, snr, llr8
        ((0, 0), 25, 3, 18336, 29.0, False), ((25, 25), 25, 2, 6200, 17.0, False), ((50, 50), 30, 3, 21384, 29.0, False), ((80, 80), 4, 1, 328, 8.0, False),
        ((84, 84), 16, 2, 7992, 4.0, False),  # too noisy: fails in both
        ((0, 50), 50, 3, 36696, 29.0, True),
    ]
    n = len(ues)
    grants = (capi.HipPuschRx * n)()
    grids, ces, sbs, datas, single = [], [], [], [], []
    for i, (n_prb, L_prb, mod, tbs, snr, llr8) in enumerate(ues):
        nof_re = 12 * 12 * L_prb
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        grid, ce, seed = _pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, 0x100 + i, 4, 33, snr, bits)
        # (a noise estimate of its own per grant, one of them none at all -- zero forcing: the one equaliser launch of the call takes them per grant)
        grants[i] = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 8, 1 if llr8 else 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, 0,
                                    (0.01, 0.0, 0.02, 0.005, 0.3, 0.015)[i], 0)
        grids.append(grid)
        ces.append(ce)
        Cn = O.cbsegm(tbs)["C"]
        # the single-grant call first, on its own soft buffer
        sb1 = _rx_softbuffer(capi, Cn, np.int8 if llr8 else np.int16)
        d1 = np.zeros(tbs // 8 + 16, np.uint8)
        r1 = capi.HipGrantRes()
        assert lib.srsran_hip_pusch_decode(C.byref(grants[i]), O.P(grid), O.P(ce), C.byref(sb1[0]), O.P(d1), C.byref(r1)) == 0
        single.append((r1.crc_ok, r1.avg_iterations_block, d1, sb1))
        sbs.append(_rx_softbuffer(capi, Cn, np.int8 if llr8 else np.int16))
        datas.append(np.zeros(tbs // 8 + 16, np.uint8))
    res = (capi.HipGrantRes * n)()
    assert lib.srsran_hip_pusch_decode_multi(n, grants, (C.c_void_p * n)(*[a.ctypes.data for a in grids]), (C.c_void_p * n)(*[a.ctypes.data for a in ces]),
                                             (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]),
                                             (C.c_void_p * n)(*[a.ctypes.data for a in datas]), res) == 0, capi.last_error()
    oks = []
    for i in range(n):
        ok, avg, d1, sb1 = single[i]
        assert res[i].crc_ok == ok and abs(res[i].avg_iterations_block - avg) < 1e-6, i
        assert np.array_equal(datas[i], d1), i
        assert np.array_equal(sbs[i][3], sb1[3]), i
        for a, b in zip(sbs[i][1], sb1[1]):  # the rows of failed blocks, too
            assert np.array_equal(a, b), i
        oks.append(ok)
    assert oks == [1, 1, 1, 1, 0, 1], oks


@pytest.mark.parametrize("mod,tbs,nof_re,eq,llr8", [(3, 75376, 15000, True, False), (4, 31704, 5200, True, False), (2, 6200, 2400, False, False), (1, 328, 300, True, True),
                                                     (0, 104, 260, False, False)],
                         ids=["64qam_13cb_eq", "256qam_eq", "16qam_preequalised", "qpsk_small_8bit", "bpsk"])
def test_pdsch_codeword_in_one_call(hiplib, mod, tbs, nof_re, eq, llr8):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(tbs + nof_re)
    Qm = O.QM[mod]
    nbits = nof_re * Qm
    seg = O.cbsegm(tbs)
    rnti, tti, cell_id, iters, scaling, noise = 0x1234, 5, 301, 10, 0.8, 0.02
    seed = O.pdsch_seed(rnti, 0, 2 * (tti % 10), cell_id)
    payload_bits = rng.integers(0, 2, tbs).astype(np.uint8)
    e = _oracle_tx_bits(tbs, Qm, nbits, 0, payload_bits)
    x = O.modulate_bytes(mod, np.packbits(e), nbits, seed=seed, scramble=True, scaling=scaling if eq else 1.0)
    snr = {0: 6.0, 1: 9.0, 2: 17.0, 3: 28.0, 4: 34.0}[mod]
    sigma = 10 ** (-snr / 20) / np.sqrt(2)
    h = (0.9 + 0.1 * rng.standard_normal(nof_re) + 0.1j * rng.standard_normal(nof_re)).astype(np.complex64) if eq else np.ones(nof_re, np.complex64)
    y = (h * x + sigma * (rng.standard_normal(nof_re) + 1j * rng.standard_normal(nof_re))).astype(np.complex64)
    dt = np.int8 if llr8 else np.int16
    g = capi.HipPdschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, iters, 1 if llr8 else 0, 1), scaling, noise)
    sb, rows, keep, flags = _rx_softbuffer(capi, seg["C"], dt)
    data = np.zeros(tbs // 8 + 16, np.uint8)
    res = capi.HipGrantRes()
    assert lib.srsran_hip_pdsch_decode(C.byref(g), O.P(y), O.P(h) if eq else None, C.byref(sb), O.P(data), C.byref(res)) == 0, capi.last_error()
    # one call at a time
    d = y
    if eq:
        d = np.zeros(nof_re, np.complex64)
        assert lib.srsran_predecoding_single(O.P(y), O.P(h), O.P(d), None, nof_re, scaling, noise) == nof_re
    llr = np.zeros(nbits, dt)
    assert (lib.srsran_demod_soft_demodulate_b if llr8 else lib.srsran_demod_soft_demodulate_s)(mod, O.P(d), O.P(llr), nof_re) == 0
    llr = O.sequence_apply(llr, seed)
    soft = np.zeros((seg["C"], SB), dt)
    crc = np.zeros(seg["C"], np.uint8)
    ret, want, avg = O.sch_decode_tb(tbs, Qm, 0, llr, soft, crc, iters)
    assert ret == 0 and res.crc_ok == 1 and abs(res.avg_iterations_block - avg) < 1e-6
    assert np.array_equal(data[:tbs // 8], want[:tbs // 8]) and np.array_equal(np.unpackbits(data[:tbs // 8]), payload_bits)
    # ... and with the intermediate results the reference leaves in q->d / q->e handed back: the same verdict, the equalised symbols and soft bits of the stages
    sb, rows, keep, flags = _rx_softbuffer(capi, seg["C"], dt)
    d_out, e_out, data2 = np.full(nof_re + 4, 7, np.complex64), np.full(nbits + 8, 7, dt), np.zeros_like(data)
    assert lib.srsran_hip_pdsch_decode_dbg(C.byref(g), O.P(y), O.P(h) if eq else None, C.byref(sb), O.P(data2), C.byref(res), O.P(d_out), O.P(e_out)) == 0
    assert res.crc_ok == 1 and np.array_equal(data2, data) and np.array_equal(e_out[:nbits], llr) and np.all(e_out[nbits:] == 7)
    assert np.array_equal(d_out[:nof_re].view(np.uint32), d.view(np.uint32)) if eq else np.all(d_out == 7)  # without an equaliser the symbols are the input


def test_grant_entry_points_refuse_what_they_cannot_take(hiplib):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    sb, rows, keep, flags = _rx_softbuffer(capi, 13, np.int16)
    grid = np.zeros(14 * 1200, np.complex64)
    data = np.zeros(10000, np.uint8)
    res = capi.HipGrantRes()
    ok = capi.HipPuschRx(capi.HipGrantTb(2, 6200, 0, 12 * 12 * 25, 1, 8, 0, 1), 100, 7, (C.c_uint32 * 2)(0, 0), 25, 0, 0.0, 0)
    for field, val in (("L_prb", 7), ("L_prb", 0), ("cp_nsymb", 5), ("cell_nof_prb", 20)):
        bad = capi.HipPuschRx.from_buffer_copy(ok)
        setattr(bad, field, val)
        assert lib.srsran_hip_pusch_decode(C.byref(bad), O.P(grid), O.P(grid), C.byref(sb), O.P(data), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS, field
    for field, val in (("tbs", 0), ("tbs", 6201), ("rv", 4), ("mod", 4), ("mod", 0), ("nof_re", 100)):
        bad = capi.HipPuschRx.from_buffer_copy(ok)
        setattr(bad.tb, field, val)
        assert lib.srsran_hip_pusch_decode(C.byref(bad), O.P(grid), O.P(grid), C.byref(sb), O.P(data), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS, field
    assert lib.srsran_hip_pusch_decode(C.byref(ok), None, O.P(grid), C.byref(sb), O.P(data), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert lib.srsran_hip_pusch_decode_multi(0, None, None, None, None, None, None) == 0  # an empty TTI is a no-op


def test_modulator_against_the_reference_tables(hiplib):
    """srsran_hip_modulate_bytes against what the reference's srsran_mod_modulate_bytes produced (tests/golden/mod_ref.npz): every constellation point,
    seeded bits behind the packed scrambler, bit for bit as float32; a scaled case against the oracle"""
    import srslte_amd as S

    lib = S.lib()
    d = np.load(os.path.join(G, "mod_ref.npz"))
    for m in range(5):
        qm = O.QM[m]
        bits, sym = d["walk_bits_%d" % m], d["walk_sym_%d" % m]
        out = np.zeros(sym.size, np.complex64)
        assert lib.srsran_hip_modulate_bytes(m, O.P(bits), O.P(out), sym.size * qm, 0, 0, 1.0) == sym.size
        assert np.array_equal(out.view(np.uint32), sym.view(np.uint32)), m
        seed, nb = [int(v) for v in d["rand_seed_%d" % m]]
        raw, want = np.ascontiguousarray(d["rand_bits_%d" % m]), d["rand_sym_%d" % m]
        out = np.zeros(want.size, np.complex64)
        assert lib.srsran_hip_modulate_bytes(m, O.P(raw), O.P(out), nb, seed, 1, 1.0) == want.size
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), m
        assert lib.srsran_hip_modulate_bytes(m, O.P(raw), O.P(out), nb, seed, 1, 0.7071) == want.size
        assert np.array_equal(out.view(np.uint32), O.modulate_bytes(m, raw, nb, seed=seed, scramble=True, scaling=0.7071).view(np.uint32)), m
    assert lib.srsran_hip_modulate_bytes(3, O.P(raw), O.P(out), 7, 0, 0, 1.0) == -1  # not a multiple of Qm (mod.c:141-144)


@pytest.mark.parametrize("mod,tbs,nof_re,nl,scaling", [(3, 75376, 15000, 1, 1.0), (4, 97896, 14000, 1, 0.5), (2, 6200, 2400, 2, 1.0), (1, 328, 300, 1, 1.4142135), (1, 40, 120, 1, 1.0)],
                         ids=["64qam_13cb", "256qam_scaled", "16qam_two_layers", "qpsk_small", "qpsk_k40"])
def test_pdsch_codeword_encode_in_one_call(hiplib, mod, tbs, nof_re, nl, scaling):
    """payload -> constellation points in one call, equal to the oracle's chain (encode_tb restated + scrambling + the reference-pinned modulator), all
    redundancy versions; a retransmission from the soft buffer (data = NULL)"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(tbs)
    Qm = O.QM[mod]
    nbits = nof_re * Qm
    seed = O.pdsch_seed(0x77, 1, 8, 499)
    payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
    sb, rows = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
    for k, rv in enumerate((0, 2, 3, 1)):
        g = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, rv, nof_re, seed, 0, 0, nl), scaling)
        out = np.zeros(nof_re + 8, np.complex64)
        assert lib.srsran_hip_pdsch_encode(C.byref(g), C.byref(sb), O.P(payload) if k == 0 else None, O.P(out)) == 0, capi.last_error()
        e, _ = O.tb_coded_bits(tbs, Qm * nl, nbits, rv, None, payload=np.unpackbits(payload), tx_order=True)
        want = O.modulate_bytes(mod, np.packbits(e), nbits, seed=seed, scramble=True, scaling=scaling)
        assert np.array_equal(out[:nof_re].view(np.uint32), want.view(np.uint32)), rv
        assert not out[nof_re:].any()
        # the scrambled coded bits by themselves (q->e of the reference's object)
        out2, e_out = np.zeros(nof_re + 8, np.complex64), np.full(nbits // 8 + 9, 0xEE, np.uint8)
        assert lib.srsran_hip_pdsch_encode_dbg(C.byref(g), C.byref(sb), None, O.P(out2), O.P(e_out)) == 0, capi.last_error()
        assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))
        scr = e ^ O.sequence_bits(seed, nbits)
        assert np.array_equal(np.unpackbits(e_out)[:nbits], scr) and np.all(e_out[(nbits + 7) // 8:] == 0xEE), rv


def test_pdsch_codewords_of_a_tti_in_one_call(hiplib):
    """srsran_hip_pdsch_encode_multi: the codewords of one TTI (different modulations, sizes, redundancy versions, power scalings, two layers; one of them a
    retransmission from its soft buffer) in one call give the oracle's chain for each -- and what the single call gives.  A second TTI has codewords of
    2044, 2048 and 2052 symbols around the 2048 of a workgroup: one short of full, exactly full (so the next codeword's first workgroup follows a full
    one: a wrong tile0 shows in it) and four symbols into a second workgroup.  Every output has a sentinel behind it."""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(2024)
    ttis = [  # (mod, tbs, nof_re, nl, scaling, rv) per codeword; the codeword that is a retransmission
        ([(3, 36696, 7200, 1, 1.0, 0), (2, 6200, 2400, 2, 1.0, 2), (1, 328, 300, 1, 1.4142135, 0), (4, 31704, 5200, 1, 0.5, 3), (1, 40, 120, 1, 1.0, 1),
          (3, 18336, 3600, 1, 1.0, 0)], 3),
        ([(1, 328, 2044, 1, 1.0, 0), (1, 328, 2048, 1, 1.0, 0), (1, 328, 2052, 1, 1.0, 0)], None),
    ]
    sentinel = np.complex64(7 - 7j)
    for ues, retx in ttis:
        n = len(ues)
        grants = (capi.HipPdschTx * n)()
        sbs, pays, outs, wants = [], [], [], []
        for i, (mod, tbs, nof_re, nl, scaling, rv) in enumerate(ues):
            Qm, nbits = O.QM[mod], nof_re * O.QM[mod]
            seed = O.pdsch_seed(0x50 + i, 0, 6, 401)
            payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
            grants[i] = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, rv, nof_re, seed, 0, 0, nl), scaling)
            sb = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
            if i == retx:  # a retransmission: the first transmission (rv 0) left the payload in the soft buffer
                g0 = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 0, 0, nl), scaling)
                tmp = np.zeros(nof_re, np.complex64)
                assert lib.srsran_hip_pdsch_encode(C.byref(g0), C.byref(sb[0]), O.P(payload), O.P(tmp)) == 0
            e, _ = O.tb_coded_bits(tbs, Qm * nl, nbits, rv, None, payload=np.unpackbits(payload), tx_order=True)
            wants.append(O.modulate_bytes(mod, np.packbits(e), nbits, seed=seed, scramble=True, scaling=scaling))
            sbs.append(sb)
            pays.append(payload)
            outs.append(np.full(nof_re + 8, sentinel, np.complex64))
        data = (C.c_void_p * n)(*[None if i == retx else pays[i].ctypes.data for i in range(n)])
        assert lib.srsran_hip_pdsch_encode_multi(n, grants, (C.POINTER(capi.SoftbufferTx) * n)(*[C.pointer(s[0]) for s in sbs]), data,
                                                 (C.c_void_p * n)(*[o.ctypes.data for o in outs])) == 0, capi.last_error()
        for i, (mod, tbs, nof_re, nl, scaling, rv) in enumerate(ues):
            assert np.array_equal(outs[i][:nof_re].view(np.uint32), wants[i].view(np.uint32)), i
            assert np.all(outs[i][nof_re:] == sentinel), i
            single = np.zeros(nof_re, np.complex64)
            assert lib.srsran_hip_pdsch_encode(C.byref(grants[i]), C.byref(sbs[i][0]), None, O.P(single)) == 0  # (from the soft buffer the multi call filled)
            assert np.array_equal(single.view(np.uint32), outs[i][:nof_re].view(np.uint32)), i
    assert lib.srsran_hip_pdsch_encode_multi(0, None, None, None, None) == 0


@pytest.mark.parametrize("mod,tbs,L_prb,nsymb", [(3, 75376, 100, 12), (2, 6200, 25, 11), (1, 328, 4, 12), (2, 11448, 45, 10)], ids=["64qam_100prb", "16qam_srs", "qpsk", "ext_cp"])
def test_ulsch_encode_in_one_call(hiplib, mod, tbs, L_prb, nsymb):
    """UE transmit side without UCI: encode_tb + the channel interleaver on the device = the oracle's e bits read through the oracle's table"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(tbs + 1)
    Qm = O.QM[mod]
    nof_re = nsymb * 12 * L_prb
    payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
    sb, rows = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
    lut = O.ulsch_interleaver_lut(nof_re, Qm, nsymb)
    for k, rv in enumerate((0, 2)):
        tb = capi.HipGrantTb(mod, tbs, rv, nof_re, 0, 0, 0, 1)
        q = np.full(nof_re * Qm // 8 + 8, 0xFF, np.uint8)
        assert lib.srsran_hip_ulsch_encode(C.byref(tb), nsymb, C.byref(sb), O.P(payload) if k == 0 else None, O.P(q)) == 0, capi.last_error()
        g, _ = O.tb_coded_bits(tbs, Qm, nof_re * Qm, rv, None, payload=np.unpackbits(payload), tx_order=True)
        assert np.array_equal(np.unpackbits(q[:nof_re * Qm // 8]), g[lut]), rv
        assert np.all(q[nof_re * Qm // 8:] == 0xFF)


def test_multi_grant_calls_from_worker_threads(hiplib):
    """three worker threads at once, each decoding its own TTI's grants in one srsran_hip_pusch_decode_multi and encoding its own codewords in one
    srsran_hip_pdsch_encode_multi, 20 rounds: every call of every thread gives what the single calls gave (staging contexts, job lists in the pinned
    images and the two-wave / scalar latency kernels are per thread or re-entrant; the reference runs one PHY worker thread per subframe in flight)"""
    import threading

    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb = 100, 7

    def worker(tid, errors):
        try:
            rng = np.random.default_rng(500 + tid)
            ues = [((0, 0), 25, 3, 18336, 29.0), ((25, 25), (12, 15, 16)[tid], 2, 5480, 17.0), ((50, 50), 4, 1, 328, 8.0), ((60, 60), 30, 3, 21384, 29.0)]
            n = len(ues)
            grants = (capi.HipPuschRx * n)()
            grids, ces, want = [], [], []
            for i, (n_prb, L_prb, mod, tbs, snr) in enumerate(ues):
                nof_re = 12 * 12 * L_prb
                bits = rng.integers(0, 2, tbs).astype(np.uint8)
                grid, ce, seed = _pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, 0x300 + 16 * tid + i, 4, 33, snr, bits)
                grants[i] = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 8, 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, 0, 0.01, 0)
                grids.append(grid)
                ces.append(ce)
                want.append(np.packbits(bits))
            cws = [(3, 18336, 3600, 0), (2, 5736, 1584, 2), (1, 328, 300, 0)]
            m = len(cws)
            tx = (capi.HipPdschTx * m)()
            sbt, pays, single = [], [], []
            for i, (mod, tbs, nof_re, rv) in enumerate(cws):
                tx[i] = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, rv, nof_re, 0x4000 + 64 * tid + i, 0, 0, 1), 1.0)
                sbt.append(_tx_softbuffer(capi, O.cbsegm(tbs)["C"]))
                pays.append(rng.integers(0, 256, tbs // 8).astype(np.uint8))
                o = np.zeros(nof_re, np.complex64)
                assert lib.srsran_hip_pdsch_encode(C.byref(tx[i]), C.byref(sbt[i][0]), O.P(pays[i]), O.P(o)) == 0
                single.append(o)
            for rnd in range(20):
                sbs = [_rx_softbuffer(capi, O.cbsegm(u[3])["C"], np.int16) for u in ues]
                datas = [np.zeros(u[3] // 8 + 16, np.uint8) for u in ues]
                res = (capi.HipGrantRes * n)()
                assert lib.srsran_hip_pusch_decode_multi(n, grants, (C.c_void_p * n)(*[a.ctypes.data for a in grids]), (C.c_void_p * n)(*[a.ctypes.data for a in ces]),
                                                         (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]),
                                                         (C.c_void_p * n)(*[a.ctypes.data for a in datas]), res) == 0, capi.last_error()
                for i, u in enumerate(ues):
                    assert res[i].crc_ok == 1 and np.array_equal(datas[i][:u[3] // 8], want[i]), (tid, rnd, i)
                outs = [np.zeros(c[2], np.complex64) for c in cws]
                assert lib.srsran_hip_pdsch_encode_multi(m, tx, (C.POINTER(capi.SoftbufferTx) * m)(*[C.pointer(s[0]) for s in sbt]),
                                                         (C.c_void_p * m)(*[p.ctypes.data for p in pays]), (C.c_void_p * m)(*[o.ctypes.data for o in outs])) == 0
                for i in range(m):
                    assert np.array_equal(outs[i].view(np.uint32), single[i].view(np.uint32)), (tid, rnd, i)
        except BaseException as e:  # noqa: B902 -- carried to the main thread
            errors.append((tid, repr(e)))

    errors = []
    ths = [threading.Thread(target=worker, args=(t, errors)) for t in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
