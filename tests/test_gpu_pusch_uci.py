"""PUSCH grants that carry control information in one device call: srsran_hip_pusch_decode_uci{,_multi} (include/srsran_amd/phy_chan_abi.h).

The transmit side is numpy on top of the oracle: the transport block's coded bits for G Qm bits, random bits as the CQI code word in front, written row
by row around the RI positions, the ACK positions overwritten (TS 36.212 5.2.2.8), scrambled and modulated by the oracle, transform precoding, a
frequency-selective channel and noise as tests/test_gpu_chan.py does.  The expected side is the per-stage soft bits (the reference-named entry points one
call at a time, each held to the oracle) pushed through a LITERAL restatement of the reference's de-multiplexer -- the table of ulsch_interleave_gen
(sch.c:660-681) with zeros at the RI positions, applied in index order like srsran_vec_lut_sis, the positions of uci.c:364-416 -- and the oracle's
decode_tb.  The kernel itself uses a closed form; nothing of it is used here.  Last, the reference's own pusch_test judges the binding of
tests/ref_link/uci_bind.c: payload, ACK bits and validity, RI and CQI against what the program sent."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import oracle_api as O
import test_gpu_chan as T
from ref_link_common import add_ctest_data, make_data_dir, run_program

pytestmark = pytest.mark.gpu
SB = T.SB
ACK_COLS = {True: (2, 3, 8, 9), False: (1, 2, 6, 7)}
RI_COLS = {True: (1, 4, 7, 10), False: (0, 3, 5, 8)}


# ---- literal restatements of the reference -------------------------------------------------------------------------------------------------------------

def _positions(n, Qm, H, cols, sets):
    """uci.c:364-416: the Qm positions of ACK / RI symbol n in q_bits"""
    rows = H // cols
    assert rows >= 1 + n // 4
    row = rows - 1 - n // 4
    col = sets[cols > 10][(3 * n) % 4]
    return [row * Qm + rows * col * Qm + k for k in range(Qm)]


def _interleave_gen(H, cols, Qm, ri_present):
    """sch.c:660-681 ulsch_interleave_gen: the table, 0 at the RI positions"""
    rows = H // cols
    lut = np.zeros(H * Qm, np.int64)
    idx = 0
    for j in range(rows):
        for i in range(cols):
            for k in range(Qm):
                p = j * Qm + i * rows * Qm + k
                if ri_present[p]:
                    lut[p] = 0
                else:
                    lut[p] = idx
                    idx += 1
    return lut


def _literal_demux(q, H, cols, Qm, Qa, Qr, Qc):
    """sch.c:1022-1119 + 993-1020 on the descrambled soft bits q: (ack soft bits, ack positions, ri soft bits, ri positions, cqi soft bits, e bits of the
    transport block, g)"""
    q = q.copy()
    ackp = [p for n in range(Qa) for p in _positions(n, Qm, H, cols, ACK_COLS)]
    ack = q[ackp].copy() if ackp else np.zeros(0, q.dtype)
    q[ackp] = 0  # sch.c:1077-1080
    rip = [p for n in range(Qr) for p in _positions(n, Qm, H, cols, RI_COLS)]
    ri = q[rip].copy() if rip else np.zeros(0, q.dtype)
    present = np.zeros(H * Qm, bool)
    present[rip] = True
    lut = _interleave_gen(H, cols, Qm, present)
    g = np.zeros(H * Qm, q.dtype)
    for i in range(H * Qm):  # srsran_vec_lut_sis, vector.c:141-146: in order, a later write to the same index wins
        g[lut[i]] = q[i]
    return ack, np.array(ackp, np.uint32), ri, np.array(rip, np.uint32), g[:Qc * Qm].copy(), np.ascontiguousarray(g[Qc * Qm:(H - Qr) * Qm]), g


# ---- transmit side ---------------------------------------------------------------------------------------------------------------------------------------

def _uci_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, rv, rnti, tti, cell_id, snr_db, payload_bits, Qa, Qr, Qc):
    """the grid a UE's PUSCH with control information leaves at the eNB: (grid, ce, seed)"""
    Qm = O.QM[mod]
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    G = cols * 12 * L_prb - Qr - Qc
    e = T._oracle_tx_bits(tbs, Qm, G * Qm, rv, payload_bits)
    return _uci_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, e, rnti, tti, cell_id, snr_db, Qa, Qr, Qc)


def _uci_mux(rng, e, H, cols, Qm, Qa, Qr, Qc):
    """TS 36.212 5.2.2.8 on bits: e (uint8 [(H - Qr - Qc) Qm], the transport block's part of the data stream -- a code word or anything else) behind a random
    CQI code word, written row by row around the RI positions, random RI bits, the ACK positions overwritten with random bits: q (uint8 [H Qm])"""
    rows = H // cols
    assert e.size == (H - Qr - Qc) * Qm
    g = np.concatenate([rng.integers(0, 2, Qc * Qm).astype(np.uint8), e])
    rip = [p for n in range(Qr) for p in _positions(n, Qm, H, cols, RI_COLS)]
    ackp = [p for n in range(Qa) for p in _positions(n, Qm, H, cols, ACK_COLS)]
    present = np.zeros(H * Qm, bool)
    present[rip] = True
    # row by row around the RI positions: position p = j Qm + i rows Qm + k in the order (j, i, k)
    j, i, k = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(Qm), indexing="ij")
    order = (j * Qm + i * rows * Qm + k).reshape(-1)
    order = order[~present[order]]
    assert order.size == g.size
    q = np.zeros(H * Qm, np.uint8)
    q[order] = g
    q[rip] = rng.integers(0, 2, len(rip))
    q[ackp] = rng.integers(0, 2, len(ackp))
    return q


def _uci_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, e, rnti, tti, cell_id, snr_db, Qa, Qr, Qc):
    """the "bits -> grid" half: e multiplexed with control information (_uci_mux), then the signal path of tests/test_gpu_chan.py: (grid, ce, seed)"""
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    q = _uci_mux(rng, e, cols * 12 * L_prb, cols, O.QM[mod], Qa, Qr, Qc)
    return T._pusch_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, q, rnti, tti, cell_id, snr_db)


class _UciOut:
    """caller's memory for the control soft bits of one grant, with guard entries behind every array"""

    def __init__(self, capi, Qm, Qa, Qr, Qc, pad=4):
        self.n = (Qa * Qm, Qr * Qm, Qc * Qm)
        self.ack_llr = np.full(Qa * Qm + pad, 0x7777, np.int16)
        self.ack_c = np.full(Qa * Qm + pad, 0x77, np.uint8)
        self.ack_pos = np.full(Qa * Qm + pad, 0x77777777, np.uint32)
        self.ri_llr = np.full(Qr * Qm + pad, 0x7777, np.int16)
        self.ri_c = np.full(Qr * Qm + pad, 0x77, np.uint8)
        self.ri_pos = np.full(Qr * Qm + pad, 0x77777777, np.uint32)
        self.cqi_llr = np.full(Qc * Qm + pad, 0x7777, np.int16)
        self.c = capi.HipPuschUciOut(*[a.ctypes.data for a in (self.ack_llr, self.ack_c, self.ack_pos, self.ri_llr, self.ri_c, self.ri_pos, self.cqi_llr)])

    def arrays(self):
        na, nr, nc = self.n
        return (self.ack_llr[:na], self.ack_c[:na], self.ack_pos[:na], self.ri_llr[:nr], self.ri_c[:nr], self.ri_pos[:nr], self.cqi_llr[:nc])

    def guards_intact(self):
        na, nr, nc = self.n
        return (np.all(self.ack_llr[na:] == 0x7777) and np.all(self.ack_c[na:] == 0x77) and np.all(self.ack_pos[na:] == 0x77777777) and
                np.all(self.ri_llr[nr:] == 0x7777) and np.all(self.ri_c[nr:] == 0x77) and np.all(self.ri_pos[nr:] == 0x77777777) and np.all(self.cqi_llr[nc:] == 0x7777))


def _grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, rv, seed, iters, noise, llr8=False, epre=0):
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    return capi.HipPuschRx(capi.HipGrantTb(mod, tbs, rv, cols * 12 * L_prb, seed, iters, 1 if llr8 else 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb,
                           shortened, noise, epre)


# ---- 1. parity with the oracle's chain -----------------------------------------------------------------------------------------------------------------------

UCI_COUNTS = [(40, 0, 0), (0, 1, 0), (0, 7, 0), (0, 0, 60), (24, 5, 60)]


def _parity_cases():
    out = []
    for case in T.PUSCH_CASES:
        if case[8]:
            continue  # 16-bit soft bits only
        rows = 12 * case[3]
        for Qa, Qr, Qc in UCI_COUNTS:
            out.append(case[:8] + (min(Qa, 4 * rows), Qr, min(Qc, rows)))
    # at the cap Q'ack = Q'ri = 4 * 12 * L_prb: 8 of 12 columns are gone, which needs a low code rate
    out.append((6, 7, (1, 1), 4, 0, 1, 104, 8.0, 4 * 48, 4 * 48, 10))
    out.append((25, 7, (0, 0), 25, 0, 2, 2216, 17.0, 4 * 300, 4 * 300, 40))
    # one RI symbol in front of a CQI code word: g[0] is visible as cqi_llr[0]
    out.append((25, 7, (0, 0), 25, 1, 2, 6200, 17.0, 8, 1, 20))
    return out


def _case_id(c):
    return "prb%d_L%d_cp%d%s_mod%d_tbs%d_ack%d_ri%d_cqi%d" % (c[0], c[3], c[1], "_srs" if c[4] else "", c[5], c[6], c[8], c[9], c[10])


@pytest.mark.parametrize("case", _parity_cases(), ids=_case_id)
def test_pusch_uci_grant_against_the_oracle_chain(hiplib, case):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, snr_db, Qa, Qr, Qc = case
    rng = np.random.default_rng(7000 + tbs + L_prb + 13 * Qa + 101 * Qr + 7 * Qc)
    rnti, tti, cell_id, noise, iters = 0x46, 7, 211, 0.01, 8
    Qm = O.QM[mod]
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    H = cols * 12 * L_prb
    seg = O.cbsegm(tbs)
    payload_bits = rng.integers(0, 2, tbs).astype(np.uint8)
    grid, ce, seed = _uci_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, rnti, tti, cell_id, snr_db, payload_bits, Qa, Qr, Qc)
    g = _grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, seed, iters, noise, epre=1)
    uci = capi.HipPuschUci(Qa, Qr, Qc)
    out = _UciOut(capi, Qm, Qa, Qr, Qc)
    sb, rows_, keep, flags = T._rx_softbuffer(capi, seg["C"] + 1, np.int16)
    data = np.zeros(tbs // 8 + 16, np.uint8)
    res = capi.HipGrantRes()
    assert lib.srsran_hip_pusch_decode_uci(C.byref(g), C.byref(uci), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res), C.byref(out.c)) == 0, capi.last_error()
    # ---- the same stages one call at a time, the literal de-multiplexer, the oracle's decode_tb
    q, epre = T._per_stage_pusch_llrs(lib, capi, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, rnti, tti, cell_id, noise, False)
    ack, ackp, ri, rip, cqi, e, gbits = _literal_demux(q, H, cols, Qm, Qa, Qr, Qc)
    chips = O.sequence_bits(seed, H * Qm)
    ack_llr, ack_c, ack_pos, ri_llr, ri_c, ri_pos, cqi_llr = out.arrays()
    assert np.array_equal(ack_pos, ackp) and np.array_equal(ri_pos, rip)
    assert np.array_equal(ack_llr, ack) and np.array_equal(ack_c, chips[ackp] if Qa else chips[:0])
    assert np.array_equal(ri_llr, ri) and np.array_equal(ri_c, chips[rip] if Qr else chips[:0])
    assert np.array_equal(cqi_llr, cqi)
    assert out.guards_intact()
    if Qr > 0 and Qc > 0:
        # g[0]: the reference's table holds 0 at every RI position and the in-order loop leaves the soft bit of the highest one there
        n_last = 1 if Qr >= 2 else 0
        assert cqi_llr[0] == q[_positions(n_last, Qm, H, cols, RI_COLS)[-1]] == gbits[0]
    soft = np.zeros((seg["C"], SB), np.int16)
    crc = np.zeros(seg["C"], np.uint8)
    ret, want, avg = O.sch_decode_tb(tbs, Qm, 0, e, soft, crc, iters)
    assert res.crc_ok == (1 if ret == 0 else 0)
    assert abs(res.avg_iterations_block - avg) < 1e-6
    assert abs(res.epre - epre) <= 1e-5 * epre
    assert np.array_equal(flags[:seg["C"]].astype(np.uint8), crc)
    if ret == 0:
        assert np.array_equal(data[:tbs // 8], want[:tbs // 8]) and np.array_equal(np.unpackbits(data[:tbs // 8]), payload_bits)
        assert sb.tb_crc and flags[:seg["C"]].all()
    assert ret == 0, "the case is meant to decode (snr %.1f dB)" % snr_db
    assert not data[tbs // 8 + 6:].any()


# ---- 2. no control information: the plain call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [T.PUSCH_CASES[2], T.PUSCH_CASES[3], T.PUSCH_CASES[6]], ids=["16qam_srs", "qpsk", "qpsk_8bit"])
def test_all_counts_zero_is_the_plain_call(hiplib, case):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, snr_db, llr8 = case
    rng = np.random.default_rng(31 + tbs)
    dt = np.int8 if llr8 else np.int16
    bits = rng.integers(0, 2, tbs).astype(np.uint8)
    grid, ce, seed = T._pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, 0x46, 7, 211, snr_db, bits)
    g = _grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, seed, 8, 0.01, llr8=llr8, epre=1)
    Cn = O.cbsegm(tbs)["C"]
    got = []
    for with_uci in (False, True):
        sb, rows_, keep, flags = T._rx_softbuffer(capi, Cn, dt)
        data = np.zeros(tbs // 8 + 16, np.uint8)
        res = capi.HipGrantRes()
        if with_uci:
            uci = capi.HipPuschUci(0, 0, 0)
            assert lib.srsran_hip_pusch_decode_uci(C.byref(g), C.byref(uci), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res), None) == 0, capi.last_error()
        else:
            assert lib.srsran_hip_pusch_decode(C.byref(g), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res)) == 0, capi.last_error()
        got.append((res.crc_ok, res.avg_iterations_block, res.epre, data, flags.copy()))
    a, b = got
    assert a[0] == b[0] == 1 and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert np.array_equal(np.unpackbits(b[3][:tbs // 8]), bits)


# ---- 3. HARQ ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_pusch_uci_harq_with_other_counts_in_the_retransmission(hiplib):
    """a first transmission with control information that cannot decode, then rv 2 with OTHER counts on the same soft buffer: the rows that come back are
    the oracle's combined soft bits"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    nof_prb, cp_nsymb, n_prb, L_prb, mod, tbs = 50, 7, (4, 4), 20, 2, 12960
    rnti, tti, cell_id, noise, iters = 0x51, 3, 17, 0.05, 6
    rng = np.random.default_rng(5)
    Qm, cols = O.QM[mod], 12
    H = cols * 12 * L_prb
    seg = O.cbsegm(tbs)
    payload_bits = rng.integers(0, 2, tbs).astype(np.uint8)
    sb, rows, keep, flags = T._rx_softbuffer(capi, seg["C"], np.int16)
    soft = np.zeros((seg["C"], SB), np.int16)
    crc = np.zeros(seg["C"], np.uint8)
    cb_data = np.zeros((seg["C"], 768), np.uint8)
    outcomes = []
    for rv, snr, (Qa, Qr, Qc) in ((0, 9.0, (30, 6, 44)), (2, 13.0, (12, 0, 25)), (3, 15.0, (0, 3, 0))):
        grid, ce, seed = _uci_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, rv, rnti, tti, cell_id, snr, payload_bits, Qa, Qr, Qc)
        g = _grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, rv, seed, iters, noise)
        uci = capi.HipPuschUci(Qa, Qr, Qc)
        out = _UciOut(capi, Qm, Qa, Qr, Qc)
        data = np.zeros(tbs // 8 + 16, np.uint8)
        res = capi.HipGrantRes()
        assert lib.srsran_hip_pusch_decode_uci(C.byref(g), C.byref(uci), O.P(grid), O.P(ce), C.byref(sb), O.P(data), C.byref(res), C.byref(out.c)) == 0, capi.last_error()
        q, _ = T._per_stage_pusch_llrs(lib, capi, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, rnti, tti, cell_id, noise, False)
        ack, ackp, ri, rip, cqi, e, _g = _literal_demux(q, H, cols, Qm, Qa, Qr, Qc)
        got = out.arrays()
        assert np.array_equal(got[0], ack) and np.array_equal(got[3], ri) and np.array_equal(got[6], cqi), rv
        ret, want, avg = O.sch_decode_tb(tbs, Qm, rv, e, soft, crc, iters, cb_data=cb_data)
        assert res.crc_ok == (1 if ret == 0 else 0) and abs(res.avg_iterations_block - avg) < 1e-6, (rv, ret, res.crc_ok, avg, res.avg_iterations_block)
        assert np.isnan(res.epre)
        assert np.array_equal(flags[:seg["C"]].astype(np.uint8), crc)
        for i in range(seg["C"]):
            if not crc[i]:
                K = seg["K1"] if i < seg["C1"] else seg["K2"]
                span = 3 * (K + 32) + 12
                assert np.array_equal(rows[i][:span], soft[i][:span]), (rv, i)
        if ret == 0:
            assert np.array_equal(np.unpackbits(data[:tbs // 8]), payload_bits)
        outcomes.append(ret)
        if ret == 0:
            break
    assert outcomes[0] != 0 and outcomes[-1] == 0, outcomes


# ---- 4. the grants of a TTI ------------------------------------------------------------------------------------------------------------------------------------

TTI_UES = [  # n_prb, L_prb, mod, tbs, snr, llr8, (Q'ack, Q'ri, Q'cqi)
    ((0, 0), 25, 3, 18336, 29.0, False, (24, 5, 60)), ((25, 25), 25, 2, 6200, 17.0, False, (0, 0, 0)), ((50, 50), 30, 3, 21384, 29.0, False, (0, 1, 33)),
    ((80, 80), 4, 1, 328, 8.0, False, (40, 0, 0)), ((84, 84), 16, 2, 7992, 4.0, False, (10, 2, 20)),  # too noisy: fails in both
    ((0, 50), 50, 3, 36696, 29.0, True, (0, 0, 0)), ((10, 10), 12, 2, 2600, 17.0, False, (0, 0, 48)),
]


def _tti(capi, rng, ues, rnti0):
    """grants, signals and the single-call results of one TTI"""
    import srslte_amd as S

    lib = S.lib()
    nof_prb, cp_nsymb = 100, 7
    n = len(ues)
    grants, ucis = (capi.HipPuschRx * n)(), (capi.HipPuschUci * n)()
    grids, ces, single = [], [], []
    for i, (n_prb, L_prb, mod, tbs, snr, llr8, (Qa, Qr, Qc)) in enumerate(ues):
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        grid, ce, seed = _uci_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, rnti0 + i, 4, 33, snr, bits, Qa, Qr, Qc)
        grants[i] = _grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, seed, 8, (0.01, 0.0, 0.02, 0.005, 0.3, 0.015, 0.01)[i % 7], llr8=llr8)
        ucis[i] = capi.HipPuschUci(Qa, Qr, Qc)
        grids.append(grid)
        ces.append(ce)
        Cn = O.cbsegm(tbs)["C"]
        sb1 = T._rx_softbuffer(capi, Cn, np.int8 if llr8 else np.int16)
        d1 = np.zeros(tbs // 8 + 16, np.uint8)
        r1 = capi.HipGrantRes()
        o1 = _UciOut(capi, O.QM[mod], Qa, Qr, Qc)
        assert lib.srsran_hip_pusch_decode_uci(C.byref(grants[i]), C.byref(ucis[i]), O.P(grid), O.P(ce), C.byref(sb1[0]), O.P(d1), C.byref(r1), C.byref(o1.c)) == 0
        single.append((r1.crc_ok, r1.avg_iterations_block, d1, sb1, o1))
    return grants, ucis, grids, ces, single


def _run_tti(capi, lib, ues, grants, ucis, grids, ces):
    n = len(ues)
    sbs = [T._rx_softbuffer(capi, O.cbsegm(u[3])["C"], np.int8 if u[5] else np.int16) for u in ues]
    datas = [np.zeros(u[3] // 8 + 16, np.uint8) for u in ues]
    outs = [_UciOut(capi, O.QM[u[2]], *u[6]) for u in ues]
    oc = (capi.HipPuschUciOut * n)(*[o.c for o in outs])
    res = (capi.HipGrantRes * n)()
    assert lib.srsran_hip_pusch_decode_uci_multi(n, grants, ucis, (C.c_void_p * n)(*[a.ctypes.data for a in grids]), (C.c_void_p * n)(*[a.ctypes.data for a in ces]),
                                                 (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]), (C.c_void_p * n)(*[a.ctypes.data for a in datas]),
                                                 res, oc) == 0, capi.last_error()
    return sbs, datas, outs, res


def _same_as_single(ues, single, sbs, datas, outs, res):
    oks = []
    for i in range(len(ues)):
        ok, avg, d1, sb1, o1 = single[i]
        assert res[i].crc_ok == ok and abs(res[i].avg_iterations_block - avg) < 1e-6, i
        assert np.array_equal(datas[i], d1), i
        assert np.array_equal(sbs[i][3], sb1[3]), i
        for a, b in zip(sbs[i][1], sb1[1]):  # the rows of failed blocks, too
            assert np.array_equal(a, b), i
        for a, b in zip(outs[i].arrays(), o1.arrays()):
            assert np.array_equal(a, b), i
        assert outs[i].guards_intact(), i
        oks.append(ok)
    return oks


def test_pusch_uci_grants_of_a_tti_in_one_call(hiplib):
    """srsran_hip_pusch_decode_uci_multi: seven grants of one TTI, with and without control information, different allocations and modulations, one of them
    8-bit, decoded in one call give what the single call gives for each -- every output"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(99)
    grants, ucis, grids, ces, single = _tti(capi, rng, TTI_UES, 0x100)
    sbs, datas, outs, res = _run_tti(capi, lib, TTI_UES, grants, ucis, grids, ces)
    assert _same_as_single(TTI_UES, single, sbs, datas, outs, res) == [1, 1, 1, 1, 0, 1, 1]
    assert lib.srsran_hip_pusch_decode_uci_multi(0, None, None, None, None, None, None, None, None) == 0  # an empty TTI is a no-op


def test_pusch_uci_multi_from_worker_threads(hiplib):
    """three worker threads at once, each decoding its own TTI's grants (with and without control information) in one call, 10 rounds"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()

    def worker(tid, errors):
        try:
            rng = np.random.default_rng(700 + tid)
            ues = [((0, 0), 25, 3, 18336, 29.0, False, (24, 5, 60)), ((25, 25), (12, 15, 16)[tid], 2, 5480, 17.0, False, (0, 0, 0)),
                   ((50, 50), 4, 1, 328, 8.0, False, (8 + tid, 1, 0)), ((60, 60), 30, 3, 21384, 29.0, False, (0, 3 + tid, 33))]
            grants, ucis, grids, ces, single = _tti(capi, rng, ues, 0x300 + 16 * tid)
            for rnd in range(10):
                sbs, datas, outs, res = _run_tti(capi, lib, ues, grants, ucis, grids, ces)
                assert _same_as_single(ues, single, sbs, datas, outs, res) == [1, 1, 1, 1], (tid, rnd)
        except BaseException as e:  # noqa: B902 -- carried to the main thread
            errors.append((tid, repr(e)))

    errors = []
    ths = [threading.Thread(target=worker, args=(t, errors)) for t in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------------------

def test_pusch_uci_refuses_what_it_cannot_take(hiplib):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    L_prb, mod, tbs = 25, 2, 6200
    Qm = O.QM[mod]
    grid = np.zeros(14 * 1200, np.complex64)

    def call(g, uci, out, n_sb=2):
        sb, rows, keep, flags = T._rx_softbuffer(capi, n_sb, np.int16)
        for r in rows:
            r[:] = 123
        data = np.full(tbs // 8 + 16, 0xA5, np.uint8)
        res = capi.HipGrantRes(7, 7.0, 7.0)
        rc = lib.srsran_hip_pusch_decode_uci(C.byref(g), C.byref(uci), O.P(grid), O.P(grid), C.byref(sb), O.P(data), C.byref(res), C.byref(out.c) if out else None)
        untouched = all(np.all(r == 123) for r in rows) and np.all(data == 0xA5) and not flags.any() and not sb.tb_crc
        return rc, untouched, res

    ok = _grant(capi, 100, 7, (0, 0), L_prb, 0, mod, tbs, 0, 1, 8, 0.0)
    bit8 = _grant(capi, 100, 7, (0, 0), L_prb, 0, mod, tbs, 0, 1, 8, 0.0, llr8=True)
    cap = 4 * 12 * L_prb
    for g, counts, with_out, why in ((bit8, (4, 0, 0), True, "8-bit soft bits with control information"), (ok, (cap + 1, 0, 0), True, "Q'ack beyond the cap"),
                                     (ok, (0, cap + 1, 0), True, "Q'ri beyond the cap"), (ok, (0, 100, 12 * 12 * L_prb - 100), True, "nothing left for the block"),
                                     (ok, (4, 0, 0), False, "no output at all"), (ok, (0, 0, 9), None, "no CQI output")):
        out = _UciOut(capi, Qm, *[min(c, cap) for c in counts]) if with_out is not False else None
        if with_out is None:
            out.c.cqi_llr = None
        rc, untouched, res = call(g, capi.HipPuschUci(*counts), out)
        assert rc == capi.SRSRAN_ERROR_INVALID_INPUTS, why
        assert untouched, why
        assert res.crc_ok == 0 and res.avg_iterations_block == 0.0 and np.isnan(res.epre), why  # every result is initialised before anything is checked
        assert "srsran_hip_pusch_decode_uci" in capi.last_error(), why
    # a bad grant in the middle of a TTI: every res[i] is initialised, those behind it too
    n = 3
    grants = (capi.HipPuschRx * n)(ok, ok, ok)
    ucis = (capi.HipPuschUci * n)(capi.HipPuschUci(0, 0, 0), capi.HipPuschUci(cap + 1, 0, 0), capi.HipPuschUci(0, 0, 0))
    outs = [_UciOut(capi, Qm, cap, 0, 0) for _ in range(n)]
    sbs = [T._rx_softbuffer(capi, 2, np.int16) for _ in range(n)]
    datas = [np.zeros(tbs // 8 + 16, np.uint8) for _ in range(n)]
    res = (capi.HipGrantRes * n)(*[capi.HipGrantRes(7, 7.0, 7.0) for _ in range(n)])
    assert lib.srsran_hip_pusch_decode_uci_multi(n, grants, ucis, (C.c_void_p * n)(*[grid.ctypes.data] * n), (C.c_void_p * n)(*[grid.ctypes.data] * n),
                                                 (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]), (C.c_void_p * n)(*[a.ctypes.data for a in datas]),
                                                 res, (capi.HipPuschUciOut * n)(*[o.c for o in outs])) == capi.SRSRAN_ERROR_INVALID_INPUTS
    for i in range(n):
        assert res[i].crc_ok == 0 and res[i].avg_iterations_block == 0.0 and np.isnan(res[i].epre), i
        assert not datas[i].any(), i


# ---- 6. the reference judges it ----------------------------------------------------------------------------------------------------------------------------------
# pusch_test compares payload, ACK bits and their validity, RI and CQI with what it sent and exits non-zero on any difference.  The three lines of the
# reference's own ctest list that carry control information, then lines of our own for what those do not reach: one ACK bit (the chip path of the 1-bit
# decoder), four (block code), RI alone and with ACK + CQI, low and high offset indices, a retransmission's redundancy version; 6, 25 and 100 PRB.
# Four subframes per line, ONE for the lines with -r: pusch_test.c:313-319 sets cfg.grant.tb.rv once and never back, so from its second subframe on the
# program's own transmitter encodes new data with rv != 0 first, and srsran_rm_turbo_tx_lut (rm_turbo.c:358) fills the circular buffer at rv 0 only: it
# sends what the reset soft buffer held and every link set, the reference's own objects included, reports "Unmatched data" there.

REF_LINES = [
    "-n 50 -L 50 -m 14 -p uci_ack 2 -p cqi wideband",
    "-n 100 -L 50 -m 21 -p uci_ack 2 -p cqi wideband",
    "-n 100 -L 50 -m 27 -p uci_ack 2 -p cqi wideband -p enable_64qam",
    "-n 6 -L 6 -m 10 -p uci_ack 1",
    "-n 25 -L 25 -m 14 -p uci_ack 1 -p cqi wideband",
    "-n 25 -L 25 -m 14 -p uci_ack 4",
    "-n 100 -L 100 -m 21 -p uci_ack 4 -p cqi wideband",
    "-n 6 -L 6 -m 10 -p ri 1",
    "-n 25 -L 25 -m 14 -p ri 1 -p uci_ack 2 -p cqi wideband",
    "-n 100 -L 50 -m 21 -p ri 1 -p uci_ack 1 -p cqi wideband",
    "-n 25 -L 25 -m 14 -p uci_ack 2 -p I_offset_ack 2",
    "-n 25 -L 25 -m 14 -p uci_ack 2 -p I_offset_ack 14",
    "-n 25 -L 25 -m 14 -p ri 1 -p I_offset_ri 0",
    "-n 25 -L 25 -m 14 -p ri 1 -p I_offset_ri 12",
    "-n 25 -L 25 -m 14 -p cqi wideband -p I_offset_cqi 2",
    "-n 25 -L 25 -m 14 -p cqi wideband -p I_offset_cqi 15",
    "-n 25 -L 25 -m 14 -r 2 -p uci_ack 2 -p cqi wideband",
    "-n 100 -L 100 -m 5 -r 2 -p ri 1 -p uci_ack 2 -p cqi wideband",
    "-n 6 -L 6 -m 5 -r 2 -p uci_ack 1",
]


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return add_ctest_data(make_data_dir(tmp_path_factory.mktemp("uci_ref")))


@pytest.mark.parametrize("line", REF_LINES, ids=lambda s: s.replace(" -", "_").replace(" ", "").lstrip("-"))
def test_reference_pusch_test_on_the_uci_binding(hiplib, line, data_dir):
    subframes = 1 if "-r" in line.split() else 4
    args = line.split() + ["-s", str(subframes)]
    os.environ["CHAN_BIND_REPORT"] = "1"
    try:
        rc, out = run_program("bin_uci", "pusch_test", args, data_dir, timeout=600)
    finally:
        del os.environ["CHAN_BIND_REPORT"]
    assert rc == 0, "pusch_test %s -> %d\n%s" % (" ".join(args), rc, out[-3000:])
    m = re.search(r"\[chan_bind\] pusch_decode dev (\d+) ref (\d+)", out)
    assert m is not None, out[-1500:]
    dev, ref = int(m.group(1)), int(m.group(2))
    assert dev == subframes and ref == 0, (dev, ref)
