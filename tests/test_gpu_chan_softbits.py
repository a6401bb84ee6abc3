"""The transport block's soft bits of every grant-level receive call, soft bit by soft bit: srsran_hip_pusch_decode{,_multi}, srsran_hip_pusch_decode_uci{,_multi}
and srsran_hip_pdsch_decode (include/srsran_amd/phy_chan_abi.h).

tests/test_gpu_chan.py and tests/test_gpu_pusch_uci.py look at the data soft bits through a turbo decoder that decodes -- and so corrects a soft bit in the
wrong slot or an ACK position that was not zeroed.  Here NO block may decode: the grid is built from random bits instead of a code word (the "bits -> grid"
halves of the two modules' signal helpers: T._pusch_grid, U._uci_grid), no code block passes its CRC, and the call hands every soft-buffer row back to the
caller.  After a first transmission the rows are a one-to-one image of the e bits the demodulator's store placed (sums where the circular buffer wraps), after
a second one the de-matcher's accumulating path has run on top.

Expected side, the construction the other two modules use: the q soft bits of the same stages one reference-named call at a time (T._per_stage_pusch_llrs,
which asserts the demodulator against the oracle), the ORACLE's de-interleaver table -- with control information the LITERAL de-multiplexer
U._literal_demux -- and the oracle's decode_tb with two half iterations.  Per transmission: return code 0, crc_ok 0, no code-block flag, the oracle's
iteration average, EVERY row of EVERY block equal bit for bit over its 3 (K + 32) + 12 entries and zero behind them, nothing written behind the last block's
bytes, and with control information every ACK / RI / CQI soft bit, chip and position and the guards.  The precondition is asserted, not assumed: the
oracle fails every block (a case that cannot show its rows is a failed case).

The shapes are the smallest allocations that still cross every boundary of the kernels (a tile is 2048 symbols, a wave's share 512, a pass 64): 144 .. 2160
symbols, all three modulations, 16- and 8-bit stores, 12 / 11 / 10 / 9 columns (both column sets of the de-multiplexer's rank), puncturing and repetition
in the de-matcher, Q'ri not a multiple of 4, the counts at their cap of four columns, one and two blocks, four cell widths, hopping, the cell's top edge,
zero forcing; two 8-bit allocations with an odd L_prb x columns (132 and 540 symbols, 16-QAM and 64-QAM), the only ones whose last 4 symbols take the 8-bit
demodulator's scalar tail -- which truncates where the vector body rounds: each asserts that the tail rule does change soft bits of its own input (_Ue.tail_is_seen).
The PDSCH paths get the same treatment in tests/test_gpu_pdsch_softbits.py.  The expected side of a case (literal de-multiplexer included) takes 1 to 15 ms on the CPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
import test_gpu_chan as T
import test_gpu_pusch_uci as U

pytestmark = pytest.mark.gpu
SB = T.SB
ITERS = 2  # half iterations: nothing is meant to decode
CELL_ID = 211
GROUP = {False: 4, True: 8}  # symbols per iteration of the demodulator's 16-QAM / 64-QAM vector bodies, by llr8: the last H % GROUP symbols take the scalar tail

# the allocations: cell_nof_prb, cp_nsymb, shortened, n_prb_tilde, L_prb, mod, tbs, llr8, noise_estimate, snr_db
GRANTS = {
    "qpsk_L1": (6, 7, 0, (5, 5), 1, 1, 104, False, 0.01, 8.0),  # 144 symbols: less than one wave's share; the top edge of a 6-PRB cell
    "64qam_L1_ext_8bit": (15, 6, 0, (3, 11), 1, 3, 72, True, 0.0, 25.0),  # 120 symbols, 10 columns, 6-byte stores; 720 e bits into 300 entries; hopping; ZF
    "64qam_L1_ext": (15, 6, 0, (3, 11), 1, 3, 72, False, 0.02, 25.0),
    "16qam_L3_srs": (25, 7, 1, (2, 2), 3, 2, 600, False, 0.01, 17.0),  # 396 symbols, 11 columns
    "16qam_L4_srs": (6, 7, 1, (2, 0), 4, 2, 1544, False, 0.0, 17.0),  # 528 symbols: a second wave with 16 symbols; hopping; ZF
    "qpsk_L5_ext_srs_8bit": (25, 6, 1, (20, 20), 5, 1, 808, True, 0.05, 8.0),  # 540 symbols, 9 columns, 2-byte stores; the top edge of a 25-PRB cell
    "qpsk_L5_ext_srs": (25, 6, 1, (20, 3), 5, 1, 808, False, 0.05, 8.0),
    "64qam_L15": (100, 7, 0, (85, 85), 15, 3, 6712, False, 0.01, 25.0),  # 2160 symbols: a second tile; two blocks (K 3392 / 3328); the top edge of 100 PRB
    "16qam_L16_srs_8bit": (100, 7, 1, (10, 60), 16, 2, 6200, True, 0.02, 17.0),  # 2112 symbols: a second tile with one pass; 4-byte stores; two blocks
    "16qam_L16_srs": (25, 7, 1, (9, 0), 16, 2, 6200, False, 0.01, 17.0),
    # 8 bit with L_prb x columns odd: the only allocations whose count is no multiple of 8, so that the 8-bit demodulator's last 4 symbols take its scalar tail
    "16qam_L1_srs_8bit": (25, 7, 1, (7, 7), 1, 2, 328, True, 0.01, 17.0),  # 132 symbols, 11 columns: all in one wave, 132 % 8 == 4
    "64qam_L5_ext_srs_8bit": (25, 6, 1, (20, 3), 5, 3, 1544, True, 0.02, 25.0),  # 540 symbols, 9 columns: the tail in a second wave, 540 % 8 == 4; hopping
}

# single grants: (allocation, (Q'ack, Q'ri, Q'cqi)); all zero = the plain call
SINGLE = [
    ("qpsk_L1", (0, 0, 0)), ("qpsk_L1", (1, 0, 0)), ("qpsk_L1", (0, 1, 0)), ("qpsk_L1", (0, 2, 1)), ("qpsk_L1", (48, 48, 10)),
    ("64qam_L1_ext_8bit", (0, 0, 0)), ("64qam_L1_ext", (5, 3, 7)), ("64qam_L1_ext", (48, 48, 5)),
    ("16qam_L3_srs", (0, 0, 0)), ("16qam_L3_srs", (7, 5, 9)), ("16qam_L3_srs", (0, 0, 36)),
    ("16qam_L4_srs", (0, 0, 0)), ("16qam_L4_srs", (13, 6, 0)),
    ("qpsk_L5_ext_srs_8bit", (0, 0, 0)), ("qpsk_L5_ext_srs", (9, 2, 31)),
    ("64qam_L15", (0, 0, 0)), ("64qam_L15", (24, 5, 60)), ("64qam_L15", (720, 720, 100)),
    ("16qam_L16_srs_8bit", (0, 0, 0)), ("16qam_L16_srs", (30, 7, 44)),
    ("16qam_L1_srs_8bit", (0, 0, 0)), ("64qam_L5_ext_srs_8bit", (0, 0, 0)),
]

# the grants of a TTI, all inside a 100-PRB grid: (allocation, n_prb_tilde, counts for the call with control information).  Two grants of one PRB with a
# three-PRB one between them in list order (the host sorts by L_prb and runs one transform launch per size: 12 + 10 + 10 rows of 12 points in one, two
# column counts in it), the same for 5 and 16 PRB; all five 8-bit grants; hopping; the top edge.
TTI = [
    ("64qam_L15", (0, 0), (24, 5, 60)), ("qpsk_L1", (15, 99), (0, 2, 1)), ("16qam_L16_srs", (16, 16), (30, 7, 44)), ("16qam_L3_srs", (32, 32), (0, 0, 0)),
    ("64qam_L1_ext_8bit", (35, 35), (0, 0, 0)), ("qpsk_L5_ext_srs_8bit", (36, 59), (0, 0, 0)), ("16qam_L4_srs", (41, 41), (13, 6, 0)),
    ("16qam_L16_srs_8bit", (45, 84), (0, 0, 0)), ("qpsk_L5_ext_srs", (61, 36), (9, 2, 31)), ("64qam_L1_ext", (99, 66), (48, 48, 5)),
    ("16qam_L1_srs_8bit", (67, 67), (0, 0, 0)), ("64qam_L5_ext_srs_8bit", (68, 73), (0, 0, 0)),
]
TTI_SUBFRAME = 7


class _Ue:
    """one grant's HARQ process on both sides: the library's soft buffer (the caller's rows) and the oracle's"""

    def __init__(self, capi, name, counts, rnti, n_prb=None, cell=None):
        self.capi, self.name, self.counts, self.rnti = capi, name, counts, rnti
        self.cell, self.cp, self.short, self.n_prb, self.L, self.mod, self.tbs, self.llr8, self.noise, self.snr = GRANTS[name]
        if n_prb is not None:
            self.cell, self.n_prb = cell, n_prb
        self.Qm = O.QM[self.mod]
        self.cols = 2 * (self.cp - 1) - (1 if self.short else 0)
        self.H = self.cols * 12 * self.L
        self.dt = np.int8 if self.llr8 else np.int16
        self.seg = O.cbsegm(self.tbs)
        self.nb = self.seg["C"]
        self.sb, self.rows, self.keep, self.flags = T._rx_softbuffer(capi, self.nb + 1, self.dt)  # (one row more than the block has: it stays zero)
        self.soft = np.zeros((self.nb, SB), self.dt)
        self.crc = np.zeros(self.nb, np.uint8)
        self.lut = O.ulsch_interleaver_lut(self.H, self.Qm, self.cols)

    def transmit(self, rng, rv, counts=None, gain=1.0):
        """a transmission of RANDOM bits in place of the code word: grid, estimates, the grant and the caller's outputs"""
        capi = self.capi
        self.counts = self.counts if counts is None else counts
        Qa, Qr, Qc = self.counts
        self.rv = rv
        e = rng.integers(0, 2, (self.H - Qr - Qc) * self.Qm).astype(np.uint8)
        sig = (rng, self.cell, self.cp, self.n_prb, self.L, self.short, self.mod)
        if any(self.counts):
            self.grid, self.ce, seed = U._uci_grid(*sig, e, self.rnti, TTI_SUBFRAME, CELL_ID, self.snr, Qa, Qr, Qc)
        else:
            self.grid, self.ce, seed = T._pusch_grid(*sig, e[self.lut], self.rnti, TTI_SUBFRAME, CELL_ID, self.snr)
        if gain != 1.0:
            self.grid = np.ascontiguousarray(self.grid * np.float32(gain))
        self.seed = seed
        self.grant = U._grant(capi, self.cell, self.cp, self.n_prb, self.L, self.short, self.mod, self.tbs, rv, seed, ITERS, self.noise, llr8=self.llr8)
        self.uci = capi.HipPuschUci(Qa, Qr, Qc)
        self.out = U._UciOut(capi, self.Qm, Qa, Qr, Qc)
        self.data = np.full(self.tbs // 8 + 16, 0xA5, np.uint8)

    def new_softbuffer(self):
        """a second soft buffer on the library's side in the state of the first (the same transmissions through another entry point)"""
        sb, rows, keep, flags = T._rx_softbuffer(self.capi, self.nb + 1, self.dt)
        for a, b in zip(rows, self.rows):
            a[:] = b
        return sb, rows, keep, flags

    def expect(self, lib):
        """the oracle's side of the transmission: self.soft / self.crc move on, returns what the call must report"""
        d = []
        q, _ = T._per_stage_pusch_llrs(lib, self.capi, self.grid, self.ce, self.cell, self.cp, self.n_prb, self.L, self.short, self.mod, self.rnti, TTI_SUBFRAME,
                                       CELL_ID, self.noise, self.llr8, symbols_out=d)
        if self.mod in (2, 3) and self.H % GROUP[self.llr8]:
            self.tail_is_seen(lib, d[0], q)
        ctl = None
        if any(self.counts):
            ack, ackp, ri, rip, cqi, e, gbits = U._literal_demux(q, self.H, self.cols, self.Qm, *self.counts)
            ctl = (q, ack, ackp, ri, rip, cqi, gbits)
        else:
            e = np.zeros_like(q)
            e[self.lut] = q  # srsran_vec_lut_sis(q_bits, lut, g_bits, n): g[lut[i]] = q[i]
        ret, _, avg = O.sch_decode_tb(self.tbs, self.Qm, self.rv, e, self.soft, self.crc, ITERS)
        # the precondition: no block decodes, so every row comes back
        assert ret == -1 and not self.crc.any(), (self.name, self.counts, self.rv, ret, self.crc)
        return avg, ctl

    def tail_is_seen(self, lib, d, q):
        """the demodulator's symbols with 16 more behind them, on the oracle: the q soft bits must change, and only in the symbols its scalar tail covers (the last
        H % 8 of 8-bit 16-QAM / 64-QAM; 16 bit: H % 4, which no allocation has).  A grant that cannot show this is a failed case"""
        more = O.qam_symbols(self.mod, 16, self.H, snr_db=self.snr)
        llr = O.demod_soft(self.mod, np.concatenate([d, more]), "b" if self.llr8 else "s")[:q.size]
        body = np.zeros_like(llr)
        (lib.srsran_sequence_pusch_apply_c if self.llr8 else lib.srsran_sequence_pusch_apply_s)(O.P(llr), O.P(body), self.rnti, 2 * (TTI_SUBFRAME % 10), CELL_ID, llr.size)
        diff = np.flatnonzero(body != q)
        tag = (self.name, self.counts, self.rv)
        assert diff.size > 0, tag + ("the tail rule changes no soft bit of this grant",)
        assert diff[0] >= (self.H - self.H % GROUP[self.llr8]) * self.Qm, tag + (int(diff[0]),)
        print("%s rv %d: %d soft bits that the tail rule decides" % (self.name, self.rv, diff.size))

    def spans(self):
        return [3 * ((self.seg["K1"] if i < self.seg["C1"] else self.seg["K2"]) + 32) + 12 for i in range(self.nb)]

    def check(self, res, avg, ctl, sb=None, rows=None, flags=None, data=None, out=None):
        tag = (self.name, self.counts, self.rv)
        sb, rows, flags = (self.sb, self.rows, self.flags) if sb is None else (sb, rows, flags)
        data = self.data if data is None else data
        out = self.out if out is None else out
        assert res.crc_ok == 0 and not sb.tb_crc, tag
        assert not flags.any(), tag
        assert abs(res.avg_iterations_block - avg) < 1e-6, tag + (res.avg_iterations_block, avg)
        assert np.isnan(res.epre), tag
        for i, span in enumerate(self.spans()):
            bad = np.flatnonzero(rows[i][:span] != self.soft[i][:span])
            assert bad.size == 0, tag + ("block %d: %d of %d soft bits differ, the first at %d: %d, the oracle has %d" %
                                         (i, bad.size, span, bad[0], rows[i][bad[0]], self.soft[i][bad[0]]),)
            assert not rows[i][span:].any() and not self.soft[i][span:].any(), tag + (i,)
        assert not rows[self.nb].any(), tag
        # the bytes of the blocks end at tbs / 8 + 3 (one block: K / 8) or + 6 (the last block's CRC24B behind the CRC24A): nothing is written behind them
        assert np.all(data[self.tbs // 8 + (6 if self.nb > 1 else 3):] == 0xA5), tag
        if ctl is None:
            return
        q, ack, ackp, ri, rip, cqi, gbits = ctl
        Qa, Qr, Qc = self.counts
        chips = O.sequence_bits(self.seed, self.H * self.Qm)
        ack_llr, ack_c, ack_pos, ri_llr, ri_c, ri_pos, cqi_llr = out.arrays()
        assert np.array_equal(ack_pos, ackp) and np.array_equal(ri_pos, rip), tag
        assert np.array_equal(ack_llr, ack) and np.array_equal(ack_c, chips[ackp] if Qa else chips[:0]), tag
        assert np.array_equal(ri_llr, ri) and np.array_equal(ri_c, chips[rip] if Qr else chips[:0]), tag
        assert np.array_equal(cqi_llr, cqi), tag
        assert out.guards_intact(), tag
        if Qr > 0 and Qc > 0:  # g[0]: the soft bit of the highest RI position (RI symbol 1; symbol 0 when there is only one)
            assert cqi_llr[0] == q[U._positions(1 if Qr >= 2 else 0, self.Qm, self.H, self.cols, U.RI_COLS)[-1]] == gbits[0], tag


def _single_call(lib, capi, ue, with_uci, sb=None, data=None, out=None):
    sb = ue.sb if sb is None else sb
    data = ue.data if data is None else data
    out = ue.out if out is None else out
    res = capi.HipGrantRes(7, 7.0, 7.0)
    if with_uci:
        rc = lib.srsran_hip_pusch_decode_uci(C.byref(ue.grant), C.byref(ue.uci), O.P(ue.grid), O.P(ue.ce), C.byref(sb), O.P(data), C.byref(res), C.byref(out.c))
    else:
        rc = lib.srsran_hip_pusch_decode(C.byref(ue.grant), O.P(ue.grid), O.P(ue.ce), C.byref(sb), O.P(data), C.byref(res))
    assert rc == 0, (ue.name, ue.counts, ue.rv, capi.last_error())
    return res


# ---- 1. single grants: rv 0 into an empty soft buffer (the de-matcher's first-write path), then rv 2 with other bits on top (its accumulating path) ----------------

@pytest.mark.parametrize("name,counts", SINGLE, ids=["%s_ack%d_ri%d_cqi%d" % ((n,) + c) for n, c in SINGLE])
def test_pusch_grant_rows_against_the_oracle(hiplib, name, counts):
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(4000 + 31 * SINGLE.index((name, counts)))
    ue = _Ue(capi, name, counts, 0x46)
    # counts (0, 0, 0) with 16-bit soft bits: also through the call that takes control information, on a soft buffer of its own -- identical rows
    twin = ue.new_softbuffer() if not any(counts) and not ue.llr8 else None
    for rv in (0, 2):
        ue.transmit(rng, rv)
        res = _single_call(lib, capi, ue, any(counts))
        avg, ctl = ue.expect(lib)
        ue.check(res, avg, ctl)
        if twin is not None:
            data2 = np.full_like(ue.data, 0xA5)
            res2 = _single_call(lib, capi, ue, True, sb=twin[0], data=data2)
            ue.check(res2, avg, None, sb=twin[0], rows=twin[1], flags=twin[3], data=data2)
            for a, b in zip(twin[1], ue.rows):
                assert np.array_equal(a, b), (name, rv)


def test_pusch_8bit_rows_where_the_sum_leaves_int8(hiplib):
    """8-bit soft bits combined beyond the number format: rv 0, then rv 0 three more times with the grid scaled by 3 (QPSK soft bits of about +-60 on top of
    +-20).  The reference's 8-bit de-matcher adds with wrap-around (rm_turbo.c:474-476 `output[..] += input[i]` on int8_t; there is no clamp in it), and
    so does the oracle's: the rows must follow it there too.  That sums do leave [-128, 127] is asserted on the expected side: each transmission's own
    contribution (the oracle on an empty soft buffer; E < 3 K + 12, so every entry gets at most one soft bit) is added to the previous rows in wide
    arithmetic."""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(77)
    ue = _Ue(capi, "qpsk_L5_ext_srs_8bit", (0, 0, 0), 0x46)
    assert ue.H * ue.Qm < 3 * ue.seg["K1"] + 12
    wrapped = 0
    for k in range(4):
        ue.transmit(rng, 0, gain=1.0 if k == 0 else 3.0)
        res = _single_call(lib, capi, ue, False)
        before = ue.soft.astype(np.int32)
        avg, ctl = ue.expect(lib)
        ue.check(res, avg, ctl)
        # this transmission alone
        q, _ = T._per_stage_pusch_llrs(lib, capi, ue.grid, ue.ce, ue.cell, ue.cp, ue.n_prb, ue.L, ue.short, ue.mod, ue.rnti, TTI_SUBFRAME, CELL_ID, ue.noise, True)
        e = np.zeros_like(q)
        e[ue.lut] = q
        alone = np.zeros((ue.nb, SB), np.int8)
        O.sch_decode_tb(ue.tbs, ue.Qm, 0, e, alone, np.zeros(ue.nb, np.uint8), ITERS)
        wide = before + alone
        assert np.array_equal(wide.astype(np.int8), ue.soft)  # (astype wraps)
        wrapped += int(np.count_nonzero((wide > 127) | (wide < -128)))
    assert wrapped > 0, "no combined soft bit left the int8 range: the case does not reach the edge it is for"


# ---- 2. the grants of a TTI in one call, held to the oracle directly ---------------------------------------------------------------------------------------------------

def _multi_call(lib, capi, ues, with_uci):
    n = len(ues)
    grants = (capi.HipPuschRx * n)(*[u.grant for u in ues])
    grids, ces = (C.c_void_p * n)(*[u.grid.ctypes.data for u in ues]), (C.c_void_p * n)(*[u.ce.ctypes.data for u in ues])
    sbs = (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(u.sb) for u in ues])
    datas = (C.c_void_p * n)(*[u.data.ctypes.data for u in ues])
    res = (capi.HipGrantRes * n)(*[capi.HipGrantRes(7, 7.0, 7.0) for _ in range(n)])
    if with_uci:
        ucis = (capi.HipPuschUci * n)(*[u.uci for u in ues])
        oc = (capi.HipPuschUciOut * n)(*[u.out.c for u in ues])
        rc = lib.srsran_hip_pusch_decode_uci_multi(n, grants, ucis, grids, ces, sbs, datas, res, oc)
    else:
        rc = lib.srsran_hip_pusch_decode_multi(n, grants, grids, ces, sbs, datas, res)
    assert rc == 0, capi.last_error()
    return res


@pytest.mark.parametrize("with_uci", [False, True], ids=["multi", "uci_multi"])
def test_pusch_tti_rows_against_the_oracle(hiplib, with_uci):
    """srsran_hip_pusch_decode_multi and srsran_hip_pusch_decode_uci_multi over ten grants of one TTI (the job lists of the equaliser, the transform runs per
    allocation size and both demodulator launches), rv 0 and then rv 2 on the same soft buffers: every row of every grant against the oracle, not against
    the single call"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(8100 + int(with_uci))
    ues = [_Ue(capi, name, counts if with_uci else (0, 0, 0), 0x100 + i, n_prb=n_prb, cell=100) for i, (name, n_prb, counts) in enumerate(TTI)]
    sizes = [u.L for u in ues]
    # two grants of one size with another size between them in list order
    assert any(sizes[i] == sizes[k] and any(x != sizes[i] for x in sizes[i + 1:k]) for i in range(len(sizes)) for k in range(i + 2, len(sizes)))
    assert sum(u.llr8 for u in ues) == sum(g[7] for g in GRANTS.values())  # every 8-bit grant of the table
    assert not with_uci or (any(any(u.counts) for u in ues) and not all(any(u.counts) for u in ues))
    for rv in (0, 2):
        for u in ues:
            u.transmit(rng, rv)
        res = _multi_call(lib, capi, ues, with_uci)
        for i, u in enumerate(ues):
            avg, ctl = u.expect(lib)
            u.check(res[i], avg, ctl)


# ---- 3. PDSCH through the product entry point -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mod,tbs,nof_re,eq,llr8", [(1, 328, 300, False, True), (4, 6200, 2100, True, False)], ids=["qpsk_8bit_preequalised", "256qam_eq_scaled"])
def test_pdsch_codeword_rows_against_the_oracle(hiplib, mod, tbs, nof_re, eq, llr8):
    """srsran_hip_pdsch_decode on random bits: rv 0, then rv 2 on the same soft buffer; the rows against the oracle's decode_tb on the soft bits of the stages
    one call at a time (the equaliser with scaling 0.8 and the demodulator on the library, each held to the oracle in test_gpu_modem.py; the oracle's
    descrambler)"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = S.lib()
    rng = np.random.default_rng(tbs + nof_re)
    Qm = O.QM[mod]
    nbits = nof_re * Qm
    seg = O.cbsegm(tbs)
    nb = seg["C"]
    scaling, noise = 0.8, 0.02
    seed = O.pdsch_seed(0x1234, 0, 10, 301)
    dt = np.int8 if llr8 else np.int16
    sb, rows, keep, flags = T._rx_softbuffer(capi, nb + 1, dt)
    soft = np.zeros((nb, SB), dt)
    crc = np.zeros(nb, np.uint8)
    snr = {1: 9.0, 4: 34.0}[mod]
    sigma = 10 ** (-snr / 20) / np.sqrt(2)
    for rv in (0, 2):
        bits = rng.integers(0, 2, nbits).astype(np.uint8)
        x = O.modulate_bytes(mod, np.packbits(bits), nbits, seed=seed, scramble=True, scaling=scaling if eq else 1.0)
        h = (0.9 + 0.1 * rng.standard_normal(nof_re) + 0.1j * rng.standard_normal(nof_re)).astype(np.complex64) if eq else np.ones(nof_re, np.complex64)
        y = (h * x + sigma * (rng.standard_normal(nof_re) + 1j * rng.standard_normal(nof_re))).astype(np.complex64)
        g = capi.HipPdschRx(capi.HipGrantTb(mod, tbs, rv, nof_re, seed, ITERS, 1 if llr8 else 0, 1), scaling, noise)
        data = np.full(tbs // 8 + 16, 0xA5, np.uint8)
        res = capi.HipGrantRes(7, 7.0, 7.0)
        assert lib.srsran_hip_pdsch_decode(C.byref(g), O.P(y), O.P(h) if eq else None, C.byref(sb), O.P(data), C.byref(res)) == 0, capi.last_error()
        d = y
        if eq:
            d = np.zeros(nof_re, np.complex64)
            assert lib.srsran_predecoding_single(O.P(y), O.P(h), O.P(d), None, nof_re, scaling, noise) == nof_re
        llr = np.zeros(nbits, dt)
        assert (lib.srsran_demod_soft_demodulate_b if llr8 else lib.srsran_demod_soft_demodulate_s)(mod, O.P(d), O.P(llr), nof_re) == 0
        assert np.array_equal(llr, O.demod_soft(mod, d, "b" if llr8 else "s"))
        llr = O.sequence_apply(llr, seed)
        ret, _, avg = O.sch_decode_tb(tbs, Qm, rv, llr, soft, crc, ITERS)
        assert ret == -1 and not crc.any(), (rv, ret, crc)  # the precondition: every row comes back
        assert res.crc_ok == 0 and not sb.tb_crc and not flags.any(), rv
        assert abs(res.avg_iterations_block - avg) < 1e-6, (rv, res.avg_iterations_block, avg)
        for i in range(nb):
            span = 3 * ((seg["K1"] if i < seg["C1"] else seg["K2"]) + 32) + 12
            bad = np.flatnonzero(rows[i][:span] != soft[i][:span])
            assert bad.size == 0, (rv, i, bad.size, span, int(bad[0]))
            assert not rows[i][span:].any(), (rv, i)
        assert not rows[nb].any(), rv
        assert np.all(data[tbs // 8 + (6 if nb > 1 else 3):] == 0xA5), rv
