"""One device call per NR codeword (include/srsran_amd/phy_nr_chan_abi.h) against the oracle, bit for bit.

Expected side of a received codeword: x = the library's own host-pointer srsran_predecoding_single(y, h, ...) when channel estimates are given (it has its
own oracle test in test_gpu_modem.py), else the symbols; e = O.sequence_apply(-O.demod_soft(mod, x, "b"), seed) with the negation wrapping in int8;
then O.sch_nr_decode_tb.  Every integer result is compared with np.array_equal.

Shapes: the smallest that cross the kernels' boundaries (tile 2048 symbols, wave share 512, pass 64, odd counts) -- see SHAPES."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

QM = {1: 2, 2: 4, 3: 6, 4: 8}
# (mod, nof_re, tbs, R), and what the oracle must report for it: (base graph, code blocks, lifting size)
SHAPES = [((1, 24, 24, 0.5), (2, 1, 7)),         # far below one wave; CRC16, 30 filler bits
          ((1, 156, 120, 0.4), (2, 1, 24)),
          ((2, 513, 1032, 0.5), (2, 1, 112)),     # one symbol into a second wave's share; odd count
          ((2, 1999, 3848, 0.48), (1, 1, 176)),   # odd; just short of a tile
          ((3, 2049, 4104, 0.35), (1, 1, 192)),   # one symbol into a second tile; 6-byte stores
          ((3, 2050, 9480, 0.8), (1, 2, 224)),
          ((4, 2100, 9000, 0.55), (1, 2, 208)),   # 8-byte stores
          ((4, 4133, 25104, 0.76), (1, 3, 384))]  # two sizes of E (11016 / 11024); a third tile
ESN0 = {1: 6.0, 2: 13.0, 3: 19.0, 4: 26.0}
SCALING, MAX_ITER = 0.8, 6
SBW, DS = 66 * 384, 8448 // 8
NEW_DATA = 0x100
GUARD = 16


def _lib(hiplib):
    from srslte_amd import capi

    for name in ("srsran_hip_nr_cw_decode", "srsran_hip_nr_cw_decode_dbg", "srsran_hip_nr_cw_decode_multi", "srsran_hip_nr_cw_encode",
                 "srsran_hip_nr_cw_encode_multi", "srsran_hip_sequence_nr_seed"):
        assert hasattr(hiplib, name), "%s is missing from the library" % name  # a missing symbol FAILS
    return hiplib, capi


@functools.lru_cache(maxsize=None)
def _cfg(i):
    (mod, n, tbs, R), (graph, blocks, Z) = SHAPES[i]
    cfg = O.sch_nr_tb_info(tbs, R, mod, n * QM[mod], 1, 0)
    assert (cfg.bg + 1, cfg.C, cfg.Z) == (graph, blocks, Z), (i, cfg.bg, cfg.C, cfg.Z)
    cfg.Nref = (66 if cfg.bg == 0 else 50) * cfg.Z  # full buffer (the library takes Nref = 0 for it)
    return cfg


def _N(cfg):
    return (66 if cfg.bg == 0 else 50) * cfg.Z


def _seed(i):
    return ((0x4601 + 37 * i) << 15) + ((i & 1) << 14) + 500 + i


def _noise(rng, n, esn0_db):
    sigma = np.sqrt(10.0 ** (-esn0_db / 10.0) / 2.0)
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


@functools.lru_cache(maxsize=None)
def _payload(i, key=0):
    return np.random.default_rng(1000 + 10 * i + key).integers(0, 256, SHAPES[i][0][2] // 8).astype(np.uint8)


def _tx_symbols(i, bits, seed):
    mod = SHAPES[i][0][0]
    return O.modulate_bytes(mod, np.packbits(bits), bits.size, seed, True, 1.0)


def _rx_symbols(i, bits, seed, esn0_db, rng, mode):
    """bits -> scrambled constellation points + noise [-> through a random channel of magnitude 0.5 ... 1.5].  mode: 'none' (already equalised), 'zf', 'mmse'.
    The noise goes on in front of the channel, so the operating point is the same in every mode.  Returns (symbols, ce or None, noise_estimate)."""
    n = SHAPES[i][0][1]
    d = _tx_symbols(i, bits, seed).astype(np.complex128) + _noise(rng, n, esn0_db)
    if mode == "none":
        return d.astype(np.complex64), None, 0.0
    h = rng.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    return (d * h).astype(np.complex64), h.astype(np.complex64), (1e-3 if mode == "mmse" else 0.0)


def _equalised(hiplib, y, h, ne):
    if h is None:
        return y
    x = np.zeros_like(y)
    assert hiplib.srsran_predecoding_single(O.P(y), O.P(h), O.P(x), None, y.size, 1.0, ne) == y.size
    return x


def _soft_bits(hiplib, mod, y, h, ne, seed):
    d = O.demod_soft(mod, _equalised(hiplib, y, h, ne), "b")
    return O.sequence_apply(-d, seed)  # int8 negation wraps: -(-128) = -128


class Softbuffer:
    """the reference's srsran_softbuffer_rx_t on host memory, rows used as int8 (sch_nr.c:570), with guard bytes behind every row"""

    def __init__(self, max_cb, size=SBW):
        from srslte_amd import capi

        self.rows = [np.zeros(size + GUARD, np.int8) for _ in range(max_cb)]
        self.keep = [np.zeros(DS + GUARD, np.uint8) for _ in range(max_cb)]
        self.flags = np.zeros(max_cb, np.bool_)
        self.c = capi.SoftbufferRx(max_cb, size, (C.c_void_p * max_cb)(*[r.ctypes.data for r in self.rows]),
                                   (C.c_void_p * max_cb)(*[k.ctypes.data for k in self.keep]), self.flags.ctypes.data_as(C.POINTER(C.c_bool)), False)

    def snapshot(self):
        return [r.copy() for r in self.rows], [k.copy() for k in self.keep], self.flags.copy()

    def same_as(self, snap):
        return (all(np.array_equal(a, b) for a, b in zip(self.rows, snap[0])) and all(np.array_equal(a, b) for a, b in zip(self.keep, snap[1])) and
                np.array_equal(self.flags, snap[2]))


class Oracle:
    """the oracle's soft buffer of one HARQ process"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.soft, self.crc, self.data = np.zeros((cfg.C, SBW), np.int8), np.zeros(cfg.C, np.uint8), np.zeros((cfg.C, DS), np.uint8)

    def decode(self, rv, e, max_iter=MAX_ITER):
        return O.sch_nr_decode_tb(self.cfg, rv, SCALING, max_iter, e, self.soft, self.crc, self.data)


def _rx(capi, i, rv, seed, ne, max_iter=MAX_ITER, nof_bits=None):
    mod, n, tbs, R = SHAPES[i][0]
    return capi.HipNrCwRx(capi.HipNrTb(R, tbs, mod, rv, 1, n * QM[mod] if nof_bits is None else nof_bits, 0, 0, 0, 0, 0), n, seed, SCALING, max_iter, ne, 0)


def _check_state(sb, orc, tag):
    """flags, stored code blocks and the rows of undecoded blocks equal the oracle's; nothing behind a row's N entries or a stored block is written"""
    cfg = orc.cfg
    N, cb_bytes = _N(cfg), (cfg.Kp - cfg.L_cb + 7) // 8
    assert np.array_equal(sb.flags[:cfg.C].astype(np.uint8), orc.crc) and not sb.flags[cfg.C:].any(), (tag, sb.flags, orc.crc)
    for r in range(cfg.C):
        if orc.crc[r]:
            assert np.array_equal(sb.keep[r][:cb_bytes], orc.data[r][:cb_bytes]), (tag, r)
        else:
            assert np.array_equal(sb.rows[r][:N], orc.soft[r][:N]), (tag, r)
        assert not sb.rows[r][N:].any() and not sb.keep[r][cb_bytes:].any(), (tag, r)
    for r in range(cfg.C, len(sb.rows)):
        assert not sb.rows[r].any() and not sb.keep[r].any(), (tag, r)


def _check_result(res, out, tbs, ok, avg, orc, o_out, tag):
    assert res.nof_cb == orc.cfg.C and res.all_decoded == int(orc.crc.all()) and res.crc_ok == (ok if orc.crc.all() else 0), (tag, res.crc_ok, res.all_decoded, ok)
    print(tag, "avg_iter", res.avg_iter, "oracle", avg)
    assert abs(res.avg_iter - avg) < 1e-6, (tag, res.avg_iter, avg)
    if orc.crc.all():
        assert np.array_equal(out[:tbs // 8], o_out), tag
    else:
        assert np.all(out[:tbs // 8] == 0xEE), tag
    assert np.all(out[tbs // 8:] == 0xEE), tag


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_decoding_codewords(hiplib, i):
    """every shape, with channel estimates (MMSE and zero forcing) and without: return code, result, payload, guard bytes; through _dbg every soft bit"""
    L, capi = _lib(hiplib)
    (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
    payload, seed = _payload(i), _seed(i)
    e_tx = O.sch_nr_encode_tb(cfg, 0, payload)
    for k, mode in enumerate(("mmse", "zf", "none")):
        rng = np.random.default_rng(100 * i + k)
        y, h, ne = _rx_symbols(i, e_tx, seed, ESN0[mod], rng, mode)
        e = _soft_bits(L, mod, y, h, ne, seed)
        orc = Oracle(cfg)
        o_out, ok, avg = orc.decode(0, e)
        assert orc.crc.all() and ok == 1 and np.array_equal(o_out, payload), (i, mode, orc.crc)  # precondition: the oracle decodes every block
        sb = Softbuffer(cfg.C + 1)
        out, e_out = np.full(tbs // 8 + GUARD, 0xEE, np.uint8), np.full(e.size + GUARD, 0x55, np.int8)
        res = capi.HipNrTbResult()
        g = _rx(capi, i, NEW_DATA if k else 0, seed, ne)  # (a soft buffer as srsran_softbuffer_rx_reset leaves it needs no flag)
        rc = L.srsran_hip_nr_cw_decode_dbg(C.byref(g), O.P(y), O.P(h) if h is not None else None, C.byref(sb.c), O.P(out), C.byref(res), O.P(e_out))
        assert rc == 0, (i, mode, capi.last_error())
        assert np.array_equal(e_out[:e.size], e) and np.all(e_out[e.size:] == 0x55), (i, mode, int((e_out[:e.size] != e).sum()))
        _check_result(res, out, tbs, ok, avg, orc, o_out, (i, mode))
        _check_state(sb, orc, (i, mode))
        # the plain call gives the same
        sb2, out2, res2 = Softbuffer(cfg.C + 1), np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
        assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(y), O.P(h) if h is not None else None, C.byref(sb2.c), O.P(out2), C.byref(res2)) == 0
        assert np.array_equal(out2, out) and (res2.crc_ok, res2.all_decoded, res2.avg_iter, res2.nof_cb) == (res.crc_ok, res.all_decoded, res.avg_iter, res.nof_cb)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_soft_bit_placement_where_nothing_decodes(hiplib, i):
    """symbols built from random bits: no flag, payload untouched, the oracle's iteration average, every row of every block equal to the oracle's over all N
    entries and zero behind them; then a second transmission with rv 2 on top (the accumulating path) and the same comparison"""
    L, capi = _lib(hiplib)
    (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
    seed, rng = _seed(i) ^ 0x155, np.random.default_rng(7000 + i)
    sb, orc = Softbuffer(cfg.C + 1), Oracle(cfg)
    for rv, mode in ((0, "zf"), (2, "none")):
        bits = rng.integers(0, 2, n * QM[mod]).astype(np.uint8)
        y, h, ne = _rx_symbols(i, bits, seed, ESN0[mod], rng, mode)
        e = _soft_bits(L, mod, y, h, ne, seed)
        o_out, ok, avg = orc.decode(rv, e)
        assert not orc.crc.any() and avg == MAX_ITER, (i, rv, orc.crc, avg)  # precondition: none of the blocks decodes
        out, res = np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
        g = _rx(capi, i, rv, seed, ne)
        assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(y), O.P(h) if h is not None else None, C.byref(sb.c), O.P(out), C.byref(res)) == 0, capi.last_error()
        _check_result(res, out, tbs, ok, avg, orc, o_out, (i, rv))
        _check_state(sb, orc, (i, rv))


def test_harq_retransmission_decodes(hiplib):
    """the 2050-symbol 64-QAM shape at 14 dB: rv 0 (new data) leaves both blocks undecoded, rv 2 for the undecoded blocks on top decodes; flags, rows,
    average and payload are held to the oracle after each call"""
    L, capi = _lib(hiplib)
    i = 5
    (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
    payload, seed, rng = _payload(i, 1), _seed(i) + 3, np.random.default_rng(100)
    sb, orc = Softbuffer(cfg.C), Oracle(cfg)
    for step, (rv, flag, mode) in enumerate(((0, NEW_DATA, "mmse"), (2, 0, "zf"))):
        e_tx = O.sch_nr_encode_tb(cfg, rv, payload)
        assert not orc.crc.any()  # both blocks are still undecoded: the retransmission carries all of them
        y, h, ne = _rx_symbols(i, e_tx, seed, 14.0, rng, mode)
        e = _soft_bits(L, mod, y, h, ne, seed)
        o_out, ok, avg = orc.decode(rv, e)
        out, res = np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
        g = _rx(capi, i, rv | flag, seed, ne)
        assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(y), O.P(h), C.byref(sb.c), O.P(out), C.byref(res)) == 0, capi.last_error()
        _check_result(res, out, tbs, ok, avg, orc, o_out, ("harq", rv))
        _check_state(sb, orc, ("harq", rv))
        if step == 0:
            assert not orc.crc.any(), orc.crc  # precondition: the first transmission leaves both blocks undecoded
        else:
            assert orc.crc.all() and ok == 1 and np.array_equal(out[:tbs // 8], payload)  # ... and the second decodes


@pytest.mark.parametrize("mod", [1, 2, 3, 4])
def test_pusch_order_gives_the_same_soft_bits(hiplib, mod):
    """pusch_nr_decode_codeword descrambles and then changes the sign, pdsch_nr_decode_codeword the other way round.  On an input that saturates the
    demodulator (-128 and 127 both occur) the two orders give the same soft bits, so one call serves both channels.  If the equality below ever
    fails, srsran_hip_nr_cw_decode needs an order flag."""
    L, capi = _lib(hiplib)
    i = [k for k, s in enumerate(SHAPES) if s[0][0] == mod][0]
    (_, n, tbs, R), seed = SHAPES[i][0], _seed(i) + 11
    x = (6.0 * O.qam_symbols(mod, n, 40 + mod, snr_db=12.0)).astype(np.complex64)
    d = O.demod_soft(mod, x, "b")
    assert d.min() == -128 and d.max() == 127
    pdsch, pusch = O.sequence_apply(-d, seed), -O.sequence_apply(d, seed)
    assert np.array_equal(pdsch, pusch)
    sb, out, res = Softbuffer(_cfg(i).C), np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
    e_out = np.zeros(d.size, np.int8)
    g = _rx(capi, i, NEW_DATA, seed, 0.0)
    assert L.srsran_hip_nr_cw_decode_dbg(C.byref(g), O.P(x), None, C.byref(sb.c), O.P(out), C.byref(res), O.P(e_out)) == 0, capi.last_error()
    assert np.array_equal(e_out, pusch)


def _multi_entries(L):
    """ten codewords: all shapes plus two repeats, modulations mixed, with and without channel estimates, not sorted by size; entry 3 is a retransmission
    into a soft buffer with a flag set, entry 9 runs with another iteration limit (a second decoder pass)"""
    entries = []
    order = [7, 0, 4, 5, 2, 6, 1, 3, 5, 2]
    for k, i in enumerate(order):
        (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
        rng = np.random.default_rng(9000 + k)
        payload, seed = _payload(i, 2 + k), _seed(i) + 100 * k
        mode = ("mmse", "none", "zf")[k % 3]
        max_iter = 4 if k == 9 else MAX_ITER
        sb, orc, rv = Softbuffer(cfg.C + 1), Oracle(cfg), 0
        if k == 3:
            # HARQ state of a process whose first block is decoded and stored and whose second holds the soft bits of a failed first transmission
            assert cfg.C == 2
            clean = Oracle(cfg)
            clean.decode(0, (20 * (1 - 2 * O.sch_nr_encode_tb(cfg, 0, payload).astype(np.int16))).astype(np.int8))
            assert clean.crc.all()
            y0, _, _ = _rx_symbols(i, O.sch_nr_encode_tb(cfg, 0, payload), seed, 14.0, rng, "none")
            orc.decode(0, _soft_bits(L, mod, y0, None, 0.0, seed))
            assert not orc.crc.any()
            orc.crc[0], orc.data[0] = 1, clean.data[0]
            sb.flags[0] = True
            sb.keep[0][:DS] = clean.data[0]
            sb.rows[1][:SBW] = orc.soft[1]
            # the retransmission: sch_nr_decode reads the soft bits of the undecoded blocks back to back from the start of the codeword (sch_nr.c:584-656)
            rv = 2
            E0 = O.sch_nr_get_E(cfg, 0)
            e2 = O.sch_nr_encode_tb(cfg, rv, payload)
            bits = np.concatenate([e2[E0:], rng.integers(0, 2, E0).astype(np.uint8)])
        else:
            bits = O.sch_nr_encode_tb(cfg, rv, payload)
        y, h, ne = _rx_symbols(i, bits, seed, 14.0 if k == 3 else ESN0[mod], rng, mode)
        e = _soft_bits(L, mod, y, h, ne, seed)
        o_out, ok, avg = orc.decode(rv, e, max_iter)
        entries.append(dict(i=i, rv=rv, seed=seed, ne=ne, max_iter=max_iter, y=y, h=h, sb=sb, orc=orc, o_out=o_out, ok=ok, avg=avg, tbs=tbs, payload=payload))
    assert entries[3]["orc"].crc.all() and np.array_equal(entries[3]["o_out"], entries[3]["payload"])  # the retransmission completes the transport block
    return entries


def test_multi_call(hiplib):
    """ten codewords in one call: every result, payload, flag and row equals what the oracle gives for that codeword alone; the same list with one
    invalid entry is refused with every result initialised and no payload or soft buffer touched"""
    L, capi = _lib(hiplib)
    ent = _multi_entries(L)
    n = len(ent)
    g = (capi.HipNrCwRx * n)(*[_rx(capi, t["i"], t["rv"], t["seed"], t["ne"], t["max_iter"]) for t in ent])
    outs = [np.full(t["tbs"] // 8 + GUARD, 0xEE, np.uint8) for t in ent]
    syms = (C.c_void_p * n)(*[t["y"].ctypes.data for t in ent])
    ces = (C.c_void_p * n)(*[t["h"].ctypes.data if t["h"] is not None else None for t in ent])
    sbs = (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(t["sb"].c) for t in ent])
    pays = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    # refused first, on untouched buffers
    snaps = [t["sb"].snapshot() for t in ent]
    bad = (capi.HipNrCwRx * n)(*g)
    bad[6].tb.nof_bits += 2
    res = (capi.HipNrTbResult * n)(*[capi.HipNrTbResult(7, 7, 7.0, 7) for _ in range(n)])
    assert L.srsran_hip_nr_cw_decode_multi(n, bad, syms, ces, sbs, pays, res) == capi.SRSRAN_ERROR_INVALID_INPUTS
    for k, t in enumerate(ent):
        assert (res[k].crc_ok, res[k].all_decoded, res[k].avg_iter, res[k].nof_cb) == (0, 0, 0.0, 0), k
        assert np.all(outs[k] == 0xEE) and t["sb"].same_as(snaps[k]), k
    assert L.srsran_hip_nr_cw_decode_multi(n, g, syms, ces, sbs, pays, res) == 0, capi.last_error()
    for k, t in enumerate(ent):
        _check_result(res[k], outs[k], t["tbs"], t["ok"], t["avg"], t["orc"], t["o_out"], ("multi", k))
        if k == 3:  # the stored first block is left as it was; the second one is stored now
            cb_bytes = (t["orc"].cfg.Kp - t["orc"].cfg.L_cb + 7) // 8
            assert t["sb"].flags[:2].all() and all(np.array_equal(t["sb"].keep[r][:cb_bytes], t["orc"].data[r][:cb_bytes]) for r in range(2))
        else:
            _check_state(t["sb"], t["orc"], ("multi", k))
    assert sum(int(t["orc"].crc.all()) for t in ent) >= 9


def _tx(capi, i, rv, seed, scaling):
    mod, n, tbs, R = SHAPES[i][0]
    return capi.HipNrCwTx(capi.HipNrTb(R, tbs, mod, rv, 1, n * QM[mod], 0, 0, 0, 0, 0), n, seed, scaling, 0)


@functools.lru_cache(maxsize=None)
def _tx_expected(i, rv, scaling):
    mod, n = SHAPES[i][0][:2]
    e = O.sch_nr_encode_tb(_cfg(i), rv, _payload(i))
    return O.modulate_bytes(mod, np.packbits(e), e.size, _seed(i), True, scaling)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_transmit(hiplib, i):
    """srsran_hip_nr_cw_encode = sch_nr_encode -> scrambling -> modulation: the oracle's points for every redundancy version, at scaling 1 and 0.5"""
    L, capi = _lib(hiplib)
    n, payload = SHAPES[i][0][1], _payload(i)
    for rv in range(4):
        for scaling in (1.0, 0.5):
            out = np.full(n + GUARD, 7 + 7j, np.complex64)
            g = _tx(capi, i, rv, _seed(i), scaling)
            assert L.srsran_hip_nr_cw_encode(C.byref(g), O.P(payload), O.P(out)) == 0, capi.last_error()
            want = _tx_expected(i, rv, scaling)
            assert np.array_equal(out[:n].view(np.uint32), want.view(np.uint32)) and np.all(out[n:] == 7 + 7j), (i, rv, scaling)


def test_transmit_multi_and_loopback(hiplib):
    """the codewords of a slot in one transmit call equal the single calls and the oracle; encode -> noise -> decode returns the payload"""
    L, capi = _lib(hiplib)
    order = [6, 0, 7, 3, 1, 5, 2, 4]
    n = len(order)
    g = (capi.HipNrCwTx * n)(*[_tx(capi, i, k % 4, _seed(i), 0.5 if k % 2 else 1.0) for k, i in enumerate(order)])
    outs = [np.full(SHAPES[i][0][1] + GUARD, 7 + 7j, np.complex64) for i in order]
    data = (C.c_void_p * n)(*[_payload(i).ctypes.data for i in order])
    syms = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    assert L.srsran_hip_nr_cw_encode_multi(n, g, data, syms) == 0, capi.last_error()
    for k, i in enumerate(order):
        nre = SHAPES[i][0][1]
        single = np.zeros(nre, np.complex64)
        assert L.srsran_hip_nr_cw_encode(C.byref(g[k]), O.P(_payload(i)), O.P(single)) == 0
        want = _tx_expected(i, k % 4, 0.5 if k % 2 else 1.0)
        assert np.array_equal(outs[k][:nre].view(np.uint32), want.view(np.uint32)) and np.array_equal(single.view(np.uint32), want.view(np.uint32)), (k, i)
        assert np.all(outs[k][nre:] == 7 + 7j)
    for i in (2, 7):  # loopback
        mod, nre, tbs, R = SHAPES[i][0]
        x = np.zeros(nre, np.complex64)
        gt = _tx(capi, i, 0, _seed(i), 1.0)
        assert L.srsran_hip_nr_cw_encode(C.byref(gt), O.P(_payload(i)), O.P(x)) == 0
        y = (x + _noise(np.random.default_rng(5 + i), nre, ESN0[mod])).astype(np.complex64)
        sb, out, res = Softbuffer(_cfg(i).C), np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
        gr = _rx(capi, i, NEW_DATA, _seed(i), 0.0)
        assert L.srsran_hip_nr_cw_decode(C.byref(gr), O.P(y), None, C.byref(sb.c), O.P(out), C.byref(res)) == 0
        assert res.crc_ok == 1 and res.all_decoded == 1 and np.array_equal(out[:tbs // 8], _payload(i)) and np.all(out[tbs // 8:] == 0xEE), i


def test_calls_from_worker_threads(hiplib):
    """three worker threads at once, each with its own staging context (taken from the pool srsran_hip_warmup fills): ten rounds of a receive and a
    transmit call per thread, every result equal to the one computed beforehand"""
    import threading

    L, capi = _lib(hiplib)
    assert L.srsran_hip_warmup(2) == 0
    work = []
    for t, i in enumerate((6, 3, 5)):
        (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
        payload, seed = _payload(i), _seed(i) + t
        y, h, ne = _rx_symbols(i, O.sch_nr_encode_tb(cfg, 0, payload), seed, ESN0[mod], np.random.default_rng(300 + t), "zf")
        orc = Oracle(cfg)
        o_out, ok, avg = orc.decode(0, _soft_bits(L, mod, y, h, ne, seed))
        assert orc.crc.all() and ok == 1
        work.append((i, seed, y, h, ne, avg, payload))
    errors = []

    def worker(i, seed, y, h, ne, avg, payload):
        try:
            assert L.srsran_hip_set_thread_device(0) == 0
            n, tbs = SHAPES[i][0][1], SHAPES[i][0][2]
            for _ in range(10):
                sb, out, res = Softbuffer(_cfg(i).C), np.full(tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult()
                g = _rx(capi, i, NEW_DATA, seed, ne)
                assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(y), O.P(h), C.byref(sb.c), O.P(out), C.byref(res)) == 0
                assert res.crc_ok == 1 and abs(res.avg_iter - avg) < 1e-6 and np.array_equal(out[:tbs // 8], payload) and sb.flags.all()
                pts = np.zeros(n, np.complex64)
                gt = _tx(capi, i, 0, _seed(i), 1.0)
                assert L.srsran_hip_nr_cw_encode(C.byref(gt), O.P(payload), O.P(pts)) == 0
                assert np.array_equal(pts.view(np.uint32), _tx_expected(i, 0, 1.0).view(np.uint32))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((i, repr(e)))

    for w in work:
        _tx_expected(w[0], 0, 1.0)  # computed once, before the threads start
    threads = [threading.Thread(target=worker, args=w) for w in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_refusals(hiplib):
    """every rule of the header returns negative and writes nothing (but zeroes the result)"""
    L, capi = _lib(hiplib)
    i = 5
    (mod, n, tbs, R), cfg = SHAPES[i][0], _cfg(i)
    y = O.qam_symbols(mod, n, 3)
    sb, out, e_out = Softbuffer(cfg.C), np.full(tbs // 8 + GUARD, 0xEE, np.uint8), np.full(n * QM[mod], 0x55, np.int8)
    sb.rows[0][:100] = 5
    snap = sb.snapshot()
    good = _rx(capi, i, 0, 1, 0.0)

    def refused(g, sym, soft, pay, want_res=True):
        res = capi.HipNrTbResult(7, 7, 7.0, 7)
        rc = L.srsran_hip_nr_cw_decode_dbg(C.byref(g) if g is not None else None, sym, None, C.byref(soft) if soft is not None else None, pay,
                                           C.byref(res) if want_res else None, O.P(e_out))
        assert rc < 0, rc
        assert not want_res or (res.crc_ok, res.all_decoded, res.avg_iter, res.nof_cb) == (0, 0, 0.0, 0)
        assert np.all(out == 0xEE) and np.all(e_out == 0x55) and sb.same_as(snap)

    refused(None, O.P(y), sb.c, O.P(out))
    refused(good, None, sb.c, O.P(out))
    refused(good, O.P(y), None, O.P(out))
    refused(good, O.P(y), sb.c, None)
    refused(good, O.P(y), sb.c, O.P(out), want_res=False)
    for m in (0, 5):  # BPSK and beyond 256-QAM
        g = _rx(capi, i, 0, 1, 0.0)
        g.tb.mod = m
        refused(g, O.P(y), sb.c, O.P(out))
    refused(_rx(capi, i, 0, 1, 0.0, nof_bits=n * QM[mod] - QM[mod]), O.P(y), sb.c, O.P(out))  # nof_bits != nof_re * Qm
    small = capi.SoftbufferRx(cfg.C - 1, SBW, sb.c.buffer_f, sb.c.data, sb.c.cb_crc, False)  # too few rows
    refused(good, O.P(y), small, O.P(out))
    short = capi.SoftbufferRx(cfg.C, _N(cfg) - 1, sb.c.buffer_f, sb.c.data, sb.c.cb_crc, False)  # rows too short
    refused(good, O.P(y), short, O.P(out))
    # more code blocks than the staging context takes: 54 codewords of three blocks
    k, cnt = 7, 54
    big_y = O.qam_symbols(4, SHAPES[k][0][1], 4)
    big_sb, big_out = Softbuffer(3), np.full(SHAPES[k][0][2] // 8, 0xEE, np.uint8)
    g = (capi.HipNrCwRx * cnt)(*[_rx(capi, k, NEW_DATA, 1, 0.0) for _ in range(cnt)])
    res = (capi.HipNrTbResult * cnt)()
    rc = L.srsran_hip_nr_cw_decode_multi(cnt, g, (C.c_void_p * cnt)(*[big_y.ctypes.data] * cnt), None,
                                         (C.POINTER(capi.SoftbufferRx) * cnt)(*[C.pointer(big_sb.c)] * cnt), (C.c_void_p * cnt)(*[big_out.ctypes.data] * cnt), res)
    assert rc < 0 and np.all(big_out == 0xEE) and not big_sb.flags.any() and not any(r.any() for r in big_sb.rows)
    # transmit side
    pts, pay = np.full(n, 7 + 7j, np.complex64), _payload(i)
    for g, d, s in ((None, O.P(pay), O.P(pts)), (_tx(capi, i, 0, 1, 1.0), None, O.P(pts)), (_tx(capi, i, 0, 1, 1.0), O.P(pay), None)):
        assert L.srsran_hip_nr_cw_encode(C.byref(g) if g is not None else None, d, s) < 0
    for field, value in (("mod", 0), ("mod", 5), ("nof_bits", n * QM[mod] + 1), ("rv", 4)):
        g = _tx(capi, i, 0, 1, 1.0)
        setattr(g.tb, field, value)
        assert L.srsran_hip_nr_cw_encode(C.byref(g), O.P(pay), O.P(pts)) < 0, field
    assert np.all(pts == 7 + 7j)
