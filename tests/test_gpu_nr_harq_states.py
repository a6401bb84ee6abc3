"""The HARQ soft-buffer protocol of the two NR receive entry points that take the reference's srsran_softbuffer_rx_t -- srsran_hip_nr_cw_decode (one codeword,
soft bits made on the device) and srsran_hip_sch_nr_decode_tb (one transport block, soft bits from the caller) -- driven through ONE table of soft-buffer
states and held to the oracle's sch_nr_decode on its own buffers.

Shape: the three-block 256-QAM codeword of test_gpu_nr_cw.SHAPES (Z 384), the smallest in which the range of rows [first, last] that one copy moves can
hold a block of the other kind in its middle.  A state is a pattern over the three blocks: D = decoded and stored (flag set, packed bits in data[r]; its
row keeps the stale soft bits it held when it decoded), S = undecoded with the soft bits of a failed first transmission in its row; "clean" = the buffer as
srsran_softbuffer_rx_reset leaves it.  The retransmission (rv 2) carries the bits of the undecoded blocks back to back from the start of the codeword
(sch_nr.c:584-656) at two levels: WEAK (8 dB: no further block decodes -- asserted --, so the rows combine and come back) and STRONG (26 dB: every block
decodes -- asserted --, so the flags and data[r] are written).  On the clean buffer rv 2 is a first transmission without the systematic bits: at either
level the decoder settles on the all-zero word, which sch_nr.c:633-639 does not count as decoded, so there the precondition is "no block decodes" twice.
Both entry points get the same soft bits and the same expectation, computed once."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import oracle_api as O
from test_gpu_nr_cw import (DS, GUARD, MAX_ITER, NEW_DATA, SBW, SCALING, SHAPES, Oracle, Softbuffer, _cfg, _check_result, _check_state, _lib, _payload, _rx,
                            _rx_symbols, _seed, _soft_bits)

pytestmark = pytest.mark.gpu

I = 7  # (4, 4133, 25104, 0.76): three code blocks of Z 384, two sizes of E
STATES = ["clean", "SSS", "DSS", "SDS", "SSD", "DSD", "DDD"]
LEVELS = {"weak": 8.0, "strong": 26.0}


@functools.lru_cache(maxsize=None)
def _first_transmission():
    """(payload, the stored blocks of a strong-LLR decode, the rows a first transmission at 14 dB leaves with no block decoded)"""
    (mod, n, tbs, R), cfg = SHAPES[I][0], _cfg(I)
    assert cfg.C == 3
    payload, seed = _payload(I, 5), _seed(I) + 40
    e0 = O.sch_nr_encode_tb(cfg, 0, payload)
    clean = Oracle(cfg)
    clean.decode(0, (20 * (1 - 2 * e0.astype(np.int16))).astype(np.int8))
    assert clean.crc.all()
    y0, _, _ = _rx_symbols(I, e0, seed, 14.0, np.random.default_rng(4100), "none")
    dirty = Oracle(cfg)
    dirty.decode(0, _soft_bits(None, mod, y0, None, 0.0, seed))
    assert not dirty.crc.any(), dirty.crc  # precondition: the first transmission leaves every block undecoded
    return payload, clean.data.copy(), dirty.soft.copy()


def _state(pattern):
    """(library-side soft buffer, oracle) in the state `pattern`"""
    cfg = _cfg(I)
    _, stored, rows = _first_transmission()
    sb, orc, cb_bytes = Softbuffer(cfg.C + 1), Oracle(cfg), (cfg.Kp - cfg.L_cb + 7) // 8
    for r, kind in enumerate("" if pattern == "clean" else pattern):
        sb.rows[r][:SBW] = orc.soft[r] = rows[r]
        if kind == "D":
            orc.crc[r], orc.data[r] = 1, stored[r]
            sb.flags[r] = True
            sb.keep[r][:cb_bytes] = stored[r][:cb_bytes]
    return sb, orc


@functools.lru_cache(maxsize=None)
def _case(pattern, level, new_data=False):
    """symbols and soft bits of the transmission, and what the oracle makes of it on the state: dict(y, e, rv, before, orc, o_out, ok, avg)"""
    (mod, n, tbs, R), cfg = SHAPES[I][0], _cfg(I)
    payload, seed = _first_transmission()[0], _seed(I) + 40
    rng = np.random.default_rng(4200 + 10 * STATES.index(pattern) + list(LEVELS).index(level))
    _, orc = _state(pattern)
    before = orc.crc.copy()
    if new_data:  # every block is transmitted and every row overwritten: the oracle on a reset buffer
        rv, orc = 0, Oracle(cfg)
        bits = O.sch_nr_encode_tb(cfg, rv, payload)
    else:
        rv = 2
        e2, off = O.sch_nr_encode_tb(cfg, rv, payload), np.cumsum([0] + [O.sch_nr_get_E(cfg, r) for r in range(cfg.C)])
        left = [e2[off[r]:off[r + 1]] for r in range(cfg.C) if not before[r]]
        n_left = sum(x.size for x in left)
        bits = np.concatenate(left + [rng.integers(0, 2, e2.size - n_left).astype(np.uint8)])  # (nothing reads behind the undecoded blocks' bits)
    y, _, _ = _rx_symbols(I, bits, seed, LEVELS[level], rng, "none")
    e = _soft_bits(None, mod, y, None, 0.0, seed)
    o_out, ok, avg = orc.decode(rv, e)
    if level == "weak" or pattern == "clean":
        assert np.array_equal(orc.crc, np.zeros(cfg.C, np.uint8) if new_data else before), (pattern, level, orc.crc)  # precondition: no further block decodes
    else:
        assert orc.crc.all() and ok == 1 and np.array_equal(o_out, payload), (pattern, level, orc.crc, ok)  # precondition: the transport block completes
    return dict(y=y, e=e, rv=rv, before=before, orc=orc, o_out=o_out, ok=ok, avg=avg)


def _run(hiplib, entry, pattern, level, new_data=False):
    L, capi = _lib(hiplib)
    tbs, cfg = SHAPES[I][0][2], _cfg(I)
    t, tag = _case(pattern, level, new_data), (entry, pattern, level, new_data)
    sb, _ = _state(pattern)
    stale = [sb.rows[r].copy() for r in range(cfg.C)]
    out = np.full(tbs // 8 + GUARD, 0xEE, np.uint8)
    if entry == "cw":
        res = capi.HipNrTbResult()
        g = _rx(capi, I, t["rv"] | (NEW_DATA if new_data else 0), _seed(I) + 40, 0.0)
        assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(t["y"]), None, C.byref(sb.c), O.P(out), C.byref(res)) == 0, (tag, capi.last_error())
    else:
        fn = L.srsran_hip_sch_nr_decode_tb
        fn.restype, fn.argtypes = C.c_int, [C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        mod, n, _, R = SHAPES[I][0]
        tb = capi.HipNrTb(R, tbs, mod, t["rv"], 1, t["e"].size, 0, 0, 0, 0, 0)
        crc, avg = C.c_bool(False), C.c_float(-1)
        assert fn(SCALING, MAX_ITER, C.byref(tb), O.P(t["e"]), C.byref(sb.c), O.P(out), C.byref(crc), C.byref(avg)) == 0, (tag, capi.last_error())
        # (this call reports neither: the block count is the configuration's, "all decoded" is what the flags -- held to the oracle's below -- say)
        res = types.SimpleNamespace(nof_cb=cfg.C, all_decoded=int(sb.flags[:cfg.C].all()), crc_ok=int(crc.value), avg_iter=avg.value)
    _check_result(res, out, tbs, t["ok"], t["avg"], t["orc"], t["o_out"], tag)
    _check_state(sb, t["orc"], tag)
    for r in range(cfg.C):
        if t["before"][r] and not new_data:  # a block decoded earlier: flag and stored bits as they were (checked above), and its stale row not written
            assert np.array_equal(sb.rows[r], stale[r]), (tag, r)


@pytest.mark.parametrize("level", list(LEVELS))
@pytest.mark.parametrize("pattern", STATES)
@pytest.mark.parametrize("entry", ["cw", "tb"])
def test_soft_buffer_states(hiplib, entry, pattern, level):
    """every state of the table through both entry points: flags, stored blocks, rows, iteration average, payload and CRC equal the oracle's; nothing behind a
    row's N entries, a stored block or the payload is written; the row of a block decoded earlier is left alone"""
    _run(hiplib, entry, pattern, level)


@pytest.mark.parametrize("pattern", ["DSS", "SSS"])
def test_new_data_flag_resets_the_state(hiplib, pattern):
    """SRSRAN_HIP_NR_TB_NEW_DATA on a used soft buffer (the codeword call has the flag): a transmission in which nothing decodes leaves what the oracle leaves
    on a reset buffer -- the earlier flag cleared, the rows overwritten instead of combined"""
    _run(hiplib, "cw", pattern, "weak", new_data=True)
