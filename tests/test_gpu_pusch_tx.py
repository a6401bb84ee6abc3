"""PUSCH transmit with control information in one device call: srsran_hip_pusch_encode{,_dbg} and srsran_hip_ulsch_encode_uci (include/srsran_amd/phy_chan_abi.h).

Expected side: tests/pusch_tx_model.py, a literal restatement of srsran_ulsch_encode and srsran_pusch_encode's loops over the ACK / RI list (which
tests/test_pusch_tx_golden.py holds to the reference's own recorded bits), on the oracle's coded bits, sequence and constellation.  Bits and constellation
points are compared exactly, the precoded points within the transform's tolerance (tests/test_gpu_dft.py: 1e-4 relative to the output RMS, floor 1); the grid
outside the allocation must keep its guard values bit for bit.  The shapes are the smallest at which each branch of the kernel is live; one crosses a
workgroup's 2048 symbols.  Then the reference's recorded grants, the call without control information against srsran_hip_ulsch_encode, a loop-back through
srsran_hip_pusch_decode_uci and three worker threads at once."""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest

import oracle_api as O
import pusch_tx_model as M
from grant_helpers import _rx_softbuffer, _tx_softbuffer

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pusch_tx_ref.npz")
TOL = 1e-4
GUARD = np.complex64(7.25 - 3.5j)
RNTI, TTI, CELL_ID = 0x46, 7, 211


def _err(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.sqrt(np.mean(np.abs(b) ** 2))))


def _types(rng, pat, Qm, Q, is_ri=False):
    """Q Qm type bytes as the reference's encoders leave them ("rand": any type anywhere, which they never do)"""
    if Q == 0:
        return np.zeros(0, np.uint8)
    if pat == "1bit":
        return M.ack_ri_types([int(rng.integers(2))], 1, Qm, Q, is_ri=is_ri)
    if pat == "2bit":
        return M.ack_ri_types([int(rng.integers(2)), int(rng.integers(2))], 2, Qm, Q, is_ri=is_ri)
    if pat == "tdd1":
        return M.ack_ri_types([int(rng.integers(2))], 1, Qm, Q, N_bundle=2)
    if pat == "long":
        return M.long_ack_types(rng.integers(0, 2, 32), Qm, Q)
    assert pat == "rand"
    return rng.integers(0, 4, Q * Qm).astype(np.uint8)


# nof_prb, cp_nsymb, n_prb_tilde, L_prb, shortened, mod, tbs, (Q'ack, Q'ri, Q'cqi), ACK pattern, RI pattern
COUNTS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 3), (5, 3, 7)]
CASES = [(6, 7, (2, 3), 1, 0, mod, 40, cnt, "1bit", "1bit") for mod in (1, 2, 3) for cnt in COUNTS]
CASES += [
    (6, 7, (2, 3), 1, 0, 2, 40, (5, 3, 7), "2bit", "1bit"), (6, 7, (2, 3), 1, 0, 3, 40, (5, 3, 7), "2bit", "1bit"), (6, 7, (2, 3), 1, 0, 3, 40, (1, 0, 0), "2bit", "1bit"),
    (6, 7, (2, 3), 1, 0, 2, 40, (5, 3, 7), "tdd1", "1bit"), (6, 7, (2, 3), 1, 0, 3, 40, (5, 3, 7), "long", "1bit"),
    # extended CP: RI column 0 reaches row 0 -- the repetition at position 1 that the reference leaves alone
    (6, 6, (0, 5), 1, 0, 1, 40, (0, 48, 0), "1bit", "1bit"), (6, 6, (0, 5), 1, 0, 2, 40, (0, 48, 0), "1bit", "1bit"),
    # shortened, all four ACK columns full
    (6, 7, (1, 4), 2, 1, 3, 40, (96, 0, 0), "2bit", "1bit"), (6, 7, (1, 4), 2, 1, 1, 40, (96, 0, 0), "1bit", "1bit"),
    # extended and shortened: 9 columns (the <= 10 column sets)
    (6, 6, (3, 0), 3, 1, 2, 40, (7, 5, 11), "1bit", "1bit"),
    # two code blocks
    (15, 7, (1, 2), 12, 0, 3, 6200, (24, 5, 60), "2bit", "1bit"),
    # more than one workgroup (2160 symbols)
    (25, 7, (10, 0), 15, 0, 2, 6200, (24, 5, 60), "1bit", "1bit"),
    # any type at any bit, every ACK and RI column full up to row 0: a repetition in bit 0 of a symbol takes the last bit of the symbol before it
    (6, 7, (2, 3), 1, 0, 1, 40, (48, 48, 2), "rand", "rand"), (6, 7, (2, 3), 1, 0, 2, 40, (48, 48, 2), "rand", "rand"), (6, 7, (2, 3), 1, 0, 3, 40, (48, 48, 2), "rand", "rand"),
    (6, 6, (0, 5), 1, 0, 2, 40, (48, 48, 0), "rand", "rand"), (6, 6, (0, 5), 1, 1, 3, 40, (48, 48, 5), "rand", "rand"),
]


def _case_id(c):
    return "L%d_cp%d%s_mod%d_tbs%d_ack%d%s_ri%d%s_cqi%d" % (c[3], c[1], "_srs" if c[4] else "", c[5], c[6], c[7][0], c[8], c[7][1], c[9], c[7][2])


@functools.lru_cache(maxsize=None)
def _expected(idx, rv=0):
    """the model's stages for CASES[idx], computed once and only read"""
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, (Qa, Qr, Qc), apat, rpat = CASES[idx]
    rng = np.random.default_rng(9000 + idx)
    Qm = O.QM[mod]
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    H = cols * 12 * L_prb
    payload = rng.integers(0, 2, tbs).astype(np.uint8)
    ack, ri, cqi = _types(rng, apat, Qm, Qa), _types(rng, rpat, Qm, Qr, is_ri=True), rng.integers(0, 2, Qc * Qm).astype(np.uint8)
    seed = O.pusch_seed(RNTI, 2 * (TTI % 10), CELL_ID)
    e, _ = O.tb_coded_bits(tbs, Qm, (H - Qr - Qc) * Qm, rv, None, payload=payload, tx_order=True)
    m = M.pusch_encode(mod, e, cqi, ri, ack, cols, L_prb, seed)
    grid = np.full((2 * cp_nsymb, 12 * nof_prb), GUARD, np.complex64)
    M.put_grid(grid, m["z"], cp_nsymb, n_prb, L_prb, shortened)
    m.update(payload=payload, ack=ack, ri=ri, cqi=cqi, seed=seed, grid=grid.reshape(-1), cols=cols, H=H, Qm=Qm)
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


def _grant(capi, case, seed, rv=0):
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs = case[:7]
    cols = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    return capi.HipPuschTx(capi.HipGrantTb(mod, tbs, rv, cols * 12 * L_prb, seed, 0, 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened)


def _uci_in(capi, m):
    """the three arrays as the caller's memory (kept alive by the returned tuple)"""
    keep = tuple(np.array(m[k], np.uint8) for k in ("ack", "ri", "cqi"))
    return capi.HipPuschUciIn(*[a.ctypes.data if a.size else None for a in keep]), keep


def _encode_dbg(lib, capi, case, m, sb, payload_bytes, rv=0, pad=16):
    """srsran_hip_pusch_encode_dbg with guards behind every output: (q, d, z, grid)"""
    H, Qm = m["H"], m["Qm"]
    g = _grant(capi, case, m["seed"], rv)
    uci = capi.HipPuschUci(*case[7])
    uin, keep = _uci_in(capi, m)
    nq = H * Qm // 8
    q = np.full(nq + pad, 0xA5, np.uint8)
    d = np.full(H + pad, GUARD, np.complex64)
    z = np.full(H + pad, GUARD, np.complex64)
    grid = np.full(2 * case[1] * 12 * case[0] + pad, GUARD, np.complex64)
    rc = lib.srsran_hip_pusch_encode_dbg(C.byref(g), C.byref(uci), C.byref(uin), C.byref(sb), O.P(payload_bytes) if payload_bytes is not None else None, O.P(grid),
                                         O.P(q), O.P(d), O.P(z))
    assert rc == 0, capi.last_error()
    assert np.all(q[nq:] == 0xA5) and np.all(d[H:] == GUARD) and np.all(z[H:] == GUARD) and np.all(grid[-pad:] == GUARD)
    return q[:nq], d[:H], z[:H], grid[:-pad]


def _hold_to_model(m, q, d, z, grid):
    assert np.array_equal(np.unpackbits(q), m["q_tx"])
    assert np.array_equal(d.view(np.uint64), m["d"].view(np.uint64))  # a table look-up times nothing: bit-identical
    print("z err %.3g grid err %.3g" % (_err(z, m["z"].reshape(-1)), _err(grid, m["grid"])))
    assert _err(z, m["z"].reshape(-1)) < TOL
    inside = m["grid"] != GUARD
    assert np.array_equal(grid[~inside].view(np.uint64), m["grid"][~inside].view(np.uint64))  # outside the allocation: untouched
    assert inside.sum() == m["H"] and _err(grid[inside], m["grid"][inside]) < TOL
    assert np.array_equal(grid[inside].view(np.uint64), z.view(np.uint64))  # the grid holds the rows of z, in pusch_put's order


# ---- 1. parity with the model ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_pusch_encode_against_the_model(hiplib, idx):
    from srslte_amd import capi

    lib, case = hiplib, CASES[idx]
    m = _expected(idx)
    mod, tbs = case[5], case[6]
    sb, rows = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
    pay = np.packbits(m["payload"])
    q, d, z, grid = _encode_dbg(lib, capi, case, m, sb, pay)
    _hold_to_model(m, q, d, z, grid)
    # the plain call writes the same grid
    g = _grant(capi, case, m["seed"])
    uci = capi.HipPuschUci(*case[7])
    uin, keep = _uci_in(capi, m)
    grid2 = np.full(grid.size + 16, GUARD, np.complex64)
    assert lib.srsran_hip_pusch_encode(C.byref(g), C.byref(uci), C.byref(uin), C.byref(sb), O.P(pay), O.P(grid2)) == 0, capi.last_error()
    assert np.array_equal(grid2[:-16].view(np.uint64), grid.view(np.uint64)) and np.all(grid2[-16:] == GUARD)
    # srsran_ulsch_encode's level: unscrambled, placeholder and repetition bits as 0
    tb = capi.HipGrantTb(mod, tbs, 0, m["H"], m["seed"], 0, 0, 1)
    qb = np.full(m["H"] * m["Qm"] // 8 + 16, 0xA5, np.uint8)
    assert lib.srsran_hip_ulsch_encode_uci(C.byref(tb), m["cols"], C.byref(uci), C.byref(uin), C.byref(sb), O.P(pay), O.P(qb)) == 0, capi.last_error()
    assert np.array_equal(np.unpackbits(qb[:-16]), m["q_ulsch"]) and np.all(qb[-16:] == 0xA5)


def test_pusch_encode_retransmission_from_the_soft_buffer(hiplib):
    """rv 0 from `data`, then rv 2 with data == NULL: what the soft buffer holds is coded again (two code blocks, 64-QAM, 12 PRB)"""
    from srslte_amd import capi

    idx = next(i for i, c in enumerate(CASES) if c[3] == 12)
    case = CASES[idx]
    sb, rows = _tx_softbuffer(capi, O.cbsegm(case[6])["C"])
    m0, m2 = _expected(idx), _expected(idx, 2)
    _hold_to_model(m0, *_encode_dbg(hiplib, capi, case, m0, sb, np.packbits(m0["payload"])))
    _hold_to_model(m2, *_encode_dbg(hiplib, capi, case, m2, sb, None, rv=2))
    assert not np.array_equal(m0["q_tx"], m2["q_tx"])


# ---- 2. the reference's recorded grants ----------------------------------------------------------------------------------------------------------------------

def _recorded():
    return np.load(GOLDEN)


def test_ulsch_encode_uci_gives_the_reference_recorded_bits(hiplib):
    from srslte_amd import capi

    rec = _recorded()
    for i, (mod, tbs, rv, L_prb, nof_symb, Qa, Qr, Qc) in enumerate(rec["cases"].tolist()):
        Qm = O.QM[mod]
        H = nof_symb * 12 * L_prb
        types = rec["type_%d" % i]
        ri, ack = np.ascontiguousarray(types[:Qr * Qm]), np.ascontiguousarray(types[Qr * Qm:])
        cqi = np.ascontiguousarray(np.unpackbits(rec["cqi_%d" % i])[:Qc * Qm])
        assert ack.size == Qa * Qm and cqi.size == Qc * Qm
        uin = capi.HipPuschUciIn(ack.ctypes.data if Qa else None, ri.ctypes.data if Qr else None, cqi.ctypes.data if Qc else None)
        uci = capi.HipPuschUci(Qa, Qr, Qc)
        tb = capi.HipGrantTb(mod, tbs, rv, H, int(rec["seeds"][i]), 0, 0, 1)
        sb, rows = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
        pay = np.array(rec["pay_%d" % i], np.uint8)
        qb = np.full(H * Qm // 8 + 16, 0xA5, np.uint8)
        assert hiplib.srsran_hip_ulsch_encode_uci(C.byref(tb), nof_symb, C.byref(uci), C.byref(uin), C.byref(sb), O.P(pay), O.P(qb)) == 0, capi.last_error()
        assert np.array_equal(qb[:-16], rec["q_%d" % i]), str(rec["names"][i])
        assert np.all(qb[-16:] == 0xA5)


# ---- 3. no control information -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 12, 1, 40), (2, 11, 2, 40), (15, 12, 3, 6200), (3, 9, 2, 40)], ids=lambda s: "L%d_cols%d_mod%d_tbs%d" % s)
def test_all_counts_zero_is_ulsch_encode(hiplib, shape):
    from srslte_amd import capi

    L_prb, cols, mod, tbs = shape
    Qm, H = O.QM[mod], cols * 12 * L_prb
    rng = np.random.default_rng(77 + H)
    pay = rng.integers(0, 256, tbs // 8).astype(np.uint8)
    tb = capi.HipGrantTb(mod, tbs, 0, H, 1234, 0, 0, 1)
    got = []
    for uci in (None, capi.HipPuschUci(0, 0, 0), "plain"):
        sb, rows = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
        qb = np.full(H * Qm // 8 + 16, 0xA5, np.uint8)
        if uci == "plain":
            assert hiplib.srsran_hip_ulsch_encode(C.byref(tb), cols, C.byref(sb), O.P(pay), O.P(qb)) == 0, capi.last_error()
        else:
            assert hiplib.srsran_hip_ulsch_encode_uci(C.byref(tb), cols, C.byref(uci) if uci else None, None, C.byref(sb), O.P(pay), O.P(qb)) == 0, capi.last_error()
        got.append(qb)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[2]) and np.all(got[2][-16:] == 0xA5)


def test_pusch_encode_without_uci_argument(hiplib):
    """uci == NULL and in == NULL: the model without control information (the (0, 0, 0) case)"""
    from srslte_amd import capi

    idx = next(i for i, c in enumerate(CASES) if c[7] == (0, 0, 0) and c[5] == 2)
    case, m = CASES[idx], _expected(idx)
    sb, rows = _tx_softbuffer(capi, 1)
    g = _grant(capi, case, m["seed"])
    grid = np.full(m["grid"].size, GUARD, np.complex64)
    assert hiplib.srsran_hip_pusch_encode(C.byref(g), None, None, C.byref(sb), O.P(np.packbits(m["payload"])), O.P(grid)) == 0, capi.last_error()
    inside = m["grid"] != GUARD
    assert np.array_equal(grid[~inside].view(np.uint64), m["grid"][~inside].view(np.uint64)) and _err(grid[inside], m["grid"][inside]) < TOL


# ---- 4. loop-back through the receive call -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", [i for i, c in enumerate(CASES) if (c[3] == 12) or (c[3] == 1 and c[5] == 1 and c[7] == (5, 3, 7))], ids=lambda i: _case_id(CASES[i]))
def test_loop_back_through_pusch_decode_uci(hiplib, idx):
    """the grid srsran_hip_pusch_encode makes, identity channel estimates, no noise -> srsran_hip_pusch_decode_uci: the payload, and every control soft bit has
    the sign of the bit that was sent (a repetition after undoing its scrambling with the chips as uci.c:678-682 does, a placeholder as 1 ^ chip)"""
    from srslte_amd import capi
    from test_gpu_pusch_uci import _UciOut

    lib, case, m = hiplib, CASES[idx], _expected(idx)
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, (Qa, Qr, Qc) = case[:8]
    Qm, H = m["Qm"], m["H"]
    sbt, _ = _tx_softbuffer(capi, O.cbsegm(tbs)["C"])
    g = _grant(capi, case, m["seed"])
    uci = capi.HipPuschUci(Qa, Qr, Qc)
    uin, keep = _uci_in(capi, m)
    grid = np.zeros(2 * cp_nsymb * 12 * nof_prb, np.complex64)
    assert lib.srsran_hip_pusch_encode(C.byref(g), C.byref(uci), C.byref(uin), C.byref(sbt), O.P(np.packbits(m["payload"])), O.P(grid)) == 0, capi.last_error()
    ce = np.ones_like(grid)
    rx = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, H, m["seed"], 8, 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened, 0.01, 0)
    out = _UciOut(capi, Qm, Qa, Qr, Qc)
    sbr, rows, keep_r, flags = _rx_softbuffer(capi, O.cbsegm(tbs)["C"] + 1, np.int16)
    data = np.zeros(tbs // 8 + 16, np.uint8)
    res = capi.HipGrantRes()
    assert lib.srsran_hip_pusch_decode_uci(C.byref(rx), C.byref(uci), O.P(grid), O.P(ce), C.byref(sbr), O.P(data), C.byref(res), C.byref(out.c)) == 0, capi.last_error()
    assert res.crc_ok == 1
    assert np.array_equal(np.unpackbits(data[:tbs // 8]), m["payload"])
    ack_llr, ack_c, ack_pos, ri_llr, ri_c, ri_pos, cqi_llr = out.arrays()
    chips = O.sequence_bits(m["seed"], H * Qm)
    for llr, c, pos, types in ((ack_llr, ack_c, ack_pos, m["ack"]), (ri_llr, ri_c, ri_pos, m["ri"])):
        assert np.array_equal(c, chips[pos]) if pos.size else True
        for i in range(types.size):
            t, k = int(types[i]), i % Qm
            if t == M.UCI_BIT_PLACEHOLDER:
                want = 1 ^ int(c[i])
            elif t == M.UCI_BIT_REPETITION:  # the bit in front of it, scrambled with that bit's chip
                assert k >= 1 and int(types[i - 1]) < 2
                want = int(types[i - 1]) ^ int(chips[pos[i] - 1]) ^ int(c[i])
            else:
                want = t
            assert llr[i] != 0 and (llr[i] > 0) == (want == 1), (i, t, int(llr[i]))
    first = 1 if Qr > 0 else 0  # with RI symbols g[0] holds the soft bit of the highest RI position (phy_chan_abi.h)
    assert np.array_equal(cqi_llr[first:] > 0, m["cqi"][first:] == 1) and np.all(cqi_llr[first:] != 0)
    assert out.guards_intact()


# ---- 5. worker threads -----------------------------------------------------------------------------------------------------------------------------------------

def test_pusch_encode_from_worker_threads(hiplib):
    """three worker threads at once, each with its own grants, 6 rounds: every output is the single-threaded model's"""
    from srslte_amd import capi

    picks = [[i for i, c in enumerate(CASES) if c[7] == (5, 3, 7) and c[8] == "1bit" and c[5] == mod][0] for mod in (1, 2, 3)]
    big = [i for i, c in enumerate(CASES) if c[3] in (12, 15)]
    want = {i: _expected(i) for i in picks + big}

    def worker(tid, errors):
        try:
            mine = [picks[tid], big[tid % len(big)]]
            sbs = {i: _tx_softbuffer(capi, O.cbsegm(CASES[i][6])["C"]) for i in mine}
            for rnd in range(6):
                for i in mine:
                    _hold_to_model(want[i], *_encode_dbg(hiplib, capi, CASES[i], want[i], sbs[i][0], np.packbits(want[i]["payload"])))
        except BaseException as e:  # noqa: B902 -- carried to the main thread
            errors.append((tid, repr(e)))

    errors = []
    ths = [threading.Thread(target=worker, args=(t, errors)) for t in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
