"""The device Viterbi decoder and the PDCCH candidate call (include/srsran_amd/phy_conv_abi.h) through the C ABI, against what the reference gave
(tests/golden/conv_ref.npz) and against the model (tests/conv_model.py).  Every comparison is of integers or of float32 bit patterns: exact, no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

import conv_model as M
from test_conv_golden import KIND_F, KIND_S, KIND_US, p_cases, sweep_model, sweep_p_cases, sweep_v_cases, v_cases

pytestmark = pytest.mark.gpu
LEVEL = {72: 0, 144: 1, 288: 2, 576: 3}


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0
    return lib


def handle(L, framebits, tb, gain=0.0):
    from srslte_amd import capi

    q = capi.Viterbi()
    assert L.srsran_viterbi_init(C.byref(q), capi.SRSRAN_VITERBI_37, (C.c_int * 3)(*M.POLY), framebits, bool(tb)) == 0
    if gain > 0:
        L.srsran_viterbi_set_gain_quant(C.byref(q), gain)
    return q


@pytest.mark.parametrize("c", v_cases(), ids=lambda c: c["name"])
def test_handle_calls_give_the_recorded_bits(L, c):
    """decode_f / _s / _us as the case was recorded, and the recorded symbols straight in; the return value is framebits"""
    q = handle(L, c["framebits"], c["tb"], c["gain"])
    fn = {KIND_F: L.srsran_viterbi_decode_f, KIND_S: L.srsran_viterbi_decode_s, KIND_US: L.srsran_viterbi_decode_us}[c["kind"]]
    vin, sym = np.ascontiguousarray(c["vin"]), np.ascontiguousarray(c["sym"])
    data = np.full(c["L"] + 8, 0xEE, np.uint8)
    assert fn(C.byref(q), vin.ctypes.data, data.ctypes.data, c["L"]) == c["framebits"]
    assert np.array_equal(data[:c["L"]], c["bits"]) and np.all(data[c["L"]:] == 0xEE)
    data[:] = 0xEE
    assert L.srsran_viterbi_decode_us(C.byref(q), sym.ctypes.data, data.ctypes.data, c["L"]) == c["framebits"]
    assert np.array_equal(data[:c["L"]], c["bits"]) and np.all(data[c["L"]:] == 0xEE)
    L.srsran_viterbi_free(C.byref(q))


@pytest.mark.parametrize("tb", [1, 0], ids=["tail_biting", "tailed"])
def test_us_multi_gives_the_recorded_bits(L, tb):
    """every recorded frame of one kind of termination in one launch: frame lengths 32 .. 1000 side by side"""
    cases = [c for c in v_cases() if c["tb"] == tb]
    assert len(cases) >= 3
    q = handle(L, max(c["L"] for c in cases), tb)
    syms = [np.ascontiguousarray(c["sym"]) for c in cases]
    outs = [np.full(c["L"] + 8, 0xEE, np.uint8) for c in cases]
    n = len(cases)
    rc = L.srsran_hip_viterbi_decode_us_multi(C.byref(q), n, (C.c_void_p * n)(*[s.ctypes.data for s in syms]), (C.c_void_p * n)(*[o.ctypes.data for o in outs]),
                                              (C.c_uint32 * n)(*[c["L"] for c in cases]))
    assert rc == q.framebits
    for c, o in zip(cases, outs):
        assert np.array_equal(o[:c["L"]], c["bits"]) and np.all(o[c["L"]:] == 0xEE), c["name"]


def us_multi(L, q, syms, lengths):
    """srsran_hip_viterbi_decode_us_multi on the frames -> (rc, the output of each with 8 guard bytes of 0xEE behind it)"""
    n = len(syms)
    syms = [np.ascontiguousarray(s, np.uint16) for s in syms]
    outs = [np.full(n_bits + 8, 0xEE, np.uint8) for n_bits in lengths]
    rc = L.srsran_hip_viterbi_decode_us_multi(C.byref(q), n, (C.c_void_p * n)(*[s.ctypes.data for s in syms]), (C.c_void_p * n)(*[o.ctypes.data for o in outs]),
                                              (C.c_uint32 * n)(*lengths))
    return rc, outs


def sweep_frames(tb):
    """(case, its symbols) of the length sweep's frames with this termination, in the record's order; the symbols are M.quant_f of the recorded floats or the
    recorded uint16, which the generator proved to be the reference's"""
    V, model = sweep_v_cases(), sweep_model()[0]
    return [(c, m["sym"]) for c, m in zip(V, model) if c["tb"] == tb]


def test_sweep_tail_biting_lengths_through_decode_f(L):
    """every frame length 1 .. 144 with tail biting by srsran_viterbi_decode_f on a 144-bit handle: the max search and the quantiser at every 3 L % 64, the
    chain-back at every (2 L - 6) % 64 and with fewer words than bits (L <= 5)"""
    q = handle(L, 144, 1)
    frames = [(c, s) for c, s in sweep_frames(1) if c["kind"] == KIND_F]
    assert [c["L"] for c, _ in frames] == list(range(1, 145))
    bad = []
    for c, _ in frames:
        vin, data = np.ascontiguousarray(c["vin"]), np.full(c["L"] + 8, 0xEE, np.uint8)
        assert L.srsran_viterbi_decode_f(C.byref(q), vin.ctypes.data, data.ctypes.data, c["L"]) == 144, c["name"]
        if not (np.array_equal(data[:c["L"]], c["bits"]) and np.all(data[c["L"]:] == 0xEE)):
            bad.append(c["L"])
    L.srsran_viterbi_free(C.byref(q))
    assert not bad, "lengths that failed: %s" % bad


@pytest.mark.parametrize("framebits", [144, 2048])
def test_sweep_tail_biting_lengths_side_by_side(L, framebits):
    """the 144 frames in ONE launch on the model's symbols; on the 2048-bit handle the 2048-bit frame goes first, so every short frame is decoded in an LDS
    layout sized by the longest frame the library accepts"""
    frames = [(c, s) for c, s in sweep_frames(1) if c["L"] <= 144]
    assert len(frames) == 144
    if framebits == 2048:
        frames = [(c, s) for c, s in sweep_frames(1) if c["L"] == 2048] + frames
        assert len(frames) == 145 and frames[0][0]["L"] == 2048
    q = handle(L, framebits, 1)
    rc, outs = us_multi(L, q, [s for _, s in frames], [c["L"] for c, _ in frames])
    assert rc == framebits
    bad = [c["L"] for (c, _), o in zip(frames, outs) if not (np.array_equal(o[:c["L"]], c["bits"]) and np.all(o[c["L"]:] == 0xEE))]
    assert not bad, "lengths that failed: %s" % bad


def test_sweep_tailed_lengths(L):
    """the tailed lengths around the chain-back's blocks (63, 64, 65, 127, 128, ...) in one launch and each by itself through decode_us; the 2047-bit frame
    through decode_us on the 2048-bit handle"""
    frames = sweep_frames(0)
    short = [(c, s) for c, s in frames if c["L"] <= 144]
    assert {c["L"] for c, _ in short} >= {1, 5, 6, 7, 63, 64, 65, 127, 128, 129} and [c["L"] for c, _ in frames if c["L"] > 144] == [2047]
    q = handle(L, 144, 0)
    rc, outs = us_multi(L, q, [s for _, s in short], [c["L"] for c, _ in short])
    assert rc == 144
    bad = [c["L"] for (c, _), o in zip(short, outs) if not (np.array_equal(o[:c["L"]], c["bits"]) and np.all(o[c["L"]:] == 0xEE))]
    assert not bad, "lengths that failed in the multi launch: %s" % bad
    big = handle(L, 2048, 0)
    for c, s in frames:
        sym, data = np.ascontiguousarray(s), np.full(c["L"] + 8, 0xEE, np.uint8)
        h = big if c["L"] > 144 else q
        assert L.srsran_viterbi_decode_us(C.byref(h), sym.ctypes.data, data.ctypes.data, c["L"]) == h.framebits, c["name"]
        if not (np.array_equal(data[:c["L"]], c["bits"]) and np.all(data[c["L"]:] == 0xEE)):
            bad.append(c["L"])
    assert not bad, "lengths that failed through decode_us: %s" % bad


def run_pdcch(L, llr, cands, dbg=True):
    """-> (rc, results, rm rows, symbol rows)"""
    from srslte_amd import capi

    n = len(cands)
    llr = np.ascontiguousarray(llr, np.float32)
    cand = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*c) for c in cands])
    res = (capi.HipPdcchRes * n)()
    for r in res:
        C.memset(C.byref(r), 0x77, C.sizeof(r))
    rm, sym = np.full((n, capi.HIP_DCI_SYMS), 5.0, np.float32), np.full((n, capi.HIP_DCI_SYMS), 5, np.uint16)
    if dbg:
        rc = L.srsran_hip_pdcch_dci_decode_multi_dbg(llr.ctypes.data, llr.size, n, cand, res, rm.ctypes.data, sym.ctypes.data)
    else:
        rc = L.srsran_hip_pdcch_dci_decode_multi(llr.ctypes.data, llr.size, n, cand, res)
    return rc, res, rm, sym


def check_result(r, rm_row, sym_row, want, nof_bits, tag):
    """want: dict(rm, sym, bits, crc) of a decoded candidate, or None for one the mean rule skips"""
    n3 = 3 * (nof_bits + 16)
    payload = np.frombuffer(bytes(r.payload), np.uint8)
    if want is None:
        assert (r.decoded, r.crc_rem) == (0, 0) and not payload.any() and not rm_row.any() and not sym_row.any(), tag
        return
    assert r.decoded == 1 and r.crc_rem == want["crc"], (tag, hex(r.crc_rem), hex(want["crc"]))
    assert np.array_equal(payload[:nof_bits + 16], want["bits"]) and not payload[nof_bits + 16:].any(), tag
    assert rm_row[:n3].tobytes() == want["rm"].tobytes() and not rm_row[n3:].any(), tag
    assert np.array_equal(sym_row[:n3], want["sym"]) and not sym_row[n3:].any(), tag


def test_pdcch_cases_give_the_record(L):
    """every recorded candidate in ONE call on a region that holds them back to back (each on a CCE boundary): de-matched floats, quantised symbols, payload,
    crc_rem and decoded exact; then the same call without the debug rows gives the same results"""
    P = p_cases()
    first, parts = [], []
    for c in P:
        first.append(sum(p.size for p in parts) // 72)
        parts.append(c["llr"])
    llr = np.concatenate(parts)
    cands = [(first[i], LEVEL[c["E"]], c["nof_bits"]) for i, c in enumerate(P)]
    rc, res, rm, sym = run_pdcch(L, llr, cands)
    assert rc == 0
    for i, c in enumerate(P):
        assert np.float32(c["mean"]) == np.float32(res[i].mean), c["name"]
        check_result(res[i], rm[i], sym[i], dict(rm=c["rm"], sym=c["sym"], bits=c["bits"], crc=c["crc"]) if c["mean"] > 0.3 else None, c["nof_bits"], c["name"])
    assert sum(1 for c in P if c["mean"] <= 0.3) >= 2
    rc2, res2, _, _ = run_pdcch(L, llr, cands, dbg=False)
    assert rc2 == 0 and bytes(res2) == bytes(res)


def test_sweep_dci_lengths_in_one_call(L):
    """every DCI length 17 .. 144 -- every ndummy of the rate de-matcher with every E once -- back to back on CCE boundaries (480 CCE, 128 candidates) in ONE
    call: decoded, payload and crc_rem against the record, the mean against the model's, the de-matched floats and the symbols bit for bit the model's (which
    the generator held to the reference's), zeros behind 3 L; the plain call gives the same result bytes"""
    P, model = sweep_p_cases(), sweep_model()[1]
    first = np.concatenate([[0], np.cumsum([c["E"] // 72 for c in P])])
    assert len(P) == 128 and first[-1] == 480
    llr = np.concatenate([c["llr"] for c in P])
    cands = [(int(first[i]), LEVEL[c["E"]], c["nof_bits"]) for i, c in enumerate(P)]
    rc, res, rm, sym = run_pdcch(L, llr, cands)
    assert rc == 0
    bad = []
    for i, (c, m) in enumerate(zip(P, model)):
        try:
            assert np.float32(M.pdcch_mean(llr, cands[i][0], cands[i][1])) == np.float32(res[i].mean), c["name"]
            check_result(res[i], rm[i], sym[i], dict(rm=m["rm"], sym=m["sym"], bits=c["bits"], crc=c["crc"]), c["nof_bits"], c["name"])
        except AssertionError as e:
            bad.append((c["nof_bits"] + 16, str(e)[:120]))
    assert not bad, "lengths that failed: %s" % bad
    rc2, res2, _, _ = run_pdcch(L, llr, cands, dbg=False)
    assert rc2 == 0 and bytes(res2) == bytes(res)


def search_space():
    """a 25-PRB, CFI-3 control region (21 CCE) of noise with two encoded DCIs in it and one empty CCE; 22 locations (6 + 6 + 2 + 2 of a UE's search space, 4 + 2
    common ones) x 2 format sizes"""
    nof_cce, sizes = 21, (27, 31)
    rng = np.random.default_rng(77)
    llr = rng.standard_normal(72 * nof_cce).astype(np.float32)
    llr[72 * 20:] *= np.float32(0.05)  # nothing was sent on the last CCE: its level-0 candidate falls under the mean rule
    locs = []
    for lv, count, y in ((0, 6, 9), (1, 6, 4), (2, 2, 3), (3, 2, 1)):
        for m in range(count):
            locs.append((((y + m) % (nof_cce >> lv)) << lv, lv))
    locs += [(0, 2), (4, 2), (8, 2), (12, 2), (0, 3), (8, 3)]
    locs[5] = (20, 0)
    assert len(locs) == 22 and all(72 * n + (72 << lv) <= llr.size for n, lv in locs)
    placed = [((8, 1), 27, 0x1234), ((12, 2), 31, 0xFFFF)]
    assert all(loc in locs for loc, _, _ in placed)
    for (ncce, lv), nof_bits, rnti in placed:
        tx = M.dci_encode(rng.integers(0, 2, nof_bits), rnti, 72 << lv)
        llr[72 * ncce:72 * ncce + tx.size] = (2.0 * (2.0 * tx - 1.0) + 0.5 * rng.standard_normal(tx.size)).astype(np.float32)
    return llr, [(n, lv, s) for n, lv in locs for s in sizes], placed


@pytest.fixture(scope="module")
def space():
    llr, cands, placed = search_space()
    want = []
    for ncce, lv, nof_bits in cands:
        if M.pdcch_mean(llr, ncce, lv) > 0.3:
            m = M.dci_decode(llr[72 * ncce:72 * ncce + (72 << lv)], nof_bits)
            want.append(dict(rm=m["rm"], sym=m["sym"], bits=m["bits"], crc=m["crc_rem"]))
        else:
            want.append(None)
    return llr, cands, placed, want


def test_whole_search_space_in_one_call(L, space):
    llr, cands, placed, want = space
    assert len(cands) == 44 and sum(w is None for w in want) == 2
    rc, res, rm, sym = run_pdcch(L, llr, cands)
    assert rc == 0
    for i, (ncce, lv, nof_bits) in enumerate(cands):
        check_result(res[i], rm[i], sym[i], want[i], nof_bits, cands[i])
    for (ncce, lv), nof_bits, rnti in placed:  # the two that were sent decode to their RNTIs
        assert res[cands.index((ncce, lv, nof_bits))].crc_rem == rnti


def test_four_host_threads_give_the_same_bytes(L, space):
    llr, cands, _, _ = space
    rc, res, _, _ = run_pdcch(L, llr, cands, dbg=False)
    assert rc == 0
    got = [None] * 4

    def work(i):
        for _ in range(3):
            r = run_pdcch(L, llr, cands, dbg=False)
            got[i] = (r[0], bytes(r[1]))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(g == (0, bytes(res)) for g in got)
