"""PBCH / MIB decoding on the device (include/srsran_amd/phy_pbch_abi.h) through the C ABI, against what the reference gave (tests/golden/pbch_ref.npz,
tools/gen_golden_pbch.py).  Shapes are 6, 15 and 25 PRB.

The decode stage by itself is integer-exact: rm_f, the decoder's input symbols and the 40 bits of every combination of frame_idx 1 .. 4.  The calls run over
every recorded sequence with the state carried from call to call: return, ports, offset, payload, (src, dst, nb) and frame_idx exact; d and the soft-bit rows
within the tolerances the generator measured (max |a - b| / rms(b); four times the model's deviation from the reference) and showed to hide no wrong
decision; of the job rows, every combination the reference saw before its return has the reference's verdict (a miss, and the hit last).  The call that
estimates on the device equals srsran_hip_chest_dl_estimate followed by srsran_hip_pbch_decode bit for bit; eight cells in one launch equal the eight single
calls; four host threads give what each gives alone; and the capture of the reference's pbch_file_test decodes through the library alone."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle_api as O
import pbch_model as PB

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(O.ROOT, "tests", "golden", "pbch_ref.npz"))
SEQS = PB.record_sequences(GOLDEN)
D_TOL, LLR_TOL = float(GOLDEN["d_tol"]), float(GOLDEN["llr_tol"])


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0
    return lib


def rel(a, b):
    return float(np.abs(np.asarray(a).astype(np.complex128) - b).max()) / float(np.sqrt(np.mean(np.abs(np.asarray(b, np.complex128)) ** 2)))


def cell_struct(c):
    from srslte_amd import capi

    return capi.HipPbchCell(c["nof_prb"], c["nof_ports"], c["id"], c["cp_nsymb"])


def embed(c, rows):
    """a whole-subframe grid that holds the 4 x 72 recorded points where the channel lies and a value no call may read elsewhere"""
    g = np.full((2 * c["cp_nsymb"], 12 * c["nof_prb"]), np.nan + 1j * np.nan, np.complex64)
    k0 = c["nof_prb"] * 6 - 36
    g[c["cp_nsymb"]:c["cp_nsymb"] + 4, k0:k0 + 72] = rows
    return np.ascontiguousarray(g.reshape(-1))


def state_struct(c, st):
    from srslte_amd import capi

    s = capi.HipPbchState()
    s.frame_idx = st["frame_idx"]
    flat = np.zeros(4 * 480, np.float32)
    nof_bits = 2 * PB.nof_re(c)
    flat[:4 * nof_bits] = st["llr"].reshape(-1)
    C.memmove(s.llr, flat.ctypes.data, flat.nbytes)
    return s


def state_rows(c, s):
    nof_bits = 2 * PB.nof_re(c)
    return np.ctypeslib.as_array(s.llr)[:4 * nof_bits].reshape(4, nof_bits).copy()


class Planes:
    def __init__(self, c, call):
        self.rx = embed(c, call["rx_rows"])
        self.ce = [embed(c, r) for r in call["ce_rows"]]
        self.ptr = (C.c_void_p * 4)(*([g.ctypes.data for g in self.ce] + [None] * (4 - len(self.ce))))
        self.noise = float(call["noise"])


def decode(L, c, state, pl, dbg=False):
    """-> (res, dbg outputs or None); the state struct is advanced"""
    from srslte_amd import capi

    cs, res = cell_struct(c), capi.HipPbchRes()
    if not dbg:
        assert L.srsran_hip_pbch_decode(C.byref(cs), C.byref(state), pl.rx.ctypes.data, pl.ptr, C.c_float(pl.noise), C.byref(res)) == 0
        return res, None
    d, llr_new, rows, n = np.full(3 * 240 + 4, 77.0, np.complex64), np.full(3 * 480 + 4, 77.0, np.float32), (capi.HipPbchRow * 91)(), C.c_uint32(0)
    C.memset(rows, 0x77, C.sizeof(rows))
    assert L.srsran_hip_pbch_decode_dbg(C.byref(cs), C.byref(state), pl.rx.ctypes.data, pl.ptr, C.c_float(pl.noise), C.byref(res), d.ctypes.data, llr_new.ctypes.data,
                                        rows, C.byref(n)) == 0
    assert np.all(d[720:] == 77.0) and np.all(llr_new[1440:] == 77.0) and bytes(rows[90]) == b"\x77" * 48
    return res, dict(d=d[:720].reshape(3, 240), llr_new=llr_new[:1440].reshape(3, 480), rows=rows, n=n.value)


def res_tuple(res):
    return (res.ret, res.nof_tx_ports, res.sfn_offset, res.src, res.dst, res.nb, bytes(res.payload))


def want_tuple(call):
    return (int(call["ret"]), int(call["ports"]), int(call["off"]), int(call["comb"][2]), int(call["comb"][1]), int(call["comb"][0]), bytes(call["payload"]))


# ---------------------------------------------------------------------------------------------------------------- the decode stage
@pytest.mark.parametrize("i", range(len(GOLDEN["t_names"])), ids=lambda i: str(GOLDEN["t_names"][i]))
def test_try_frames_is_bit_exact(L, i):
    from srslte_amd import capi

    c, f, llr = PB.from_row(GOLDEN["t_cell_%d" % i]), int(GOLDEN["t_f_%d" % i]), GOLDEN["t_llr_%d" % i]
    n = len(PB.combos(f))
    flat = np.ascontiguousarray(llr.reshape(-1))
    rows, rm, sym = (capi.HipPbchRow * (n + 1))(), np.full((n + 1, 120), 77.0, np.float32), np.full((n + 1, 120), 77, np.uint16)
    C.memset(rows, 0x77, C.sizeof(rows))
    cs = cell_struct(c)
    assert L.srsran_hip_pbch_try_frames_dbg(C.byref(cs), flat.ctypes.data, f, rows, rm.ctypes.data, sym.ctypes.data) == n
    assert bytes(rows[n]) == b"\x77" * 48 and np.all(rm[n] == 77.0) and np.all(sym[n] == 77)
    import conv_model as CM

    for j in range(n):
        assert np.array_equal(rm[j].view(np.uint32), GOLDEN["t_rm_f_%d" % i][j].view(np.uint32)), j
        assert np.array_equal(sym[j], CM.quant_f(GOLDEN["t_rm_f_%d" % i][j])), j
        assert np.array_equal(np.array(rows[j].bits, np.uint8), GOLDEN["t_data_%d" % i][j]), j
        hit = rows[j].crc_rem == PB.CRC_MASK[1] and rows[j].ones != 0
        assert hit == bool(GOLDEN["t_hit_%d" % i][j]) and rows[j].ones == int(GOLDEN["t_data_%d" % i][j][:24].sum()) and rows[j].zero == 0, j
    plain = (capi.HipPbchRow * n)()
    assert L.srsran_hip_pbch_try_frames(C.byref(cs), flat.ctypes.data, f, plain) == n and bytes(plain) == bytes(rows)[:48 * n]


# ---------------------------------------------------------------------------------------------------------------- the call
@pytest.mark.parametrize("s", SEQS, ids=lambda s: s["name"])
def test_decode_over_the_recorded_sequences(L, s):
    c = s["cell"]
    state = state_struct(c, PB.new_state(c))
    nants = PB.nant_list(c)
    for i, call in enumerate(s["calls"]):
        tag = (s["name"], i)
        f = state.frame_idx + 1
        assert state.frame_idx == int(call["f_in"]), tag
        before = state_struct(c, dict(frame_idx=state.frame_idx, llr=state_rows(c, state)))
        pl = Planes(c, call)
        res, o = decode(L, c, state, pl, dbg=True)
        assert res_tuple(res) == want_tuple(call), tag
        assert state.frame_idx == int(call["f_out"]), tag
        rows_now = state_rows(c, state)
        for r in range(int(call["f_out"])):
            assert rel(rows_now[r], call["llr"][r]) <= LLR_TOL, (tag, r)
        k = nants.index(int(call["d_nant"]))
        nre = PB.nof_re(c)
        dev_d = rel(o["d"][k][:nre], call["d"])
        print("%s call %d: d %.3g (tol %.3g)" % (s["name"], i, dev_d, D_TOL))
        assert dev_d <= D_TOL, tag
        # the job rows: hypothesis by hypothesis, the combinations in the reference's order; those it saw before its return are misses, the hit is last
        combos = PB.combos(f)
        assert o["n"] == len(nants) * len(combos), tag
        verdicts = [(nant, cmb, o["rows"][h * len(combos) + j].crc_rem == PB.CRC_MASK[nant] and o["rows"][h * len(combos) + j].ones != 0)
                    for h, nant in enumerate(nants) for j, cmb in enumerate(combos)]
        if call["ret"]:
            at = [(nant, cmb) for nant, cmb, _ in verdicts].index((int(call["ports"]), tuple(int(v) for v in call["comb"])))
            assert not any(v for _, _, v in verdicts[:at]) and verdicts[at][2], tag
            assert bytes(o["rows"][at].bits)[:24] == bytes(call["payload"]), tag
        else:
            assert not any(v for _, _, v in verdicts), tag
        # the plain form from the same state: the same result and state, bit for bit
        res2, _ = decode(L, c, before, pl)
        assert bytes(res2) == bytes(res) and bytes(before) == bytes(state), tag
        # the newest row kept is the LAST hypothesis's
        if not call["ret"]:
            assert np.array_equal(rows_now[int(call["f_out"]) - 1 if f < 4 else 2][:2 * nre], o["llr_new"][len(nants) - 1][:2 * nre]), tag


# ---------------------------------------------------------------------------------------------------------------- from the received grids alone
def est_struct(c, pilots, nof_rx=1):
    from srslte_amd import capi

    est = capi.HipChestDl()
    est.nof_prb, est.nof_ports, est.id, est.cp_nsymb, est.nof_rx, est.sf_idx = c["nof_prb"], c["nof_ports"] or 4, c["id"], c["cp_nsymb"], nof_rx, 0
    est.estimator_alg, est.noise_alg, est.filter_type = 0, 0, 0  # srsran_chest_dl_estimate's zeroed configuration
    keep = [np.ascontiguousarray(p) for p in pilots]
    est.pilots[0], est.pilots[1] = keep[0].ctypes.data, keep[1].ctypes.data
    return est, keep


def decode_est(L, c, state, est, rx):
    from srslte_amd import capi

    cs, res, out, es = cell_struct(c), capi.HipPbchRes(), capi.HipChestDlRes(), capi.HipChestDlState()
    y = (C.c_void_p * 4)(rx.ctypes.data, None, None, None)
    assert L.srsran_hip_pbch_decode_est(C.byref(cs), C.byref(est), C.byref(es), C.byref(state), y, C.byref(res), C.byref(out)) == 0
    return res, out


def two_steps(L, c, state, est, rx):
    """srsran_hip_chest_dl_estimate, then srsran_hip_pbch_decode"""
    from srslte_amd import capi

    ports = c["nof_ports"] or 4
    out, es, res = capi.HipChestDlRes(), capi.HipChestDlState(), capi.HipPbchRes()
    ce = [np.zeros(rx.size, np.complex64) for _ in range(ports)]
    y = (C.c_void_p * 4)(rx.ctypes.data, None, None, None)
    rows = [[ce[p].ctypes.data, None, None, None] if p < ports else [None] * 4 for p in range(4)]
    h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*r) for r in rows])
    assert L.srsran_hip_chest_dl_estimate(C.byref(est), C.byref(es), y, h, C.byref(out)) == 0
    ptr = (C.c_void_p * 4)(*([g.ctypes.data for g in ce] + [None] * (4 - ports)))
    cs = cell_struct(c)
    assert L.srsran_hip_pbch_decode(C.byref(cs), C.byref(state), rx.ctypes.data, ptr, C.c_float(out.noise_estimate), C.byref(res)) == 0
    return res, out


@pytest.mark.parametrize("s", [s for s in SEQS if s["full"]], ids=lambda s: s["name"])
def test_decode_est_is_the_two_steps_and_the_record(L, s):
    c = s["cell"]
    est, keep = est_struct(c, s["pilots"])
    a, b = state_struct(c, PB.new_state(c)), state_struct(c, PB.new_state(c))
    for i, call in enumerate(s["calls"]):
        rx = np.ascontiguousarray(call["rx"])
        res, out = decode_est(L, c, a, est, rx)
        res2, out2 = two_steps(L, c, b, est, rx)
        assert bytes(res) == bytes(res2) and bytes(a) == bytes(b) and bytes(out) == bytes(out2), (s["name"], i)
        assert res_tuple(res) == want_tuple(call) and a.frame_idx == int(call["f_out"]), (s["name"], i)
        assert abs(out.noise_estimate - float(call["noise"])) <= 1e-3 * float(call["noise"]), (s["name"], i)


# ---------------------------------------------------------------------------------------------------------------- several cells, several threads
def picked_calls():
    """eight recorded calls at different frame_idx, with mixed port counts and both prefixes: (sequence, call)"""
    by = {s["name"]: s for s in SEQS}
    pick = [("noise4_told0", 3), ("hi_4p_told4", 0), ("ext_1p", 0), ("low_start1", 1), ("noise6_then_2p", 6), ("low_start3", 2), ("hi_1p_told0", 0), ("noise6_then_2p", 2)]
    out = [(by[n], i) for n, i in pick]
    assert len({int(s["calls"][i]["f_in"]) for s, i in out}) == 4 and {s["cell"]["cp_nsymb"] for s, _ in out} == {6, 7}
    assert {s["cell"]["nof_ports"] for s, _ in out} == {0, 1, 2, 4}
    return out


def single_calls(L, picked):
    out = []
    for s, i in picked:
        c = s["cell"]
        st = state_struct(c, PB.state_before(c, s, i))
        res, _ = decode(L, c, st, Planes(c, s["calls"][i]))
        assert res_tuple(res) == want_tuple(s["calls"][i]), (s["name"], i)
        out.append((bytes(res), bytes(st)))
    return out


def test_decode_multi_of_eight_cells_is_the_eight_single_calls(L):
    from srslte_amd import capi

    picked = picked_calls()
    alone = single_calls(L, picked)
    for n in (8, 3, 1):
        cells = (capi.HipPbchCell * n)(*[cell_struct(s["cell"]) for s, _ in picked[:n]])
        states = [state_struct(s["cell"], PB.state_before(s["cell"], s, i)) for s, i in picked[:n]]
        sp = (C.POINTER(capi.HipPbchState) * n)(*[C.pointer(st) for st in states])
        planes = [Planes(s["cell"], s["calls"][i]) for s, i in picked[:n]]
        rx = (C.c_void_p * n)(*[p.rx.ctypes.data for p in planes])
        ce = ((C.c_void_p * 4) * n)(*[p.ptr for p in planes])
        noise = (C.c_float * n)(*[p.noise for p in planes])
        res = (capi.HipPbchRes * (n + 1))()
        C.memset(res, 0x77, C.sizeof(res))
        assert L.srsran_hip_pbch_decode_multi(n, cells, sp, rx, ce, noise, res) == 0
        assert bytes(res[n]) == b"\x77" * 48
        for k in range(n):
            assert (bytes(res[k]), bytes(states[k])) == alone[k], (n, k)


def test_four_host_threads_with_different_cells(L):
    picked = picked_calls()[:4]
    alone = single_calls(L, picked)
    got, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = single_calls(L, [picked[k]])[0]
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == alone


# ---------------------------------------------------------------------------------------------------------------- the known answer, through the library alone
@pytest.mark.parametrize("told", (2, 0))
def test_the_capture_decodes_through_the_library_alone(L, told):
    """the first 1920 samples of the reference's pbch_file_test capture -> srsran_ofdm_rx_sf (6 PRB) -> srsran_hip_pbch_decode_est with cell 150:
    2 ports, offset 0, the MIB of pbch_file_test.c:45-46"""
    from srslte_amd import capi

    x = np.load(os.path.join(O.ROOT, "tests", "golden", "sync_captures.npz"))["pbch_1_92M_x"][:1920]
    bin_, grid = np.zeros(1920, np.complex64), np.zeros(14 * 72, np.complex64)
    q, cfg = capi.Ofdm(), capi.OfdmCfg()
    cfg.nof_prb, cfg.in_buffer, cfg.out_buffer, cfg.cp = 6, bin_.ctypes.data, grid.ctypes.data, capi.CP_NORM
    assert L.srsran_ofdm_rx_init_cfg(C.byref(q), C.byref(cfg)) == 0
    bin_[:] = x  # behind the initialisation, which zeroes the input buffer as the reference's does
    L.srsran_ofdm_rx_sf(C.byref(q))
    L.srsran_ofdm_rx_free(C.byref(q))
    s = [s for s in SEQS if s["name"] == "capture_told%d" % told][0]
    c = s["cell"]
    assert c == PB.cell(6, told, 150) and rel(grid, s["calls"][0]["rx"]) < 1e-4
    est, keep = est_struct(c, s["pilots"])
    state = state_struct(c, PB.new_state(c))
    res, out = decode_est(L, c, state, est, grid)
    assert (res.ret, res.nof_tx_ports, res.sfn_offset) == (1, 2, 0) and state.frame_idx == 0
    assert "".join(str(b) for b in res.payload) == "011010000001110000000000"
    assert res_tuple(res) == want_tuple(s["calls"][0])
    v = [C.c_uint32() for _ in range(4)]
    L.srsran_hip_pbch_mib_unpack(res.payload, *[C.byref(t) for t in v])
    assert [t.value for t in v] == [50, 0, 2, 28]
