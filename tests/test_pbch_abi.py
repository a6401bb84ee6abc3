"""CPU-only checks of the PBCH entry points (include/srsran_amd/phy_pbch_abi.h), in the manner of test_ctrl_abi.py: the library exports them and the ctypes
mirror binds them, the structs have the declared sizes in the header and in the mirror, a plain C caller compiles under -Wall -Werror, srsran_hip_pbch_nof_re
/ _table equal the record's map cases (tests/golden/pbch_ref.npz) and the model (tests/pbch_model.py), srsran_hip_pbch_mib_unpack reads the recorded
payloads as the model does, every refusal comes before the device is looked for with one line on stderr, zeroed results and an untouched state, and a valid
call without a device fails loudly.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import pbch_model as PB
from test_conv_abi import _compile_run, _one_line

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_pbch_nof_re", "srsran_hip_pbch_table", "srsran_hip_pbch_mib_unpack", "srsran_hip_pbch_try_frames", "srsran_hip_pbch_try_frames_dbg",
           "srsran_hip_pbch_decode", "srsran_hip_pbch_decode_dbg", "srsran_hip_pbch_decode_est", "srsran_hip_pbch_decode_est_dbg", "srsran_hip_pbch_decode_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pbch_ref.npz"))


def cell_struct(capi, c):
    return capi.HipPbchCell(c["nof_prb"], c["nof_ports"], c["id"], c["cp_nsymb"])


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_struct_sizes_in_header_and_mirror():
    from srslte_amd import capi

    items = ["sizeof(srsran_hip_pbch_cell_t)", "sizeof(srsran_hip_pbch_state_t)", "offsetof(srsran_hip_pbch_state_t, llr)", "sizeof(srsran_hip_pbch_res_t)",
             "offsetof(srsran_hip_pbch_res_t, payload)", "sizeof(srsran_hip_pbch_row_t)", "offsetof(srsran_hip_pbch_row_t, crc_rem)",
             "offsetof(srsran_hip_pbch_row_t, ones)", "SRSRAN_HIP_PBCH_MAX_ROWS", "SRSRAN_HIP_PBCH_MAX_CELLS"]
    src = ('#include "srsran_amd/phy_pbch_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("pbch_layout", src, os.path.join(ROOT, "include")).split()]
    assert got == [16, 7684, 4, 48, 24, 48, 40, 42, 90, 8]
    S, R, W = capi.HipPbchState, capi.HipPbchRes, capi.HipPbchRow
    assert [C.sizeof(capi.HipPbchCell), C.sizeof(S), S.llr.offset, C.sizeof(R), R.payload.offset, C.sizeof(W), W.crc_rem.offset, W.ones.offset] == got[:8]


def test_header_takes_a_plain_c_callers_arrays():
    """a C caller that holds the arrays a caller of srsran_ue_mib_decode holds compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_pbch_abi.h"\n#include <stddef.h>\n'
           "int take(const srsran_hip_pbch_cell_t* cell, srsran_hip_pbch_state_t* st, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* es,\n"
           "         srsran_hip_pbch_row_t* rows, float* f, uint16_t* us) {\n"
           "  cf_t* sf_symbols[SRSRAN_MAX_PORTS] = {NULL}; const cf_t* ce[SRSRAN_MAX_PORTS] = {NULL}; const cf_t* ces[2][SRSRAN_MAX_PORTS] = {{NULL}};\n"
           "  const cf_t* rx[2] = {NULL, NULL}; srsran_hip_pbch_state_t* sts[2] = {st, st}; float noise[2] = {0.f, 0.f};\n"
           "  srsran_hip_pbch_res_t res[2]; srsran_hip_chest_dl_res_t out; uint32_t idx[SRSRAN_HIP_PBCH_MAX_RE], n, a, b, c, d; cf_t dd[3 * SRSRAN_HIP_PBCH_MAX_RE];\n"
           "  int rc = srsran_hip_pbch_nof_re(cell) + srsran_hip_pbch_table(cell, idx);\n"
           "  rc += srsran_hip_pbch_try_frames(cell, f, 1, rows) + srsran_hip_pbch_try_frames_dbg(cell, f, 4, rows, f, us);\n"
           "  rc += srsran_hip_pbch_decode(cell, st, sf_symbols[0], ce, 0.1f, res);\n"
           "  rc += srsran_hip_pbch_decode_dbg(cell, st, sf_symbols[0], ce, 0.1f, res, dd, f, rows, &n);\n"
           "  rc += srsran_hip_pbch_decode_est(cell, est, es, st, sf_symbols, res, &out);\n"
           "  rc += srsran_hip_pbch_decode_est_dbg(cell, est, es, st, sf_symbols, res, &out, dd, f, rows, &n);\n"
           "  rc += srsran_hip_pbch_decode_multi(2, cell, sts, rx, ces, noise, res);\n"
           "  srsran_hip_pbch_mib_unpack(res[0].payload, &a, &b, &c, &d);\n"
           "  return rc + (int)(a + b + c + d); }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    assert _compile_run("pbch_abi", src, os.path.join(ROOT, "include"), link=True) == ""


def test_table_equals_the_record_and_the_model(L, golden):
    from srslte_amd import capi

    for i, row in enumerate(golden["m_cells"]):
        c = PB.from_row(row)
        cs = cell_struct(capi, c)
        idx = np.full(240 + 4, 0xEEEEEEEE, np.uint32)
        n = PB.nof_re(c)
        assert L.srsran_hip_pbch_nof_re(C.byref(cs)) == n and L.srsran_hip_pbch_table(C.byref(cs), idx.ctypes.data) == n, c
        assert np.array_equal(idx[:n], golden["m_table_%d" % i]) and np.array_equal(idx[:n], PB.table(c)) and np.all(idx[n:] == 0xEEEEEEEE), c
    for prb, cid in ((50, 3), (100, 503), (110, 251), (6, 0)):  # the model alone: every id class at sizes the record does not hold
        for cp in (7, 6):
            c = PB.cell(prb, 2, cid, cp)
            idx = np.zeros(240, np.uint32)
            assert L.srsran_hip_pbch_table(C.byref(cell_struct(capi, c)), idx.ctypes.data) == PB.nof_re(c)
            assert np.array_equal(idx[:PB.nof_re(c)], PB.table(c)), c


def test_map_refusals_are_silent(L, capfd):
    from srslte_amd import capi

    idx = np.full(240, 0xEEEEEEEE, np.uint32)
    for field, value in (("nof_prb", 5), ("nof_prb", 111), ("id", 504), ("cp_nsymb", 8), ("nof_ports", 3), ("nof_ports", 5)):
        cs = cell_struct(capi, dict(PB.cell(6, 1, 1), **{field: value}))
        assert L.srsran_hip_pbch_nof_re(C.byref(cs)) == -1 and L.srsran_hip_pbch_table(C.byref(cs), idx.ctypes.data) == -1, (field, value)
    cs = cell_struct(capi, PB.cell(6, 1, 1))
    assert L.srsran_hip_pbch_nof_re(None) == -1 and L.srsran_hip_pbch_table(None, idx.ctypes.data) == -1 and L.srsran_hip_pbch_table(C.byref(cs), None) == -1
    assert np.all(idx == 0xEEEEEEEE) and capfd.readouterr().err == ""


def test_mib_unpack_reads_the_recorded_payloads(L, golden):
    assert len(golden["u_payload"]) > 15 and {6, 15, 25, 50, 75, 100} <= set(int(v) for v in golden["u_out"][:, 0])
    for p, want in zip(golden["u_payload"], golden["u_out"]):
        v = [C.c_uint32(77) for _ in range(4)]
        buf = np.ascontiguousarray(p, np.uint8)
        L.srsran_hip_pbch_mib_unpack(buf.ctypes.data, *[C.byref(x) for x in v])
        assert tuple(x.value for x in v) == tuple(int(w) for w in want) == PB.mib_unpack(p), p
    cap = golden["c_payload_%d_0" % list(golden["c_names"]).index("capture_told2")]
    assert "".join(str(b) for b in cap) == "011010000001110000000000" and PB.mib_unpack(cap)[:3] == (50, 0, 2)  # pbch_file_test.c:45-46: a 50-PRB cell's MIB
    L.srsran_hip_pbch_mib_unpack(buf.ctypes.data, None, None, None, None)  # outputs the caller does not want


# ---- refusals
class _Call:
    """valid calls on a 6-PRB cell with sentinels everywhere a call could write"""

    def __init__(self, capi, ports=0, frame_idx=2):
        self.capi = capi
        self.cell = PB.cell(6, ports, 150)
        self.grid = np.ones(14 * 72, np.complex64)
        self.ce = [self.grid.ctypes.data] * 4
        self.rx = self.grid.ctypes.data
        self.noise = 0.1
        self.state = capi.HipPbchState()
        self.state.frame_idx = frame_idx
        for i in range(4 * 480):
            self.state.llr[i] = 0.25
        self.before = bytes(self.state)
        self.res = (capi.HipPbchRes * 8)()
        C.memset(self.res, 0x77, C.sizeof(self.res))
        self.rows = (capi.HipPbchRow * 90)()
        C.memset(self.rows, 0x77, C.sizeof(self.rows))
        self.n_rows = C.c_uint32(0x77777777)
        self.d, self.llr_new = np.full(3 * 240, 5.0, np.complex64), np.full(3 * 480, 5.0, np.float32)
        self.llr, self.rm, self.sym = np.full(4 * 480, 0.5, np.float32), np.full(30 * 120, 5.0, np.float32), np.full(30 * 120, 7, np.uint16)
        self.pilots = np.ones(8 * 6, np.complex64)
        self.est = dict(nof_prb=6, nof_ports=ports or 4, id=150, cp_nsymb=7, nof_rx=1, sf_idx=0)
        self.have_pilots = True
        self.out = capi.HipChestDlRes()
        C.memset(C.byref(self.out), 0x77, C.sizeof(self.out))
        self.use = dict(cell=True, state=True, rx=True, ce=True, res=True, est=True, est_state=True, y=True, out=True, llr=True, rows=True, noise=True, states=True)

    def _common(self):
        cs = cell_struct(self.capi, self.cell)
        ce = (C.c_void_p * 4)(*self.ce)
        self.keep = (cs, ce)
        return cs, ce

    def decode(self, L, dbg):
        u = self.use
        cs, ce = self._common()
        a = [C.byref(cs) if u["cell"] else None, C.byref(self.state) if u["state"] else None, self.rx if u["rx"] else None, ce if u["ce"] else None,
             C.c_float(self.noise), self.res if u["res"] else None]
        if dbg:
            return L.srsran_hip_pbch_decode_dbg(*(a + [self.d.ctypes.data, self.llr_new.ctypes.data, self.rows, C.byref(self.n_rows)]))
        return L.srsran_hip_pbch_decode(*a)

    def decode_est(self, L, dbg):
        u, capi = self.use, self.capi
        cs, _ = self._common()
        est, es = capi.HipChestDl(), capi.HipChestDlState()
        for k, v in self.est.items():
            setattr(est, k, v)
        est.pilots[0] = self.pilots.ctypes.data if self.have_pilots else None
        est.pilots[1] = self.pilots.ctypes.data if self.have_pilots else None
        y = (C.c_void_p * 4)(self.rx if u["rx"] else None, None, None, None)
        a = [C.byref(cs) if u["cell"] else None, C.byref(est) if u["est"] else None, C.byref(es) if u["est_state"] else None,
             C.byref(self.state) if u["state"] else None, y if u["y"] else None, self.res if u["res"] else None, C.byref(self.out) if u["out"] else None]
        if dbg:
            return L.srsran_hip_pbch_decode_est_dbg(*(a + [self.d.ctypes.data, self.llr_new.ctypes.data, self.rows, C.byref(self.n_rows)]))
        return L.srsran_hip_pbch_decode_est(*a)

    def multi(self, L, n):
        u, capi = self.use, self.capi
        cells = (capi.HipPbchCell * 9)(*[cell_struct(capi, self.cell) for _ in range(9)])
        self.states = [capi.HipPbchState.from_buffer_copy(self.before) for _ in range(9)]
        sp = (C.POINTER(capi.HipPbchState) * 9)(*[C.pointer(s) for s in self.states])
        if not u["state"]:
            sp[1] = None
        rx = (C.c_void_p * 9)(*([self.rx] * 9))
        if not u["rx"]:
            rx[1] = None
        ce = ((C.c_void_p * 4) * 9)(*[(C.c_void_p * 4)(*self.ce) for _ in range(9)])
        noise = (C.c_float * 9)(*([self.noise] * 9))
        self.keep = (cells, sp, rx, ce, noise)
        return L.srsran_hip_pbch_decode_multi(n, cells if u["cell"] else None, sp if u["states"] else None, rx if u["y"] else None, ce if u["ce"] else None,
                                              noise if u["noise"] else None, self.res if u["res"] else None)

    def try_frames(self, L, f, dbg):
        u = self.use
        cs, _ = self._common()
        a = [C.byref(cs) if u["cell"] else None, self.llr.ctypes.data if u["llr"] else None, f, self.rows if u["rows"] else None]
        if dbg:
            return L.srsran_hip_pbch_try_frames_dbg(*(a + [self.rm.ctypes.data, self.sym.ctypes.data]))
        return L.srsran_hip_pbch_try_frames(*a)

    def untouched(self, n_res=1):
        """results zeroed (where the call could know how many), the state and the _dbg outputs as they were"""
        ok = bytes(self.state) == self.before and np.all(self.d == 5.0) and np.all(self.llr_new == 5.0) and np.all(self.rm == 5.0) and np.all(self.sym == 7)
        if self.use["res"] and n_res:
            ok = ok and bytes(self.res)[:48 * n_res] == bytes(48 * n_res) and bytes(self.res)[48 * n_res:] == b"\x77" * (48 * (8 - n_res))
        return ok


def _spoil(k, what):
    if what == "a ce plane":
        k.ce[(k.cell["nof_ports"] or 4) - 1] = None
    elif what == "noise nan":
        k.noise = float("nan")
    elif what == "noise inf":
        k.noise = float("inf")
    elif what == "frame_idx":
        k.state.frame_idx = 4
        k.before = bytes(k.state)
    elif what == "pilots":
        k.have_pilots = False
    elif what in k.use:
        k.use[what] = False
    elif what[0] == "est":
        k.est[what[1]] = what[2]
    else:
        k.cell[what[0]] = what[1]
        if what[0] in k.est and what[0] != "nof_ports":
            k.est[what[0]] = what[1]


CELL_RANGE = [("nof_prb", 5), ("nof_prb", 111), ("id", 504), ("cp_nsymb", 5), ("nof_ports", 3), ("nof_ports", 5)]


def test_decode_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for dbg in (False, True):
        who = "srsran_hip_pbch_decode_dbg" if dbg else "srsran_hip_pbch_decode"
        for ports in (0, 2):
            for what in ["cell", "state", "rx", "ce", "res", "a ce plane", "noise nan", "noise inf", "frame_idx"] + CELL_RANGE:
                k = _Call(capi, ports)
                _spoil(k, what)
                capfd.readouterr()
                assert k.decode(L, dbg) == INV and k.untouched(), (dbg, ports, what)
                assert not dbg or k.n_rows.value == 0
                _one_line(capfd, who, (dbg, ports, what))
        k = _Call(capi, 2)  # the planes of ports that are not tried are not looked at
        k.ce[2] = k.ce[3] = None
        if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
            capfd.readouterr()
            assert k.decode(L, dbg) == capi.SRSRAN_ERROR and k.untouched()
            assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_decode_est_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    refusals = ["cell", "state", "rx", "y", "res", "est", "est_state", "out", "frame_idx", "pilots", ("est", "nof_prb", 15), ("est", "id", 151), ("est", "cp_nsymb", 6),
                ("est", "sf_idx", 5), ("est", "nof_ports", 1), ("est", "estimator_alg", 2), ("est", "nof_rx", 0), ("est", "sf_type", 1)] + CELL_RANGE
    for dbg in (False, True):
        who = "srsran_hip_pbch_decode_est_dbg" if dbg else "srsran_hip_pbch_decode_est"
        for ports in (0, 2):
            for what in refusals:
                k = _Call(capi, ports)
                _spoil(k, what)
                capfd.readouterr()
                assert k.decode_est(L, dbg) == INV and k.untouched(), (dbg, ports, what)
                assert not k.use["out"] or bytes(k.out) == bytes(C.sizeof(k.out)), (dbg, ports, what)
                _one_line(capfd, who, (dbg, ports, what))
        k = _Call(capi, 0)
        k.est["nof_ports"] = 2  # a search needs the estimates of four ports
        capfd.readouterr()
        assert k.decode_est(L, dbg) == INV and k.untouched()
        _one_line(capfd, who, "search with two estimated ports")
        if L.srsran_hip_device_count() == 0:
            k = _Call(capi, 0)
            capfd.readouterr()
            assert k.decode_est(L, dbg) == capi.SRSRAN_ERROR and k.untouched() and bytes(k.out) == bytes(C.sizeof(k.out))
            assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_decode_multi_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_pbch_decode_multi"
    for what in ["cell", "states", "state", "rx", "y", "ce", "noise", "res", "a ce plane", "noise nan", "frame_idx"] + CELL_RANGE:
        k = _Call(capi)
        _spoil(k, what)
        capfd.readouterr()
        assert k.multi(L, 3) == INV and k.untouched(3), what
        assert all(bytes(s) == k.before for s in k.states), what
        _one_line(capfd, who, what)
    k = _Call(capi)
    capfd.readouterr()
    assert k.multi(L, 9) == INV and bytes(k.res) == b"\x77" * (48 * 8)
    _one_line(capfd, who, "n")
    k = _Call(capi)
    assert k.multi(L, 0) == 0 and capfd.readouterr().err == "" and bytes(k.res) == b"\x77" * (48 * 8)
    if L.srsran_hip_device_count() == 0:
        k = _Call(capi)
        capfd.readouterr()
        assert k.multi(L, 8) == capi.SRSRAN_ERROR and k.untouched(8) and all(bytes(s) == k.before for s in k.states)
        assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_try_frames_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for dbg in (False, True):
        who = "srsran_hip_pbch_try_frames_dbg" if dbg else "srsran_hip_pbch_try_frames"
        for what in ["cell", "llr", "rows", "f0", "f5"] + CELL_RANGE:
            k = _Call(capi, 1)
            f = 0 if what == "f0" else 5 if what == "f5" else 2
            if what not in ("f0", "f5"):
                _spoil(k, what)
            capfd.readouterr()
            assert k.try_frames(L, f, dbg) == INV and k.untouched(0) and bytes(k.rows) == b"\x77" * (48 * 90), (dbg, what)
            _one_line(capfd, who, (dbg, what))
        if L.srsran_hip_device_count() == 0:
            k = _Call(capi, 1)
            capfd.readouterr()
            assert k.try_frames(L, 4, dbg) == capi.SRSRAN_ERROR and k.untouched(0) and bytes(k.rows)[:48 * 30] == bytes(48 * 30)
            assert "no cpu fallback" in capfd.readouterr().err.lower()
