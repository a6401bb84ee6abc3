"""CPU-only checks of the PDCCH search's entry points (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pdcch_*, srsran_hip_pdcch_extract_llr,
srsran_hip_pdcch_search_sf{,_dbg}), in the manner of test_conv_abi.py: the library exports them and the ctypes mirror binds them, the description is 44 bytes
in the header and in the mirror, a plain C caller holding cf_t* sf_symbols[SRSRAN_MAX_PORTS] and cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] compiles under
-Wall -Werror, every refusal comes before the device is looked for with one line on stderr and nothing written but the zeroed results, and a valid call without a
device fails loudly.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import pdcch_map_model as PM
from test_conv_abi import _compile_run, _one_line
from test_pdcch_sf_golden import sf_struct

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_regs_pdcch_nregs", "srsran_hip_regs_pdcch_table", "srsran_hip_regs_pdcch_get", "srsran_hip_pdcch_extract_llr", "srsran_hip_pdcch_search_sf",
           "srsran_hip_pdcch_search_sf_dbg", "srsran_hip_pdcch_dci_decode_multi", "srsran_hip_pdcch_dci_decode_multi_dbg"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_eight_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_description_is_44_bytes_in_header_and_mirror():
    from srslte_amd import capi

    items = ["sizeof(srsran_hip_pdcch_sf_t)"] + ["offsetof(srsran_hip_pdcch_sf_t, %s)" % f for f in PM.FIELDS] + ["SRSRAN_MAX_PORTS"]
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("pdcch_sf_layout", src, os.path.join(ROOT, "include")).split()]
    assert got == [44] + [4 * i for i in range(11)] + [4]
    assert [C.sizeof(capi.HipPdcchSf)] + [getattr(capi.HipPdcchSf, f).offset for f in PM.FIELDS] == got[:-1]


def test_header_takes_a_plain_c_callers_arrays():
    """a C caller that holds the arrays a caller of srsran_pdcch_extract_llr holds compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n'
           "int take(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, float* f, uint16_t* us, uint32_t* idx) {\n"
           "  cf_t* sf_symbols[SRSRAN_MAX_PORTS] = {NULL}; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{NULL}};\n"
           "  cf_t* d[2] = {NULL, NULL}; const cf_t* grids[2] = {NULL, NULL}; cf_t dd[4];\n"
           "  int rc = srsran_hip_regs_pdcch_nregs(sf) + srsran_hip_regs_pdcch_table(sf, idx) + srsran_hip_regs_pdcch_get(sf, 2, grids, d);\n"
           "  rc += srsran_hip_pdcch_extract_llr(sf, sf_symbols, ce, 0.1f, f) + srsran_hip_pdcch_search_sf(sf, sf_symbols, ce, 0.1f, 1, cand, res);\n"
           "  rc += srsran_hip_pdcch_search_sf_dbg(sf, sf_symbols, ce, 0.1f, 1, cand, res, f, dd, sf_symbols, ce, f, us);\n"
           "  return rc; }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0) : 0; }\n")
    assert _compile_run("pdcch_sf_abi", src, os.path.join(ROOT, "include"), link=True) == ""


# ---- refusals
class _Call:
    """a valid search of three candidates on a 15-PRB, 2-port, 2-antenna region (cfi 2), with sentinels everywhere a call could write"""

    def __init__(self, capi, n=3):
        self.capi = capi
        self.sf = PM.describe(15, 2, 5, 2, sf_idx=4, nof_rx=2)
        self.nof_cce = PM.reg_table(self.sf).size // 36
        npts = 2 * 12 * 15
        self.grid = np.ones(npts, np.complex64)
        self.y = [self.grid.ctypes.data, self.grid.ctypes.data, None, None]
        self.h = [[self.grid.ctypes.data, self.grid.ctypes.data, None, None], [self.grid.ctypes.data, self.grid.ctypes.data, None, None], [None] * 4, [None] * 4]
        self.n = n
        self.cand = (capi.HipPdcchCand * max(n, 1))(*[capi.HipPdcchCand(i, i % 3, 27 + i) for i in range(max(n, 1))])
        self.res = (capi.HipPdcchRes * max(n, 1))()
        for r in self.res:
            C.memset(C.byref(r), 0x77, C.sizeof(r))
        self.llr = np.full(72 * self.nof_cce + 8, 5.0, np.float32)
        self.d = np.full(36 * self.nof_cce + 8, 5.0, np.complex64)
        self.rm = np.full(max(n, 1) * 432 + 8, 5.0, np.float32)
        self.sym = np.full(max(n, 1) * 432 + 8, 5, np.uint16)
        self.use = dict(sf=True, y=True, h=True, cand=True, res=True)

    def args(self):
        sf = sf_struct(self.capi, self.sf)
        y = (C.c_void_p * 4)(*self.y)
        h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in self.h])
        self.keep = (sf, y, h)
        u = self.use
        return [C.byref(sf) if u["sf"] else None, y if u["y"] else None, h if u["h"] else None, C.c_float(0.1)]

    def search(self, L, dbg, n=None):
        a = self.args() + [self.n if n is None else n, self.cand if self.use["cand"] else None, self.res if self.use["res"] else None]
        if dbg:
            return L.srsran_hip_pdcch_search_sf_dbg(*(a + [self.llr.ctypes.data, self.d.ctypes.data, None, None, self.rm.ctypes.data, self.sym.ctypes.data]))
        return L.srsran_hip_pdcch_search_sf(*a)

    def extract(self, L, llr=True):
        return L.srsran_hip_pdcch_extract_llr(*(self.args() + [self.llr.ctypes.data if llr else None]))

    def zeroed(self):
        return bytes(self.res)[:self.n * 152] == bytes(self.n * 152)

    def untouched(self):
        return np.all(self.llr == 5.0) and np.all(self.d == 5.0) and np.all(self.rm == 5.0) and np.all(self.sym == 5)


def _spoil(k, what):
    if what == "L":
        k.cand[1].L = 4
    elif what == "past the end":
        k.cand[2].ncce = k.nof_cce - 3  # an L = 2 candidate needs four CCEs
    elif what == "ncce wraps":
        k.cand[1].ncce = 0xFFFFFFFF // 72 + 1
    elif what == "nof_bits 0":
        k.cand[0].nof_bits = 0
    elif what == "nof_bits 129":
        k.cand[2].nof_bits = 129
    elif what == "a received grid":
        k.y[1] = None
    elif what == "an estimate grid":
        k.h[1][1] = None
    elif what in k.use:
        k.use[what] = False
    else:
        field, value = what
        k.sf[field] = value


OUT_OF_RANGE = [("cell_nof_prb", 5), ("cell_nof_prb", 111), ("cell_nof_ports", 3), ("cell_id", 504), ("cp_nsymb", 8), ("phich_length", 2), ("phich_resources", 4),
                ("phich_mi", 4), ("mbsfn_or_sf1_6_tdd", 2), ("cfi", 0), ("cfi", 4), ("sf_idx", 10), ("nof_rx", 3), ("nof_rx", 0)]
SEARCH_REFUSALS = ["L", "past the end", "ncce wraps", "nof_bits 0", "nof_bits 129", "a received grid", "an estimate grid", "sf", "y", "h", "cand"] + OUT_OF_RANGE


def test_search_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for dbg in (False, True):
        who = "srsran_hip_pdcch_search_sf_dbg" if dbg else "srsran_hip_pdcch_search_sf"
        for what in SEARCH_REFUSALS:
            k = _Call(capi)
            _spoil(k, what)
            capfd.readouterr()
            assert k.search(L, dbg) == INV and k.zeroed() and k.untouched(), (dbg, what)
            _one_line(capfd, who, (dbg, what))
        k = _Call(capi)
        _spoil(k, "res")
        capfd.readouterr()
        assert k.search(L, dbg) == INV and k.untouched()
        _one_line(capfd, who, (dbg, "res"))
        k = _Call(capi)
        assert k.search(L, dbg, n=257) == INV and k.untouched() and bytes(k.res)[:152] == b"\x77" * 152
        _one_line(capfd, who, (dbg, "n"))
        for what in ("sf", "y", "h", "cand", "res", ("cfi", 7)):  # an empty search is a no-op whatever else it is handed
            k = _Call(capi)
            _spoil(k, what)
            assert k.search(L, dbg, n=0) == 0 and capfd.readouterr().err == "" and k.untouched() and bytes(k.res)[:152] == b"\x77" * 152
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for dbg in (False, True):
            k = _Call(capi)
            capfd.readouterr()
            assert k.search(L, dbg) == capi.SRSRAN_ERROR and k.zeroed() and k.untouched()
            assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_extract_and_map_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for what in ["a received grid", "an estimate grid", "sf", "y", "h"] + OUT_OF_RANGE:
        k = _Call(capi)
        _spoil(k, what)
        capfd.readouterr()
        assert k.extract(L) == INV and k.untouched(), what
        _one_line(capfd, "srsran_hip_pdcch_extract_llr", what)
    k = _Call(capi)
    assert k.extract(L, llr=False) == INV
    _one_line(capfd, "srsran_hip_pdcch_extract_llr", "llr")
    # the host-only calls: -1, silently (they return a count)
    idx = np.full(4096, 0xEEEEEEEE, np.uint32)
    for what in OUT_OF_RANGE:
        k = _Call(capi)
        _spoil(k, what)
        sf = sf_struct(capi, k.sf)
        assert L.srsran_hip_regs_pdcch_nregs(C.byref(sf)) == -1 and L.srsran_hip_regs_pdcch_table(C.byref(sf), idx.ctypes.data) == -1, what
    sf = sf_struct(capi, _Call(capi).sf)
    assert L.srsran_hip_regs_pdcch_nregs(None) == -1 and L.srsran_hip_regs_pdcch_table(None, idx.ctypes.data) == -1 and L.srsran_hip_regs_pdcch_table(C.byref(sf), None) == -1
    assert np.all(idx == 0xEEEEEEEE) and capfd.readouterr().err == ""
    # a PHICH that leaves the region of cfi 1 without REGs: the reference's own initialisation divides by zero on it
    sf = sf_struct(capi, PM.describe(50, 4, 1, 3, phich_resources=3, phich_mi=3))
    assert L.srsran_hip_regs_pdcch_nregs(C.byref(sf)) == -1
    # the gather
    k = _Call(capi)
    out = np.full(36 * k.nof_cce + 8, 5.0, np.complex64)
    grids, d = (C.c_void_p * 2)(k.grid.ctypes.data, k.grid.ctypes.data), (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
    sf = sf_struct(capi, k.sf)
    bad_sf = sf_struct(capi, dict(k.sf, cfi=4))
    capfd.readouterr()
    for a in [(None, 2, grids, d), (C.byref(bad_sf), 2, grids, d), (C.byref(sf), 0, grids, d), (C.byref(sf), 11, grids, d), (C.byref(sf), 2, None, d),
              (C.byref(sf), 2, grids, None), (C.byref(sf), 2, (C.c_void_p * 2)(k.grid.ctypes.data, None), d), (C.byref(sf), 2, grids, (C.c_void_p * 2)(None, out.ctypes.data))]:
        assert L.srsran_hip_regs_pdcch_get(*a) == -1 and np.all(out == 5.0)
        _one_line(capfd, "srsran_hip_regs_pdcch_get", a[1])
    if L.srsran_hip_device_count() == 0:
        k = _Call(capi)
        capfd.readouterr()
        assert k.extract(L) == capi.SRSRAN_ERROR and k.untouched()
        assert "no cpu fallback" in capfd.readouterr().err.lower()
        assert L.srsran_hip_regs_pdcch_get(C.byref(sf), 2, grids, d) == -1 and np.all(out == 5.0)
        assert "no cpu fallback" in capfd.readouterr().err.lower()
