"""CPU-only checks of the PCFICH / PHICH entry points (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pcfich_table, srsran_hip_regs_phich_ngroups / _table,
srsran_hip_pcfich_decode{,_dbg}, srsran_hip_phich_decode_multi), in the manner of test_pdcch_sf_abi.py: the library exports them and the ctypes mirror binds them,
the structs have the declared sizes in the header and in the mirror, a plain C caller compiles under -Wall -Werror, every refusal comes before the device is
looked for with one line on stderr and nothing written but the zeroed results, and a valid call without a device fails loudly.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import pdcch_map_model as PM
from test_conv_abi import _compile_run, _one_line
from test_pdcch_sf_abi import OUT_OF_RANGE
from test_pdcch_sf_golden import sf_struct

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_regs_pcfich_table", "srsran_hip_regs_phich_ngroups", "srsran_hip_regs_phich_table", "srsran_hip_pcfich_decode", "srsran_hip_pcfich_decode_dbg",
           "srsran_hip_phich_decode_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_struct_sizes_in_header_and_mirror():
    from srslte_amd import capi

    items = ["sizeof(srsran_hip_pdcch_sf_t)", "sizeof(srsran_hip_phich_resource_t)", "sizeof(srsran_hip_phich_res_t)", "offsetof(srsran_hip_phich_res_t, distance)",
             "offsetof(srsran_hip_phich_res_t, bits)", "offsetof(srsran_hip_phich_res_t, z)", "SRSRAN_HIP_PHICH_MAX_RESOURCES"]
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("ctrl_layout", src, os.path.join(ROOT, "include")).split()]
    assert got == [44, 8, 44, 4, 8, 20, 16]
    R = capi.HipPhichRes
    assert [C.sizeof(capi.HipPdcchSf), C.sizeof(capi.HipPhichResource), C.sizeof(R), R.distance.offset, R.bits.offset, R.z.offset] == got[:-1]


def test_header_takes_a_plain_c_callers_arrays():
    """a C caller that holds the arrays a caller of srsran_pcfich_decode / srsran_phich_decode holds compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n'
           "int take(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_phich_resource_t* r, srsran_hip_phich_res_t* res, uint32_t* idx) {\n"
           "  cf_t* sf_symbols[SRSRAN_MAX_PORTS] = {NULL}; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{NULL}};\n"
           "  uint32_t cfi; float corr, data_f[32], corr3[3]; cf_t d[16];\n"
           "  int rc = srsran_hip_regs_pcfich_table(sf, idx) + srsran_hip_regs_phich_ngroups(sf) + srsran_hip_regs_phich_table(sf, 0, idx);\n"
           "  rc += srsran_hip_pcfich_decode(sf, sf_symbols, ce, 0.1f, &cfi, &corr);\n"
           "  rc += srsran_hip_pcfich_decode_dbg(sf, sf_symbols, ce, 0.1f, &cfi, &corr, data_f, d, corr3);\n"
           "  rc += srsran_hip_phich_decode_multi(sf, sf_symbols, ce, 0.1f, 1, r, res);\n"
           "  return rc + (int)res[0].ack_value; }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0) : 0; }\n")
    assert _compile_run("ctrl_abi", src, os.path.join(ROOT, "include"), link=True) == ""


# ---- refusals
class _Call:
    """valid calls on a 15-PRB, 2-port, 2-antenna subframe with two PHICH groups, with sentinels everywhere a call could write"""

    def __init__(self, capi, n=3):
        self.capi = capi
        self.sf = PM.describe(15, 2, 5, 2, sf_idx=4, nof_rx=2)
        self.grid = np.ones(3 * 12 * 15, np.complex64)
        self.y = [self.grid.ctypes.data, self.grid.ctypes.data, None, None]
        self.h = [[self.grid.ctypes.data, self.grid.ctypes.data, None, None], [self.grid.ctypes.data, self.grid.ctypes.data, None, None], [None] * 4, [None] * 4]
        self.n = n
        self.r = (capi.HipPhichResource * max(n, 1))(*[capi.HipPhichResource(i % 2, i) for i in range(max(n, 1))])
        self.res = (capi.HipPhichRes * max(n, 1))()
        C.memset(self.res, 0x77, C.sizeof(self.res))
        self.cfi, self.corr = C.c_uint32(0x77777777), C.c_float(5.0)
        self.data_f, self.d, self.corr3 = np.full(32 + 4, 5.0, np.float32), np.full(16 + 4, 5.0, np.complex64), np.full(3 + 4, 5.0, np.float32)
        self.use = dict(sf=True, y=True, h=True, r=True, res=True, cfi=True)

    def args(self):
        sf = sf_struct(self.capi, self.sf)
        y = (C.c_void_p * 4)(*self.y)
        h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in self.h])
        self.keep = (sf, y, h)
        u = self.use
        return [C.byref(sf) if u["sf"] else None, y if u["y"] else None, h if u["h"] else None, C.c_float(0.1)]

    def pcfich(self, L, dbg):
        a = self.args() + [C.byref(self.cfi) if self.use["cfi"] else None, C.byref(self.corr)]
        if dbg:
            return L.srsran_hip_pcfich_decode_dbg(*(a + [self.data_f.ctypes.data, self.d.ctypes.data, self.corr3.ctypes.data]))
        return L.srsran_hip_pcfich_decode(*a)

    def phich(self, L, n=None):
        return L.srsran_hip_phich_decode_multi(*(self.args() + [self.n if n is None else n, self.r if self.use["r"] else None, self.res if self.use["res"] else None]))

    def pcfich_zeroed(self):
        return (self.cfi.value == 0 or not self.use["cfi"]) and self.corr.value == 0 and np.all(self.data_f == 5.0) and np.all(self.d == 5.0) and np.all(self.corr3 == 5.0)

    def phich_zeroed(self):
        return bytes(self.res)[:self.n * 44] == bytes(self.n * 44)


def _spoil(k, what):
    if what == "ngroup":
        k.r[1].ngroup = 2  # the subframe has two groups
    elif what == "nseq":
        k.r[2].nseq = 8
    elif what == "nseq ext":
        k.sf["cp_nsymb"] = 6
        k.r[1].nseq = 4
    elif what == "no phich":
        k.sf["phich_mi"] = 0
    elif what == "a received grid":
        k.y[1] = None
    elif what == "an estimate grid":
        k.h[1][1] = None
    elif what == "no regs":  # a PHICH that leaves the region of cfi 1 without REGs: the map refuses it
        k.sf.update(cell_nof_prb=50, cell_nof_ports=4, phich_resources=3, phich_mi=3)
    elif what in k.use:
        k.use[what] = False
    else:
        field, value = what
        k.sf[field] = value


COMMON = ["a received grid", "an estimate grid", "sf", "y", "h", "no regs"] + OUT_OF_RANGE


def test_pcfich_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for dbg in (False, True):
        who = "srsran_hip_pcfich_decode_dbg" if dbg else "srsran_hip_pcfich_decode"
        for what in COMMON + ["cfi"]:
            k = _Call(capi)
            _spoil(k, what)
            capfd.readouterr()
            assert k.pcfich(L, dbg) == INV and k.pcfich_zeroed(), (dbg, what)
            _one_line(capfd, who, (dbg, what))
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for dbg in (False, True):
            k = _Call(capi)
            capfd.readouterr()
            assert k.pcfich(L, dbg) == capi.SRSRAN_ERROR and k.pcfich_zeroed()
            assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_phich_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_phich_decode_multi"
    for what in COMMON + ["ngroup", "nseq", "nseq ext", "no phich", "r"]:
        k = _Call(capi)
        _spoil(k, what)
        capfd.readouterr()
        assert k.phich(L) == INV and k.phich_zeroed(), what
        _one_line(capfd, who, what)
    k = _Call(capi)
    _spoil(k, "res")
    capfd.readouterr()
    assert k.phich(L) == INV
    _one_line(capfd, who, "res")
    k = _Call(capi)
    assert k.phich(L, n=17) == INV and bytes(k.res)[:44] == b"\x77" * 44
    _one_line(capfd, who, "n")
    for what in ("sf", "y", "h", "r", "res", ("cfi", 7)):  # an empty call is a no-op whatever else it is handed
        k = _Call(capi)
        _spoil(k, what)
        assert k.phich(L, n=0) == 0 and capfd.readouterr().err == "" and bytes(k.res)[:44] == b"\x77" * 44
    if L.srsran_hip_device_count() == 0:
        k = _Call(capi)
        capfd.readouterr()
        assert k.phich(L) == capi.SRSRAN_ERROR and k.phich_zeroed()
        assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_map_refusals_are_silent(L, capfd):
    from srslte_amd import capi

    idx = np.full(64, 0xEEEEEEEE, np.uint32)
    for what in OUT_OF_RANGE + ["no regs"]:
        k = _Call(capi)
        _spoil(k, what)
        sf = sf_struct(capi, k.sf)
        assert L.srsran_hip_regs_pcfich_table(C.byref(sf), idx.ctypes.data) == -1 and L.srsran_hip_regs_phich_ngroups(C.byref(sf)) == -1, what
        assert L.srsran_hip_regs_phich_table(C.byref(sf), 0, idx.ctypes.data) == -1, what
    sf = sf_struct(capi, _Call(capi).sf)
    assert L.srsran_hip_regs_pcfich_table(None, idx.ctypes.data) == -1 and L.srsran_hip_regs_pcfich_table(C.byref(sf), None) == -1
    assert L.srsran_hip_regs_phich_ngroups(None) == -1 and L.srsran_hip_regs_phich_table(None, 0, idx.ctypes.data) == -1
    assert L.srsran_hip_regs_phich_table(C.byref(sf), 0, None) == -1 and L.srsran_hip_regs_phich_table(C.byref(sf), 2, idx.ctypes.data) == -1
    none = sf_struct(capi, dict(_Call(capi).sf, phich_mi=0))
    assert L.srsran_hip_regs_phich_ngroups(C.byref(none)) == 0 and L.srsran_hip_regs_phich_table(C.byref(none), 0, idx.ctypes.data) == -1
    assert np.all(idx == 0xEEEEEEEE) and capfd.readouterr().err == ""


# ---- the search from the received grids alone
EST_SYMBOLS = ["srsran_hip_pdcch_search_est", "srsran_hip_pdcch_search_est_dbg"]


def test_search_est_is_exported_and_its_options_are_20_bytes(L):
    from srslte_amd import capi

    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in EST_SYMBOLS if s not in exported] and all(getattr(L, s).argtypes is not None for s in EST_SYMBOLS)
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n#include <stdio.h>\n'
           "int take(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* st, const srsran_hip_pdcch_est_t* opt,\n"
           "         const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* r, srsran_hip_phich_res_t* pr, float* f, uint16_t* us) {\n"
           "  cf_t* sf_symbols[SRSRAN_MAX_PORTS] = {NULL}; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{NULL}};\n"
           "  uint32_t cfi; float corr; srsran_hip_chest_dl_res_t out;\n"
           "  return srsran_hip_pdcch_search_est(sf, est, st, sf_symbols, opt, cand, res, r, pr, &cfi, &corr, &out) +\n"
           "         srsran_hip_pdcch_search_est_dbg(sf, est, st, sf_symbols, opt, cand, res, r, pr, &cfi, &corr, &out, f, f, ce, f, us); }\n"
           'int main(int argc, char** argv) { printf("%zu %zu %zu", sizeof(srsran_hip_pdcch_est_t), offsetof(srsran_hip_pdcch_est_t, cfi3_to_2),\n'
           "  offsetof(srsran_hip_pdcch_est_t, n_phich)); return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    assert [int(v) for v in _compile_run("ctrl_est_abi", src, os.path.join(ROOT, "include"), link=True).split()] == [20, 12, 16]
    assert (C.sizeof(capi.HipPdcchEst), capi.HipPdcchEst.cfi3_to_2.offset, capi.HipPdcchEst.n_phich.offset) == (20, 12, 16)


class _Est:
    """a valid search from the grids of a 15-PRB, 2-port, 2-antenna subframe: lists of 2, 3 and 4 candidates, two PHICH resources, sentinels in every output"""

    def __init__(self, capi):
        self.capi = capi
        self.sf = PM.describe(15, 2, 5, 2, sf_idx=4, nof_rx=2)
        self.grid, self.pilots = np.ones(14 * 12 * 15, np.complex64), np.ones(8 * 15, np.complex64)
        self.y = [self.grid.ctypes.data, self.grid.ctypes.data, None, None]
        self.est = dict(nof_prb=15, nof_ports=2, id=5, cp_nsymb=7, nof_rx=2, sf_idx=4, estimator_alg=1, noise_alg=0, filter_type=2)
        self.have_pilots = True
        self.n = [2, 3, 4]
        self.cand = (capi.HipPdcchCand * 9)(*[capi.HipPdcchCand(0, 0, 27 + i) for i in range(9)])
        self.res, self.ph = (capi.HipPdcchRes * 4)(), (capi.HipPhichRes * 2)()
        C.memset(self.res, 0x77, C.sizeof(self.res))
        C.memset(self.ph, 0x77, C.sizeof(self.ph))
        self.r = (capi.HipPhichResource * 2)(capi.HipPhichResource(0, 1), capi.HipPhichResource(1, 7))
        self.rule, self.n_ph = 0, 2
        self.cfi, self.corr, self.out = C.c_uint32(0x77777777), C.c_float(5.0), capi.HipChestDlRes()
        C.memset(C.byref(self.out), 0x77, C.sizeof(self.out))
        self.llr, self.rm = np.full(72 * 12 + 8, 5.0, np.float32), np.full(4 * 432 + 8, 5.0, np.float32)
        self.use = dict(sf=True, est=True, state=True, y=True, opt=True, cand=True, res=True, r=True, ph=True, cfi=True, out=True)

    def call(self, L, dbg):
        capi, u = self.capi, self.use
        sf, est, state = sf_struct(capi, self.sf), capi.HipChestDl(), capi.HipChestDlState()
        for k, v in self.est.items():
            setattr(est, k, v)
        est.pilots[0] = self.pilots.ctypes.data if self.have_pilots else None
        opt = capi.HipPdcchEst((C.c_uint32 * 3)(*self.n), self.rule, self.n_ph)
        y = (C.c_void_p * 4)(*self.y)
        a = [C.byref(sf) if u["sf"] else None, C.byref(est) if u["est"] else None, C.byref(state) if u["state"] else None, y if u["y"] else None,
             C.byref(opt) if u["opt"] else None, self.cand if u["cand"] else None, self.res if u["res"] else None, self.r if u["r"] else None,
             self.ph if u["ph"] else None, C.byref(self.cfi) if u["cfi"] else None, C.byref(self.corr), C.byref(self.out) if u["out"] else None]
        if dbg:
            return L.srsran_hip_pdcch_search_est_dbg(*(a + [self.llr.ctypes.data, None, None, self.rm.ctypes.data, None]))
        return L.srsran_hip_pdcch_search_est(*a)

    def zeroed(self):
        u, ok = self.use, np.all(self.llr == 5.0) and np.all(self.rm == 5.0) and self.corr.value == 0
        counts = u["opt"] and max(self.n) <= 256 and self.n_ph <= 16
        ok = ok and (not (u["res"] and counts) or bytes(self.res)[:max(self.n) * 152] == bytes(max(self.n) * 152))
        ok = ok and (not (u["ph"] and counts) or bytes(self.ph)[:self.n_ph * 44] == bytes(self.n_ph * 44))
        return ok and (not u["cfi"] or self.cfi.value == 0) and (not u["out"] or bytes(self.out) == bytes(C.sizeof(self.out)))


def _spoil_est(k, what):
    if what == "past the region of cfi 1":
        k.cand[1].ncce = 2  # the region of CFI 1 has two CCEs; the same candidate would fit the lists of CFI 2 and 3
    elif what == "past the region of cfi 3":
        k.cand[8].L, k.cand[8].ncce = 3, 5
    elif what == "L":
        k.cand[4].L = 4
    elif what == "nof_bits":
        k.cand[0].nof_bits = 129
    elif what == "257 candidates":
        k.n[1] = 257
    elif what == "17 resources":
        k.n_ph = 17
    elif what == "ngroup":
        k.r[1].ngroup = 2
    elif what == "nseq":
        k.r[0].nseq = 8
    elif what == "rule":
        k.rule = 2
    elif what == "a received grid":
        k.y[1] = None
    elif what == "pilots":
        k.have_pilots = False
    elif what == "no regs":
        k.sf.update(cell_nof_prb=50, cell_nof_ports=4, phich_resources=3, phich_mi=3)
        k.est.update(nof_prb=50, nof_ports=4)
    elif what in k.use:
        k.use[what] = False
    elif what[0] == "est":
        k.est[what[1]] = what[2]
    else:
        k.sf[what[0]] = what[1]
        if what[0] == "nof_rx":
            k.est["nof_rx"] = what[1]


EST_REFUSALS = ["past the region of cfi 1", "past the region of cfi 3", "L", "nof_bits", "257 candidates", "17 resources", "ngroup", "nseq", "rule", "a received grid",
                "pilots", "no regs", "sf", "est", "state", "y", "opt", "cand", "res", "r", "ph", "cfi", "out", ("est", "nof_prb", 25), ("est", "nof_ports", 1),
                ("est", "id", 6), ("est", "cp_nsymb", 6), ("est", "sf_idx", 5), ("est", "nof_rx", 1), ("est", "estimator_alg", 2), ("nof_rx", 3)] + \
    [x for x in OUT_OF_RANGE if x[0] != "nof_rx"]


def test_search_est_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    k = _Est(capi)
    assert PM.reg_table(dict(k.sf, cfi=1)).size // 36 == 2 and PM.reg_table(dict(k.sf, cfi=3)).size // 36 == 12
    for dbg in (False, True):
        who = "srsran_hip_pdcch_search_est_dbg" if dbg else "srsran_hip_pdcch_search_est"
        for what in EST_REFUSALS:
            k = _Est(capi)
            _spoil_est(k, what)
            capfd.readouterr()
            assert k.call(L, dbg) == INV and k.zeroed(), (dbg, what)
            _one_line(capfd, who, (dbg, what))
        if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
            k = _Est(capi)
            capfd.readouterr()
            assert k.call(L, dbg) == capi.SRSRAN_ERROR and k.zeroed()
            assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_search_est_holds_its_three_tables_while_the_cache_starts_over(L, capfd):
    """more descriptions than a third of the 32-entry table cache through the host path of srsran_hip_pdcch_search_est (the refusal path, which reads all three
    tables), interleaved with the srsran_hip_regs_* calls that fill the same cache: every refusal is the one the description's OWN tables call for -- the group
    count of its PHICH, the size of the region of the list's CFI -- whenever the cache starts over between the call's lookups"""
    import ctrl_model as KM
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_pdcch_search_est"
    idx = np.zeros(16, np.uint32)
    for cell_id in range(40):
        for ng in (0, 3):
            base = _Est(capi)
            base.sf.update(cell_id=cell_id, phich_resources=ng)
            nof_cce = [PM.reg_table(dict(base.sf, cfi=c)).size // 36 for c in (1, 2, 3)]
            ngroups = KM.phich_ngroups(base.sf)
            sf = sf_struct(capi, base.sf)
            if cell_id % 2:  # an entry of the same cache ahead of the call's
                assert L.srsran_hip_regs_pdcch_nregs(C.byref(sf)) == 9 * nof_cce[1]
            for c, at in ((0, 1), (1, 3), (2, 8)):  # a candidate that starts where the region of its list's CFI ends; the PHICH resources are the last valid ones
                k = _Est(capi)
                k.sf, k.est["id"] = dict(base.sf), cell_id
                k.r[0].ngroup, k.r[1].ngroup = ngroups - 1, 0
                k.cand[at].ncce = nof_cce[c]
                capfd.readouterr()
                assert k.call(L, False) == INV and k.zeroed(), (cell_id, ng, c)
                err = capfd.readouterr().err
                assert who in err and "control region" in err and len(err.strip().splitlines()) == 1, (cell_id, ng, c, err)
            k = _Est(capi)
            k.sf, k.est["id"] = dict(base.sf), cell_id
            k.r[1].ngroup = ngroups
            capfd.readouterr()
            assert k.call(L, True) == INV and "ngroup" in capfd.readouterr().err, (cell_id, ng)
            assert L.srsran_hip_regs_pcfich_table(C.byref(sf), idx.ctypes.data) == 16 and np.array_equal(idx, KM.pcfich_table(base.sf)), cell_id
            assert L.srsran_hip_regs_phich_ngroups(C.byref(sf)) == ngroups
