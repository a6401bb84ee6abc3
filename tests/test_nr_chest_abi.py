"""CPU-only checks of the NR grid calls (include/srsran_amd/phy_nr_chan_abi.h: srsran_hip_nr_sch_nof_re, srsran_hip_nr_sch_get, srsran_hip_dmrs_sch_estimate,
srsran_hip_nr_cw_decode_grid{,_dbg,_multi}), in the manner of test_chest_ul_abi.py: the library exports the entry points and the ctypes mirror binds them, the
mirror's structs have the header's layout, srsran_hip_nr_sch_nof_re gives the reference's count on every configuration of tests/golden/nr_chest_ref.npz,
and every refusal comes before the device is looked for, with one line on stderr, the results zeroed and nothing else written.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nr_chest_model as M
import oracle_api as O
from test_nr_chest_golden import case_cfg, nof_cases, record

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_nr_sch_nof_re", "srsran_hip_nr_sch_get", "srsran_hip_dmrs_sch_estimate", "srsran_hip_nr_cw_decode_grid", "srsran_hip_nr_cw_decode_grid_dbg",
           "srsran_hip_nr_cw_decode_grid_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def grid_of(capi, cfg):
    """the ctypes description of a model configuration"""
    g = capi.HipNrGrid(cfg["nof_prb"], cfg["scs"], cfg["slot_idx"], cfg.get("mapping", 0), cfg["S"], cfg["L"], cfg["dmrs_type"], cfg["typeA_pos"],
                       cfg["additional_pos"], cfg["length"], cfg["n_id"], cfg["n_scid"], cfg["cdm"], cfg["beta"], len(cfg["rvd"]))
    for i, (b, e, st, sc, sym) in enumerate(cfg["rvd"][:4]):
        g.rvd[i] = capi.HipNrRePattern(b, e, st, sc, sym)
    for rb in range(min(cfg["nof_prb"], len(cfg["prb"]), 275)):
        g.prb_idx[rb] = int(cfg["prb"][rb])
    return g


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_mirror_has_the_header_layout():
    from srslte_amd import capi

    G, P, R = capi.HipNrGrid, capi.HipNrRePattern, capi.HipNrChestRes
    fields = ["nof_prb", "scs", "slot_idx", "mapping", "S", "L", "dmrs_type", "typeA_pos", "additional_pos", "length", "n_id", "n_scid",
              "nof_dmrs_cdm_groups_without_data", "beta_dmrs", "nof_rvd", "rvd", "prb_idx"]
    rfields = ["noise_estimate", "noise_estimate_dbm", "rsrp", "rsrp_dbm", "snr_db", "cfo", "sync_error", "nof_re"]
    pfields = ["rb_begin", "rb_end", "rb_stride", "sc", "symbol"]
    items = (["sizeof(srsran_hip_nr_grid_t)"] + ["offsetof(srsran_hip_nr_grid_t, %s)" % f for f in fields] + ["sizeof(srsran_hip_nr_chest_res_t)"] +
             ["offsetof(srsran_hip_nr_chest_res_t, %s)" % f for f in rfields] + ["sizeof(srsran_hip_nr_re_pattern_t)"] +
             ["offsetof(srsran_hip_nr_re_pattern_t, %s)" % f for f in pfields])
    src = ('#include "srsran_amd/phy_nr_chan_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "nr_chest_layout.c"), os.path.join(d, "nr_chest_layout")
    open(cfile, "w").write(src)
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    want = ([C.sizeof(G)] + [getattr(G, f).offset for f in fields] + [C.sizeof(R)] + [getattr(R, f).offset for f in rfields] + [C.sizeof(P)] +
            [getattr(P, f).offset for f in pfields])
    assert got == want
    assert (C.sizeof(G), G.prb_idx.offset, C.sizeof(R), C.sizeof(P)) == (400, 124, 32, 16)


def test_header_declares_them_for_plain_c():
    """a C caller of every new entry point compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_nr_chan_abi.h"\n#include <stddef.h>\n'
           "int take(srsran_hip_nr_cw_rx_t* g, srsran_hip_nr_grid_t* grid, cf_t* sf, cf_t* x, srsran_softbuffer_rx_t* sb, uint8_t* data, srsran_hip_nr_tb_result_t* res,\n"
           "         srsran_hip_nr_chest_res_t* eo, int8_t* e) {\n"
           "  srsran_softbuffer_rx_t* sbs[1] = {sb}; uint8_t* datas[1] = {data};\n"
           "  return (int)srsran_hip_nr_sch_nof_re(grid) + srsran_hip_nr_sch_get(grid, sf, x) + srsran_hip_dmrs_sch_estimate(grid, sf, x, eo) +\n"
           "         srsran_hip_dmrs_sch_estimate(grid, sf, NULL, eo) + srsran_hip_nr_cw_decode_grid(g, grid, sf, sb, data, res, eo) +\n"
           "         srsran_hip_nr_cw_decode_grid_dbg(g, grid, sf, sb, data, res, NULL, e) + srsran_hip_nr_cw_decode_grid_multi(1, g, grid, sf, sbs, datas, res, eo); }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "nr_chest_abi.c"), os.path.join(d, "nr_chest_abi")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.call([exe]) == 0


def test_nof_re_is_the_reference_count(L):
    from srslte_amd import capi

    d = record()
    for i in range(nof_cases()):
        cfg = case_cfg(d, i)
        g = grid_of(capi, cfg)
        assert L.srsran_hip_nr_sch_nof_re(C.byref(g)) == int(d["out_%d" % i][7]) == M.nof_re(cfg), d["names"][i]
    assert L.srsran_hip_nr_sch_nof_re(None) == 0


def test_dmrs_symbol_rules_follow_the_model(L):
    """every (S + L, typeA_pos, additional_pos, length): the host count is the model's where the model has DMRS symbols, and 0 where the reference refuses"""
    from srslte_amd import capi

    base = case_cfg(record(), 0)
    for ld in range(1, 15):
        for pos in (2, 3):
            for ap in range(4):
                for length in (1, 2):
                    cfg = dict(base, S=0, L=ld, typeA_pos=pos, additional_pos=ap, length=length)
                    want = M.nof_re(cfg) if M.dmrs_symbols(cfg) else 0
                    assert L.srsran_hip_nr_sch_nof_re(C.byref(grid_of(capi, cfg))) == want, (ld, pos, ap, length)


# ---- refusals

BAD = [dict(mapping=1), dict(typeA_pos=3, additional_pos=3), dict(typeA_pos=3, additional_pos=1, S=0, L=3), dict(typeA_pos=3, additional_pos=0, S=1, L=3), dict(cdm=0), dict(cdm=4), dict(S=5, L=10),
       dict(S=14, L=1), dict(L=0), dict(prb=np.zeros(25, np.uint8)), dict(nof_prb=276), dict(nof_prb=0), dict(rvd=[(0, 276, 1, 1, 1)]), dict(rvd=[(0, 25, 0, 1, 1)]),
       dict(nof_rvd=5), dict(length=2, additional_pos=3), dict(scs=5), dict(typeA_pos=1), dict(length=3), dict(dmrs_type=2), dict(S=0, L=2)]


class _Call:
    """a valid 25-PRB QPSK codeword on a grid, with sentinels everywhere a call could write"""

    def __init__(self, capi, **kw):
        cfg = dict(case_cfg(record(), 3), rvd=[])
        nof_rvd = kw.pop("nof_rvd", None)
        nof_re = kw.pop("nof_re", None)
        cfg.update(kw)
        self.grid = grid_of(capi, cfg)
        if nof_rvd is not None:
            self.grid.nof_rvd = nof_rvd
        good = M.nof_re(dict(case_cfg(record(), 3), rvd=[]))
        n = good if nof_re is None else nof_re
        self.g = capi.HipNrCwRx(capi.HipNrTb(0.4, 1800, 1, 0x100, 1, 2 * n, 0, 0, 0, 0, 0), n, 1234, 0.8, 6, 0.0, 0)
        self.rows = np.full(25344 + 16, 0x11, np.int8)
        self.keep = np.full(1056 + 16, 0x22, np.uint8)
        self.flags = np.zeros(1, np.bool_)
        self.sb = capi.SoftbufferRx(1, 25344, (C.c_void_p * 1)(self.rows.ctypes.data), (C.c_void_p * 1)(self.keep.ctypes.data),
                                    self.flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
        self.data = np.full(1800 // 8 + 16, 0xEE, np.uint8)
        self.sf = np.zeros(14 * 12 * 276, np.complex64)
        self.x = np.full(14 * 12 * 25, 5, np.complex64)
        self.e = np.full(2 * good + 16, 0x55, np.int8)
        self.res = (capi.HipNrTbResult * 1)(capi.HipNrTbResult(7, 7, 7.0, 7))
        self.eo = (capi.HipNrChestRes * 1)(capi.HipNrChestRes(7, 7, 7, 7, 7, 7, 7, 7))

    def untouched(self):
        return (np.all(self.data == 0xEE) and np.all(self.rows == 0x11) and np.all(self.keep == 0x22) and not self.flags[0] and np.all(self.x == 5) and
                np.all(self.e == 0x55))

    def res_zeroed(self):
        r = self.res[0]
        return (r.crc_ok, r.all_decoded, r.avg_iter, r.nof_cb) == (0, 0, 0, 0)

    def est_zeroed(self):
        e = self.eo[0]
        return (e.noise_estimate, e.noise_estimate_dbm, e.rsrp, e.rsrp_dbm, e.snr_db, e.cfo, e.sync_error, e.nof_re) == (0,) * 8


def _one_line(capfd, who, tag):
    err = capfd.readouterr().err
    assert len(err.strip().splitlines()) == 1 and who in err, (tag, err)
    assert not any(w in err.lower() for w in ("hip error", "device", "illegal", "fault")), (tag, err)


def test_stage_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    for kw in BAD:
        capfd.readouterr()
        k = _Call(capi, **kw)
        assert L.srsran_hip_nr_sch_nof_re(C.byref(k.grid)) == 0, kw
        assert L.srsran_hip_nr_sch_get(C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data) == INV and k.untouched(), kw
        _one_line(capfd, "nr_sch_get", kw)
        assert L.srsran_hip_dmrs_sch_estimate(C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data, k.eo) == INV and k.untouched() and k.est_zeroed(), kw
        _one_line(capfd, "dmrs_sch_estimate", kw)
    for null in range(3):
        k = _Call(capi)
        args = [C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data]
        args[null] = None
        capfd.readouterr()
        assert L.srsran_hip_nr_sch_get(*args) == INV and k.untouched()
        _one_line(capfd, "nr_sch_get", null)
        if null < 2:
            assert L.srsran_hip_dmrs_sch_estimate(*(args + [k.eo])) == INV and k.untouched() and k.est_zeroed()
            _one_line(capfd, "dmrs_sch_estimate", null)
    k = _Call(capi)
    capfd.readouterr()
    assert L.srsran_hip_dmrs_sch_estimate(C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data, None) == INV and k.untouched()
    _one_line(capfd, "dmrs_sch_estimate", "no res")
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        k = _Call(capi)
        assert L.srsran_hip_nr_sch_get(C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data) == capi.SRSRAN_ERROR and k.untouched()
        assert L.srsran_hip_dmrs_sch_estimate(C.byref(k.grid), k.sf.ctypes.data, k.x.ctypes.data, k.eo) == capi.SRSRAN_ERROR and k.untouched() and k.est_zeroed()
        assert L.srsran_hip_dmrs_sch_estimate(C.byref(k.grid), k.sf.ctypes.data, None, k.eo) == capi.SRSRAN_ERROR
        assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_grid_call_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(kind, k, null=None):
        if kind == "multi":
            args = [1, C.pointer(k.g), C.pointer(k.grid), k.sf.ctypes.data, (C.POINTER(capi.SoftbufferRx) * 1)(C.pointer(k.sb)), (C.c_void_p * 1)(k.data.ctypes.data),
                    k.res, k.eo]
            if null is not None:
                args[1 + null] = None
            return L.srsran_hip_nr_cw_decode_grid_multi(*args)
        args = [C.byref(k.g), C.byref(k.grid), k.sf.ctypes.data, C.pointer(k.sb), k.data.ctypes.data, k.res, k.eo]
        if null is not None:
            args[null] = None
        if kind == "dbg":
            return L.srsran_hip_nr_cw_decode_grid_dbg(*(args + [k.e.ctypes.data]))
        return L.srsran_hip_nr_cw_decode_grid(*args)

    twins = [dict(nof_re=100), dict(nof_re=0)]  # an nof_re mismatch (the transport block's own rules are srsran_hip_nr_cw_decode's: test_nr_cw_abi.py)
    for kind in ("plain", "dbg", "multi"):
        for kw in BAD + twins:
            capfd.readouterr()
            k = _Call(capi, **kw)
            assert call(kind, k) == INV and k.untouched() and k.res_zeroed() and k.est_zeroed(), (kind, kw)
            _one_line(capfd, "nr_cw_decode", (kind, kw))
        for null in range(5):
            capfd.readouterr()
            k = _Call(capi)
            assert call(kind, k, null) == INV and k.untouched() and k.res_zeroed() and k.est_zeroed(), (kind, null)
            _one_line(capfd, "nr_cw_decode", (kind, null))
        k = _Call(capi)
        k.g.tb.mod = 0  # what the call on extracted REs refuses is refused here too
        capfd.readouterr()
        assert call(kind, k) == INV and k.untouched() and k.res_zeroed() and k.est_zeroed()
        _one_line(capfd, "nr_cw_decode", (kind, "mod"))
    assert L.srsran_hip_nr_cw_decode_grid_multi(0, None, None, None, None, None, None, None) == 0  # an empty slot is a no-op
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly
        for kind in ("plain", "dbg", "multi"):
            capfd.readouterr()
            k = _Call(capi)
            assert call(kind, k) == capi.SRSRAN_ERROR and k.untouched() and k.est_zeroed(), kind
            assert "no cpu fallback" in capfd.readouterr().err.lower()
