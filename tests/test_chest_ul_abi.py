"""CPU-only checks of the PUSCH channel estimator's calls (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_ul_estimate_pusch{,_multi},
srsran_hip_pusch_decode_est{,_multi}), in the manner of test_pdsch_sf_abi.py: the library exports the four entry points and the ctypes mirror binds them, the
mirror's structs have the header's layout, a plain C caller compiles under -Wall -Werror, and every refusal comes before the device is looked for, with one
line on stderr, the results zeroed and nothing else written.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_chest_ul_estimate_pusch", "srsran_hip_chest_ul_estimate_pusch_multi", "srsran_hip_pusch_decode_est", "srsran_hip_pusch_decode_est_multi"]
NOF_PRB, L_PRB = 15, 2
NOF_RE = 12 * 12 * L_PRB


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


def test_mirror_has_the_header_layout():
    """sizes and offsets of the two structs as a C compiler lays the header's out"""
    from srslte_amd import capi

    src = ('#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n#include <stdio.h>\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(srsran_hip_chest_ul_t), offsetof(srsran_hip_chest_ul_t, filter),\n'
           "  offsetof(srsran_hip_chest_ul_t, meas_ta_en), offsetof(srsran_hip_chest_ul_t, r), sizeof(srsran_hip_chest_ul_res_t),\n"
           "  offsetof(srsran_hip_chest_ul_res_t, snr), offsetof(srsran_hip_chest_ul_res_t, cfo_hz), offsetof(srsran_hip_chest_ul_res_t, ta_us)); return 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "chest_ul_layout.c"), os.path.join(d, "chest_ul_layout")
    open(cfile, "w").write(src)
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    E, R = capi.HipChestUl, capi.HipChestUlRes
    assert got == [C.sizeof(E), E.filter.offset, E.meas_ta_en.offset, E.r.offset, C.sizeof(R), R.snr.offset, R.cfo_hz.offset, R.ta_us.offset]
    assert got == [32, 4, 16, 24, 24, 8, 16, 20]


def test_header_declares_them_for_plain_c():
    """a C file that passes what srsran_enb_ul_get_pusch's caller holds -- the subframe grid, an entry of the pregenerated DMRS table -- compiles under
    -Wall -Werror and links (not run)"""
    src = '#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n'
    src += ("struct pregen_like { cf_t** r[8][10]; };\n"
            "int take(struct pregen_like* pregen, srsran_hip_pusch_rx_t* g, srsran_hip_pusch_uci_t* uci, cf_t* sf_symbols, cf_t* ce, srsran_softbuffer_rx_t* sb,\n"
            "         uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_pusch_uci_out_t* uo, srsran_hip_chest_ul_res_t* eo) {\n"
            "  srsran_hip_chest_ul_t est = {3, {0.3333f, 1 - 2 * 0.3333f, 0.3333f}, 1, pregen->r[0][3][g->L_prb]};\n"
            "  const cf_t* grids[1] = {sf_symbols}; cf_t* ces[1] = {ce}; srsran_softbuffer_rx_t* sbs[1] = {sb}; uint8_t* datas[1] = {data};\n"
            "  return srsran_hip_chest_ul_estimate_pusch(g, &est, sf_symbols, ce, eo) + srsran_hip_chest_ul_estimate_pusch(g, &est, sf_symbols, NULL, eo) +\n"
            "         srsran_hip_chest_ul_estimate_pusch_multi(1, g, &est, grids, ces, eo) + srsran_hip_chest_ul_estimate_pusch_multi(1, g, &est, grids, NULL, eo) +\n"
            "         srsran_hip_pusch_decode_est(g, &est, uci, sf_symbols, sb, data, res, uo, eo) +\n"
            "         srsran_hip_pusch_decode_est(g, &est, NULL, sf_symbols, sb, data, res, NULL, eo) +\n"
            "         srsran_hip_pusch_decode_est_multi(1, g, &est, uci, grids, sbs, datas, res, uo, eo); }\n"
            "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "chest_ul_abi.c"), os.path.join(d, "chest_ul_abi")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.call([exe]) == 0


class _Grant:
    """a valid 2-PRB QPSK grant of a 15-PRB cell with sentinels everywhere a call could write"""

    def __init__(self, capi):
        self.rows = np.full(18600, 0x11, np.int16)
        self.keep = np.full(18600 // 8, 0x22, np.uint8)
        self.flags = np.zeros(1, np.bool_)
        self.sb = capi.SoftbufferRx(1, 18600, (C.c_void_p * 1)(self.rows.ctypes.data), (C.c_void_p * 1)(self.keep.ctypes.data),
                                    self.flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
        self.data = np.full(64, 0xEE, np.uint8)
        self.grid = np.zeros(14 * 12 * NOF_PRB, np.complex64)
        self.ce = np.full(14 * 12 * NOF_PRB, 5, np.complex64)
        self.r = np.ones(2 * 12 * L_PRB, np.complex64)
        self.ack = [np.full(64, 0x33, dt) for dt in (np.int16, np.uint8, np.uint32)]
        self.uo = capi.HipPuschUciOut(self.ack[0].ctypes.data, self.ack[1].ctypes.data, self.ack[2].ctypes.data, None, None, None, None)
        self.g = capi.HipPuschRx(capi.HipGrantTb(1, 40, 0, NOF_RE, 1, 4, 0, 1), NOF_PRB, 7, (C.c_uint32 * 2)(3, 3), L_PRB, 0, 0.0, 0)
        self.est = capi.HipChestUl(3, (C.c_float * 3)(0.3333, 1 - 2 * 0.3333, 0.3333), 1, self.r.ctypes.data)
        self.uci = capi.HipPuschUci(0, 0, 0)
        self.res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
        self.eo = (capi.HipChestUlRes * 1)(capi.HipChestUlRes(7, 7, 7, 7, 7, 7))

    def untouched(self):
        return (np.all(self.data == 0xEE) and np.all(self.rows == 0x11) and np.all(self.keep == 0x22) and not self.flags[0] and np.all(self.ce == 5) and
                all(np.all(a == 0x33) for a in self.ack))

    def est_zeroed(self):
        e = self.eo[0]
        return (e.noise_estimate, e.noise_estimate_dbm, e.snr, e.snr_db, e.cfo_hz, e.ta_us) == (0, 0, 0, 0, 0, 0)


def _poke(k, kw):
    for name, v in kw.items():
        if name in ("tbs", "rv", "mod", "nof_re", "llr_is_8bit"):
            setattr(k.g.tb, name, v)
        elif name == "n_prb1":
            k.g.n_prb_tilde[1] = v
        elif name in ("L_prb", "cp_nsymb", "cell_nof_prb"):
            setattr(k.g, name, v)
        elif name == "filter_len":
            k.est.filter_len = v
        elif name == "tap":
            k.est.filter[v[0]] = v[1]
        elif name == "r":
            k.est.r = v
        elif name == "ack":
            k.uci.Q_prime_ack = v
        elif name == "ri_cqi":
            k.uci.Q_prime_ri, k.uci.Q_prime_cqi = v
        elif name == "ack_out":
            k.uo.ack_llr = v


def _one_line(capfd, who, tag):
    err = capfd.readouterr().err
    assert len(err.strip().splitlines()) == 1 and who in err, (tag, err)
    assert not any(w in err.lower() for w in ("hip error", "device", "illegal", "fault")), (tag, err)


EST_BAD = [dict(filter_len=1), dict(filter_len=2), dict(filter_len=4), dict(tap=(0, float("nan"))), dict(tap=(1, float("inf"))), dict(tap=(2, float("-inf"))), dict(r=None)]
GEOMETRY_BAD = [dict(L_prb=7), dict(L_prb=0), dict(cp_nsymb=5), dict(cell_nof_prb=4), dict(n_prb1=14)]


def test_stage_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(multi, null=None, **kw):
        k = _Grant(capi)
        _poke(k, kw)
        if multi:
            args = [1, C.pointer(k.g), C.pointer(k.est), (C.c_void_p * 1)(k.grid.ctypes.data), (C.c_void_p * 1)(k.ce.ctypes.data), k.eo]
            if null == "grid_entry":
                args[3] = (C.c_void_p * 1)(None)
            elif null is not None:
                args[1 + null] = None
            rc = L.srsran_hip_chest_ul_estimate_pusch_multi(*args)
        else:
            args = [C.byref(k.g), C.byref(k.est), k.grid.ctypes.data, k.ce.ctypes.data, k.eo]
            if null is not None:
                args[null] = None
            rc = L.srsran_hip_chest_ul_estimate_pusch(*args)
        assert k.untouched()
        return rc, k

    for multi in (False, True):
        for kw in EST_BAD + GEOMETRY_BAD + [dict(null=0), dict(null=1), dict(null=2)] + ([dict(null="grid_entry")] if multi else []):
            capfd.readouterr()
            rc, k = call(multi, **kw)
            assert rc == INV and k.est_zeroed(), (multi, kw)
            _one_line(capfd, "srsran_hip_chest_ul_estimate_pusch", (multi, kw))
    capfd.readouterr()
    assert L.srsran_hip_chest_ul_estimate_pusch(None, None, None, None, None) == INV  # (no out: nothing to zero)
    _one_line(capfd, "srsran_hip_chest_ul_estimate_pusch", "all null")
    assert L.srsran_hip_chest_ul_estimate_pusch_multi(0, None, None, None, None, None) == 0  # no grant: nothing to do
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for multi in (False, True):
            rc, k = call(multi)
            assert rc == capi.SRSRAN_ERROR and k.est_zeroed()
        rc, k = call(False, filter_len=0)
        assert rc == capi.SRSRAN_ERROR


def test_grant_call_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(multi, null=None, no_uci=False, **kw):
        k = _Grant(capi)
        _poke(k, kw)
        uci = None if no_uci else C.pointer(k.uci)
        if multi:
            args = [1, C.pointer(k.g), C.pointer(k.est), uci, (C.c_void_p * 1)(k.grid.ctypes.data), (C.POINTER(capi.SoftbufferRx) * 1)(C.pointer(k.sb)),
                    (C.c_void_p * 1)(k.data.ctypes.data), k.res, C.pointer(k.uo), k.eo]
            if null in ("grid", "sb", "data"):
                i = {"grid": 4, "sb": 5, "data": 6}[null]
                args[i] = type(args[i])(None)
            elif null is not None:
                args[1 + null] = None
            rc = L.srsran_hip_pusch_decode_est_multi(*args)
        else:
            args = [C.byref(k.g), C.byref(k.est), uci, k.grid.ctypes.data, C.pointer(k.sb), k.data.ctypes.data, k.res, C.pointer(k.uo), k.eo]
            if null is not None:
                args[null] = None
            rc = L.srsran_hip_pusch_decode_est(*args)
        assert k.untouched()
        return rc, k

    # what the twin (srsran_hip_pusch_decode_uci) refuses: the transport block, the allocation, the control-information rules
    twins = [dict(tbs=41), dict(rv=4), dict(mod=4), dict(mod=0), dict(tbs=0), dict(nof_re=100), dict(nof_re=0), dict(ack=4 * 12 * L_PRB + 1), dict(ri_cqi=(NOF_RE - 1, 1)),
             dict(ack=2, ack_out=None), dict(ack=2, llr_is_8bit=1)] + GEOMETRY_BAD
    nulls = {False: [dict(null=0), dict(null=1), dict(null=3), dict(null=4), dict(null=5), dict(null=6), dict(null=8), dict(ack=2, null=7)],
             True: [dict(null=0), dict(null=1), dict(null=3), dict(null=4), dict(null=5), dict(null=6), dict(null=8), dict(null="grid"), dict(null="sb"), dict(null="data"),
                    dict(ack=2, null=7)]}
    for multi in (False, True):
        for kw in EST_BAD + twins + nulls[multi]:
            capfd.readouterr()
            rc, k = call(multi, **kw)
            assert rc == INV, (multi, kw)
            if kw.get("null") != 6:
                r = k.res[0]
                assert r.crc_ok == 0 and r.avg_iterations_block == 0.0 and np.isnan(r.epre), (multi, kw)
            if kw.get("null") != 8:
                assert k.est_zeroed(), (multi, kw)
            _one_line(capfd, "srsran_hip_pusch_decode", (multi, kw))
    assert L.srsran_hip_pusch_decode_est_multi(0, None, None, None, None, None, None, None, None, None) == 0  # an empty TTI is a no-op
    if L.srsran_hip_device_count() == 0:  # a valid grant gets as far as looking for the device and fails loudly
        for multi in (False, True):
            for kw in (dict(), dict(no_uci=True), dict(ack=2), dict(filter_len=0)):
                rc, k = call(multi, **kw)
                assert rc == capi.SRSRAN_ERROR and k.est_zeroed(), (multi, kw)
