"""CPU-only checks of the downlink channel estimator's calls (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_dl_estimate,
srsran_hip_pdsch_decode{,_txdiv,_mimo}_est{,_dbg}), in the manner of test_chest_ul_abi.py and test_pdsch_sf_abi.py: the library exports the seven entry
points and the ctypes mirror binds them, the mirror's structs have the layout a C compiler gives the header's, a plain C caller compiles under -Wall -Werror,
and every refusal comes before the device is looked for, with one line on stderr, the results zeroed and nothing else written.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pdsch_map_model as PM
import test_pdsch_sf_abi as S

ROOT = S.ROOT
SYMBOLS = ["srsran_hip_chest_dl_estimate", "srsran_hip_pdsch_decode_est", "srsran_hip_pdsch_decode_est_dbg", "srsran_hip_pdsch_decode_txdiv_est",
           "srsran_hip_pdsch_decode_txdiv_est_dbg", "srsran_hip_pdsch_decode_mimo_est", "srsran_hip_pdsch_decode_mimo_est_dbg"]
NOF_PRB = S.NOF_PRB
PTS = 14 * 12 * NOF_PRB


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
    """sizes and offsets of the three structs as a C compiler lays the header's out"""
    from srslte_amd import capi

    E, T, R = capi.HipChestDl, capi.HipChestDlState, capi.HipChestDlRes
    fields = {"srsran_hip_chest_dl_t": (E, ["nof_rx", "estimator_alg", "filter_coef", "rsrp_neighbour", "decoder_zf", "pilots", "pss_signal"]),
              "srsran_hip_chest_dl_state_t": (T, ["noise_estimate", "cfo"]),
              "srsran_hip_chest_dl_res_t": (R, ["snr_db", "snr_ant_port_db", "rsrp", "rsrp_port_dbm", "rsrq_ant_port_db", "rssi_dbm", "sync_error", "rsrp_pair",
                                                "rsrp_corr_pair", "state"])}
    exprs, want = [], []
    for name, (cls, fs) in fields.items():
        exprs.append("sizeof(%s)" % name)
        want.append(C.sizeof(cls))
        for f in fs:
            exprs.append("offsetof(%s, %s)" % (name, f))
            want.append(getattr(cls, f).offset)
    src = ('#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { size_t v[] = {%s};\n'
           '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]);\n  return 0; }\n' % ", ".join(exprs))
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "chest_dl_layout.c"), os.path.join(d, "chest_dl_layout")
    open(cfile, "w").write(src)
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == want
    assert (C.sizeof(E), C.sizeof(T), C.sizeof(R)) == (96, 68, 4 * (11 + 4 + 6 * 16) + 68)


def test_header_declares_them_for_plain_c():
    """a C file that passes what srsran_ue_dl_decode_fft_estimate's caller holds -- the received grids, the estimator object's pilot table and PSS, the
    result's ce -- compiles under -Wall -Werror and links (not run)"""
    src = '#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n'
    src += ("struct chest_like { cf_t* pilots[2][10]; cf_t pss_signal[62]; };\n"
            "struct res_like { cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; };\n"
            "int take(struct chest_like* q, struct res_like* r, cf_t* sf_symbols[SRSRAN_MAX_PORTS], srsran_hip_pdsch_sf_t* sf, srsran_hip_pdsch_rx_t* a,\n"
            "         srsran_hip_pdsch_txdiv_rx_t* b, srsran_hip_pdsch_mimo_rx_t* c, srsran_softbuffer_rx_t* sb[SRSRAN_MAX_CODEWORDS], uint8_t* data[SRSRAN_MAX_CODEWORDS],\n"
            "         srsran_hip_grant_res_t* res, srsran_hip_chest_dl_state_t* st) {\n"
            "  srsran_hip_chest_dl_t est = {.nof_prb = 25, .nof_ports = 2, .id = 1, .cp_nsymb = 7, .nof_rx = 2, .sf_idx = 5, .estimator_alg = SRSRAN_HIP_ESTIMATOR_ALG_AVERAGE,\n"
            "    .noise_alg = SRSRAN_HIP_NOISE_ALG_REFS, .filter_type = SRSRAN_HIP_CHEST_FILTER_GAUSS, .filter_coef = {4.0f, 1.0f},\n"
            "    .pilots = {q->pilots[0][5], q->pilots[1][5]}, .pss_signal = q->pss_signal};\n"
            "  srsran_hip_chest_dl_res_t m;\n"
            "  int rc = srsran_hip_chest_dl_estimate(&est, st, sf_symbols, r->ce, &m) + srsran_hip_chest_dl_estimate(&est, st, sf_symbols, NULL, &m);\n"
            "  *st = m.state;\n"
            "  return rc + srsran_hip_pdsch_decode_est(a, sf, &est, st, sf_symbols[0], sb[0], data[0], res, &m) +\n"
            "         srsran_hip_pdsch_decode_est_dbg(a, sf, &est, st, sf_symbols[0], sb[0], data[0], res, &m, NULL, NULL, NULL, NULL, NULL, r->ce[0][0]) +\n"
            "         srsran_hip_pdsch_decode_txdiv_est(b, sf, &est, st, sf_symbols, sb[0], data[0], res, &m) +\n"
            "         srsran_hip_pdsch_decode_txdiv_est_dbg(b, sf, &est, st, sf_symbols, sb[0], data[0], res, &m, NULL, NULL, NULL, NULL, NULL, r->ce) +\n"
            "         srsran_hip_pdsch_decode_mimo_est(c, sf, &est, st, sf_symbols, sb, data, res, &m) +\n"
            "         srsran_hip_pdsch_decode_mimo_est_dbg(c, sf, &est, st, sf_symbols, sb, data, res, &m, NULL, NULL, NULL, NULL, NULL, r->ce); }\n"
            "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "chest_dl_abi.c"), os.path.join(d, "chest_dl_abi")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.call([exe]) == 0


class _Est:
    """a valid estimator description of S._sf's cell and subframe (15 PRB, id 1, subframe 1), a state, and a result full of sevens"""

    def __init__(self, capi, ports, nrx):
        self.p = [np.ones(8 * NOF_PRB, np.complex64), np.ones(4 * NOF_PRB, np.complex64)]
        self.pss = np.ones(62, np.complex64)
        c = capi.HipChestDl()
        c.nof_prb, c.nof_ports, c.id, c.cp_nsymb, c.nof_rx, c.sf_idx = NOF_PRB, ports, 1, 7, nrx, 1
        c.estimator_alg, c.noise_alg, c.filter_type = 0, 0, 0
        c.filter_coef[0], c.filter_coef[1] = 4.0, 1.0
        c.cfo_estimate_sf_mask = 0x3FF
        c.pilots[0], c.pilots[1], c.pss_signal = self.p[0].ctypes.data, self.p[1].ctypes.data, self.pss.ctypes.data
        self.c = c
        self.st = capi.HipChestDlState()
        self.res = capi.HipChestDlRes()
        C.memset(C.byref(self.res), 0x40, C.sizeof(self.res))

    def zeroed(self):
        return bytes(self.res) == bytes(C.sizeof(self.res))

    def poke(self, kw):
        for k, v in kw.items():
            if k == "coef":
                self.c.filter_coef[v[0]] = v[1]
            elif k == "pilot_null":
                self.c.pilots[v] = None
            elif k == "state_noise":
                self.st.noise_estimate[v[0]][v[1]] = v[2]
            elif k == "state_cfo":
                self.st.cfo = v
            else:
                setattr(self.c, k, v)


# everything the estimator's description and state are refused for (ports: the cell's)
def _est_bad(ports):
    bad = [dict(nof_prb=5), dict(nof_prb=111), dict(nof_ports=3), dict(nof_ports=0), dict(id=504), dict(cp_nsymb=5), dict(cp_nsymb=8), dict(nof_rx=0), dict(nof_rx=5),
           dict(sf_idx=10), dict(estimator_alg=2), dict(estimator_alg=3), dict(noise_alg=3), dict(filter_type=3), dict(sf_type=1), dict(sf_type=2), dict(tdd_special=1),
           dict(sync_error_enable=1), dict(coef=(0, 9.0)), dict(coef=(0, 64.0)), dict(coef=(0, float("nan"))), dict(coef=(1, float("inf"))),
           dict(filter_type=1, coef=(0, float("nan"))), dict(rsrp_neighbour=2), dict(cfo_estimate_enable=2), dict(noise_alg=1, pss_signal=None), dict(pilot_null=0),
           dict(state_noise=(0, 0, -1.0)), dict(state_noise=(3, 3, float("nan"))), dict(state_cfo=float("inf"))]
    if ports == 4:
        bad += [dict(cfo_estimate_enable=1), dict(pilot_null=1)]
    return bad


def test_stage_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(ports=2, nrx=2, null=None, null_grid=None, **kw):
        e = _Est(capi, ports, nrx)
        e.poke(kw)
        grids = [np.zeros(PTS, np.complex64) for _ in range(4)]
        ce = [[np.full(PTS, 5, np.complex64) for _ in range(4)] for _ in range(4)]
        gp = capi.PlaneArray(*[g.ctypes.data for g in grids])
        if null_grid is not None:
            gp[null_grid] = None
        args = [C.byref(e.c), C.byref(e.st), gp, capi.PlaneMatrix(*[capi.PlaneArray(*[a.ctypes.data for a in row]) for row in ce]), C.byref(e.res)]
        if null is not None:
            args[null] = None
        rc = L.srsran_hip_chest_dl_estimate(*args)
        assert all(np.all(a == 5) for row in ce for a in row) and not any(g.any() for g in grids)
        return rc, e

    for ports in (1, 2, 4):
        for kw in _est_bad(ports) + [dict(null=0), dict(null=1), dict(null=2), dict(null_grid=0), dict(null_grid=1)]:
            capfd.readouterr()
            rc, e = call(ports=ports, **kw)
            assert rc == INV and e.zeroed(), (ports, kw)
            S._one_line(capfd, "srsran_hip_chest_dl_estimate", (ports, kw))
    capfd.readouterr()
    rc, e = call(null=4)  # (no res: nothing to zero)
    assert rc == INV
    S._one_line(capfd, "srsran_hip_chest_dl_estimate", "no res")
    assert L.srsran_hip_chest_dl_estimate(None, None, None, None, None) == INV
    capfd.readouterr()
    # what is not read is not looked at: the second pilot row on 1 or 2 ports, pss_signal without PSS, filter_coef[1] with automatic taps
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for kw in (dict(), dict(pilot_null=1), dict(pss_signal=None), dict(coef=(0, 0.0)), dict(coef=(0, 8.0)), dict(filter_type=2, coef=(0, float("nan"))),
                   dict(ports=4), dict(ports=1, nrx=4, cfo_estimate_enable=1), dict(null=3)):
            rc, e = call(**kw)
            assert rc == capi.SRSRAN_ERROR and e.zeroed(), kw


# what the _est calls add to the estimator's and the twin's refusals: a description that is not the subframe's, a grant that does not span both slots
MISMATCH = [dict(nof_prb=25), dict(id=2), dict(cp_nsymb=6), dict(sf_idx=2), dict(nof_rx=3), dict(decoder_zf=2)]
SF_BAD_TAGS = ("null", "prb_5", "ports_3", "id_504", "cp_8", "sf_10", "nsymb0_8", "lstart_7", "prb_byte_2", "empty", "csi_2", "other_ports")


def _check_est_refused(capfd, capi, who, call, ports, nrx, twins):
    """call(sf_struct, dbg, est, null_est=None, **twin keywords) -> (rc, res[], k): refused with one line, results zeroed, nothing written, with and without _dbg"""
    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    n = PM.indices(S._sf(ports)).size
    good_sf = lambda csi=0: S._struct(capi, S._sf(ports), None, csi)  # noqa: E731

    def refused(tag, rc, res, e, est_checked=True):
        assert rc == INV, tag
        assert all(r.crc_ok == 0 and r.avg_iterations_block == 0.0 and np.isnan(r.epre) for r in res), tag
        assert not est_checked or e.zeroed(), tag
        S._one_line(capfd, who, tag)

    for dbg in (False, True):
        for kw in _est_bad(ports) + MISMATCH:
            capfd.readouterr()
            e = _Est(capi, ports, nrx)
            e.poke(kw)
            rc, res = call(good_sf(dbg), dbg, e)
            refused((kw, dbg), rc, res, e)
        for tag, sf, poke in [b for b in S._bad_descriptions(ports) if b[0] in SF_BAD_TAGS]:
            capfd.readouterr()
            e = _Est(capi, ports, nrx)
            rc, res = call(S._struct(capi, sf, poke), dbg, e)
            refused((tag, dbg), rc, res, e)
        for nsymb in ((7, 6), (6, 7), (7, 0)):  # a grant that leaves symbols of a slot out: the estimator's grids are whole subframes
            capfd.readouterr()
            e = _Est(capi, ports, nrx)
            sfd = S._sf(ports, nsymb=nsymb)
            rc, res = call(S._struct(capi, sfd, None), dbg, e, nof_re=PM.indices(sfd).size)
            refused((nsymb, dbg), rc, res, e)
        for kw in twins + [dict(nof_re=n + 4)]:
            capfd.readouterr()
            e = _Est(capi, ports, nrx)
            rc, res = call(good_sf(), dbg, e, **kw)
            refused((kw, dbg), rc, res, e)
        for null_est in ("est", "state", "est_out"):
            capfd.readouterr()
            e = _Est(capi, ports, nrx)
            rc, res = call(good_sf(), dbg, e, null_est=null_est)
            refused((null_est, dbg), rc, res, e, est_checked=null_est != "est_out")
    if capi.lib().srsran_hip_device_count() == 0:  # a valid grant gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for csi in (0, 1):
            for dbg in (False, True):
                e = _Est(capi, ports, nrx)
                rc, _ = call(good_sf(csi), dbg, e)
                assert rc == capi.SRSRAN_ERROR and e.zeroed(), (csi, dbg)


def _est_args(e, null_est):
    return [None if null_est == "est" else C.byref(e.c), None if null_est == "state" else C.byref(e.st)], [None if null_est == "est_out" else C.byref(e.res)]


def test_single_port_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    n = PM.indices(S._sf(1)).size

    def call(sf, dbg, e, null_est=None, nof_re=n, scaling=1.0, null=None, **tbkw):
        k = S._Grant(capi)
        g = capi.HipPdschRx(S._tb(capi, nof_re, **tbkw), scaling, 0.0)
        res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
        mid, tail = _est_args(e, null_est)
        args = [C.byref(g), C.byref(sf) if sf is not None else None] + mid + [k.y[0].ctypes.data, C.pointer(k.sbs[0]), k.out[0].ctypes.data, res] + tail
        if null is not None:
            args[null] = None
        if dbg:
            rc = L.srsran_hip_pdsch_decode_est_dbg(*args, k.d[0].ctypes.data, k.e[0].ctypes.data, k.c[0].ctypes.data, k.so[0].ctypes.data, k.co[0][0].ctypes.data,
                                                   k.h[0][0].ctypes.data)
        else:
            rc = L.srsran_hip_pdsch_decode_est(*args)
        assert k.untouched() and np.all(k.h[0][0] == 1)
        return rc, res

    twins = [dict(tbs=41), dict(rv=4), dict(mod=5), dict(tbs=0), dict(nof_re=0), dict(scaling=0.0), dict(null=0), dict(null=4), dict(null=5), dict(null=6)]
    _check_est_refused(capfd, capi, "srsran_hip_pdsch_decode_est", call, 1, 1, twins)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_est(None, None, None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS


def test_transmit_diversity_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    def make_call(ports):
        n = PM.indices(S._sf(ports)).size

        def call(sf, dbg, e, null_est=None, nof_re=n, nrx=2, scaling=1.0, g_ports=ports, null_plane=False, **tbkw):
            k = S._Grant(capi)
            if null_plane:
                k.sym[nrx - 1] = None
            g = capi.HipPdschTxdivRx(S._tb(capi, nof_re, **tbkw), g_ports, nrx, scaling, 0)
            res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
            mid, tail = _est_args(e, null_est)
            args = [C.byref(g), C.byref(sf) if sf is not None else None] + mid + [k.sym, C.pointer(k.sbs[0]), k.out[0].ctypes.data, res] + tail
            if dbg:
                rc = L.srsran_hip_pdsch_decode_txdiv_est_dbg(*args, k.d[0].ctypes.data, k.e[0].ctypes.data, k.c[0].ctypes.data, k.sym_out, k.ce_out, k.ce)
            else:
                rc = L.srsran_hip_pdsch_decode_txdiv_est(*args)
            assert k.untouched() and all(np.all(a == 1) for row in k.h for a in row)
            return rc, res

        return call

    twins = [dict(g_ports=1), dict(g_ports=3), dict(nrx=0), dict(nrx=3), dict(nof_re=133), dict(scaling=0.0), dict(scaling=float("nan")), dict(null_plane=True),
             dict(tbs=41), dict(rv=4), dict(mod=5)]
    for ports in (2, 4):
        _check_est_refused(capfd, capi, "srsran_hip_pdsch_decode_txdiv", make_call(ports), ports, 2, twins)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_txdiv_est(None, None, None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS


def test_spatial_multiplexing_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    MUX, CDD = capi.TXSCHEME_SPATIALMUX, capi.TXSCHEME_CDD
    n = PM.indices(S._sf(2)).size

    def call(sf, dbg, e, null_est=None, nof_re=n, nof_tb=2, nof_layers=None, scheme=CDD, cb=0, decoder=1, nrx=2, scaling=1.0, null_plane=False, tb1=None, skip=()):
        k = S._Grant(capi, 2)
        if null_plane:
            k.sym[1] = None
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[None if i in skip else C.pointer(k.sbs[i]) for i in range(2)])
        dp = (C.c_void_p * 2)(k.out[0].ctypes.data, k.out[1].ctypes.data)
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(S._tb(capi, nof_re), S._tb(capi, **dict(dict(nof_re=nof_re, seed=2), **(tb1 or {})))), nof_tb,
                                nof_tb if nof_layers is None else nof_layers, scheme, cb, decoder, nrx, scaling, -1.0)  # (noise_estimate is not read)
        res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
        mid, tail = _est_args(e, null_est)
        args = [C.byref(g), C.byref(sf) if sf is not None else None] + mid + [k.sym, sbp, dp, res] + tail
        if dbg:
            two = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])  # noqa: E731
            rc = L.srsran_hip_pdsch_decode_mimo_est_dbg(*args, two(k.d), two(k.e), two(k.c), k.sym_out, k.ce_out, k.ce)
        else:
            rc = L.srsran_hip_pdsch_decode_mimo_est(*args)
        assert k.untouched() and all(np.all(a == 1) for row in k.h for a in row)
        return rc, res

    twins = [dict(nrx=1), dict(nof_tb=1, nof_layers=2), dict(nof_tb=0, nof_layers=0), dict(scheme=CDD, nof_tb=1), dict(scheme=1), dict(scheme=MUX, cb=3), dict(decoder=2),
             dict(scaling=0.0), dict(null_plane=True), dict(skip=(0, 1)), dict(tb1=dict(llr_is_8bit=1)), dict(tb1=dict(nof_re=n + 2)), dict(tb1=dict(tbs=41)),
             dict(tb1=dict(mod=5))]
    _check_est_refused(capfd, capi, "srsran_hip_pdsch_decode_mimo", call, 2, 2, twins)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_mimo_est(None, None, None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS
