"""CPU-only checks of the CSI-weighted PDSCH grant calls (include/srsran_amd/phy_chan_abi.h: the _csi forms): the library exports the six entry points and the
ctypes mirror binds them, a plain C compiler takes the reference's own objects (q->symbols, q->ce, q->csi) for their arguments without a cast, and every refusal
-- those of the plain twins and the two the _csi forms add -- comes before the device is looked for.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O

ROOT = O.ROOT

SYMBOLS = ["srsran_hip_pdsch_decode_csi", "srsran_hip_pdsch_decode_csi_dbg", "srsran_hip_pdsch_decode_txdiv_csi", "srsran_hip_pdsch_decode_txdiv_csi_dbg",
           "srsran_hip_pdsch_decode_mimo_csi", "srsran_hip_pdsch_decode_mimo_csi_dbg"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_csi_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:  # and the mirror has bound them with argument types
        assert getattr(L, s).argtypes is not None, s


def test_header_declares_them_for_plain_c():
    """a C file that includes the header and passes the arrays a reference PDSCH object holds to the six calls compiles under -Wall -Werror and links against the
    library (the calls are not run)"""
    src = '#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n'
    src += ("struct pdsch_like { cf_t* symbols[SRSRAN_MAX_PORTS]; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; cf_t* d[SRSRAN_MAX_CODEWORDS]; void* e[SRSRAN_MAX_CODEWORDS];\n"
            "  float* csi[SRSRAN_MAX_CODEWORDS]; srsran_softbuffer_rx_t* sr[SRSRAN_MAX_CODEWORDS]; uint8_t* data[SRSRAN_MAX_CODEWORDS]; };\n"
            "int take(struct pdsch_like* q, srsran_hip_pdsch_rx_t* a, srsran_hip_pdsch_txdiv_rx_t* b, srsran_hip_pdsch_mimo_rx_t* c, srsran_hip_grant_res_t* res) {\n"
            "  return srsran_hip_pdsch_decode_csi(a, q->symbols[0], q->ce[0][0], NULL, q->sr[0], q->data[0], res) +\n"
            "         srsran_hip_pdsch_decode_csi(a, q->d[0], NULL, q->csi[0], q->sr[0], q->data[0], res) +\n"
            "         srsran_hip_pdsch_decode_csi_dbg(a, q->symbols[0], q->ce[0][0], NULL, q->sr[0], q->data[0], res, q->d[0], q->e[0], q->csi[0]) +\n"
            "         srsran_hip_pdsch_decode_txdiv_csi(b, q->symbols, q->ce, q->sr[0], q->data[0], res) +\n"
            "         srsran_hip_pdsch_decode_txdiv_csi_dbg(b, q->symbols, q->ce, q->sr[0], q->data[0], res, q->d[0], q->e[0], q->csi[0]) +\n"
            "         srsran_hip_pdsch_decode_mimo_csi(c, q->symbols, q->ce, q->sr, q->data, res) +\n"
            "         srsran_hip_pdsch_decode_mimo_csi_dbg(c, q->symbols, q->ce, q->sr, q->data, res, q->d, q->e, q->csi); }\n"
            "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0) : 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "csi_abi.c"), os.path.join(d, "csi_abi")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.call([exe]) == 0


def _tb(capi, nof_re=72, **kw):
    tb = capi.HipGrantTb(1, 40, 0, nof_re, 1, 4, 0, 1)  # QPSK, one code block
    for k, v in kw.items():
        setattr(tb, k, v)
    return tb


class _Grant:
    """soft buffer, payload and planes with sentinels everywhere a call could write"""

    def __init__(self, capi, n_sb=1):
        self.rows = [np.full(18600, 0x11, np.int16) for _ in range(n_sb)]
        self.keep = [np.full(18600 // 8, 0x22, np.uint8) for _ in range(n_sb)]
        self.flags = [np.zeros(1, np.bool_) for _ in range(n_sb)]
        self.sbs = [capi.SoftbufferRx(1, 18600, (C.c_void_p * 1)(self.rows[k].ctypes.data), (C.c_void_p * 1)(self.keep[k].ctypes.data),
                                      self.flags[k].ctypes.data_as(C.POINTER(C.c_bool)), False) for k in range(n_sb)]
        self.out = [np.full(16, 0xEE, np.uint8) for _ in range(n_sb)]
        self.y = [np.zeros(80, np.complex64) for _ in range(4)]
        self.h = [[np.ones(80, np.complex64) for _ in range(4)] for _ in range(4)]
        self.sym = capi.PlaneArray(*[a.ctypes.data for a in self.y])
        self.ce = capi.PlaneMatrix(*[capi.PlaneArray(*[a.ctypes.data for a in row]) for row in self.h])

    def untouched(self):
        return (all(np.all(o == 0xEE) for o in self.out) and all(np.all(r == 0x11) for r in self.rows) and all(np.all(k == 0x22) for k in self.keep) and
                not any(f[0] for f in self.flags))


def _one_line(capfd, who, tag):
    err = capfd.readouterr().err
    assert len(err.strip().splitlines()) == 1 and who in err, (tag, err)
    assert not any(w in err.lower() for w in ("hip error", "device", "illegal", "fault")), (tag, err)


def test_single_port_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    csi = np.full(72, 0.5, np.float32)
    e_out, c_out = np.full(72 * 2, 0x77, np.int16), np.full(72, 7, np.float32)

    def call(tb=None, scaling=1.0, ce=True, row=None, dbg=False):
        k = _Grant(capi)
        g = capi.HipPdschRx(tb if tb is not None else _tb(capi), scaling, 0.0)
        res = capi.HipGrantRes(7, 7.0, 7.0)
        args = (C.byref(g), k.y[0].ctypes.data, k.h[0][0].ctypes.data if ce else None, row.ctypes.data if row is not None else None, C.pointer(k.sbs[0]), k.out[0].ctypes.data,
                C.byref(res))
        rc = L.srsran_hip_pdsch_decode_csi_dbg(*args, None, e_out.ctypes.data, c_out.ctypes.data) if dbg else L.srsran_hip_pdsch_decode_csi(*args)
        assert k.untouched() and np.all(e_out == 0x77) and np.all(c_out == 7)
        return rc, res

    for dbg in (False, True):
        # the plain twin's: the grant itself, scaling 0 with an equaliser
        for kw in (dict(tb=_tb(capi, tbs=41)), dict(tb=_tb(capi, rv=4)), dict(tb=_tb(capi, mod=5)), dict(tb=_tb(capi, tbs=0)), dict(tb=_tb(capi, nof_re=0)), dict(scaling=0.0)):
            rc, res = call(dbg=dbg, **kw)
            assert rc == INV and res.crc_ok == 0 and np.isnan(res.epre), kw
        # the two the _csi form adds, one line on stderr each
        bad = csi.copy()
        for tag, kw in (("both", dict(ce=True, row=csi)), ("neither", dict(ce=False, row=None))):
            capfd.readouterr()
            rc, res = call(dbg=dbg, **kw)
            assert rc == INV and res.crc_ok == 0, tag
            _one_line(capfd, "srsran_hip_pdsch_decode_csi", tag)
        for v in (-0.25, float("nan"), float("inf"), -float("inf")):
            for at in (0, 35, 71):
                bad[:] = csi
                bad[at] = v
                capfd.readouterr()
                rc, res = call(dbg=dbg, ce=False, row=bad)
                assert rc == INV and res.crc_ok == 0, (v, at)
                _one_line(capfd, "srsran_hip_pdsch_decode_csi", (v, at))
    k = _Grant(capi)
    g = capi.HipPdschRx(_tb(capi), 1.0, 0.0)
    res = capi.HipGrantRes(7, 7.0, 7.0)
    full = (C.byref(g), k.y[0].ctypes.data, k.h[0][0].ctypes.data, None, C.pointer(k.sbs[0]), k.out[0].ctypes.data, C.byref(res))
    for drop in (0, 1, 4, 5, 6):  # a NULL argument
        assert L.srsran_hip_pdsch_decode_csi(*[None if i == drop else a for i, a in enumerate(full)]) == INV
    if L.srsran_hip_device_count() == 0:  # valid grants get as far as looking for the device and fail loudly (there is no CPU fallback); a zero entry is valid
        zero = csi.copy()
        zero[3] = 0.0
        assert call(ce=True)[0] == capi.SRSRAN_ERROR and call(ce=False, row=zero)[0] == capi.SRSRAN_ERROR


def test_transmit_diversity_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(ports=2, nrx=2, nof_re=72, scaling=1.0, tb=None, null_plane=None, dbg=False):
        k = _Grant(capi)
        if null_plane == "symbols":
            k.sym[nrx - 1] = None
        elif null_plane == "ce":
            k.ce[ports - 1][0] = None
        g = capi.HipPdschTxdivRx(tb if tb is not None else _tb(capi, nof_re), ports, nrx, scaling, 0)
        res = capi.HipGrantRes(7, 7.0, 7.0)
        args = (C.byref(g), k.sym, k.ce, C.pointer(k.sbs[0]), k.out[0].ctypes.data, C.byref(res))
        rc = L.srsran_hip_pdsch_decode_txdiv_csi_dbg(*args, None, None, None) if dbg else L.srsran_hip_pdsch_decode_txdiv_csi(*args)
        assert k.untouched()
        return rc, res

    for dbg in (False, True):
        for kw in (dict(ports=1), dict(ports=3), dict(nrx=0), dict(nrx=3), dict(nof_re=73), dict(ports=4, nof_re=74), dict(scaling=0.0), dict(scaling=float("nan")),
                   dict(scaling=float("inf")), dict(null_plane="symbols"), dict(null_plane="ce"), dict(tb=_tb(capi, tbs=41)), dict(tb=_tb(capi, rv=4)), dict(tb=_tb(capi, mod=5))):
            capfd.readouterr()
            rc, res = call(dbg=dbg, **kw)
            assert rc == INV and res.crc_ok == 0 and res.avg_iterations_block == 0.0 and np.isnan(res.epre), kw
            _one_line(capfd, "srsran_hip_pdsch_decode_txdiv", kw)
    assert L.srsran_hip_pdsch_decode_txdiv_csi(None, None, None, None, None, None) == INV
    if L.srsran_hip_device_count() == 0:
        assert call()[0] == capi.SRSRAN_ERROR and call(ports=4, nrx=1)[0] == capi.SRSRAN_ERROR


def test_spatial_multiplexing_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    MUX, CDD = capi.TXSCHEME_SPATIALMUX, capi.TXSCHEME_CDD

    def call(nof_re=72, nof_tb=2, nof_layers=None, scheme=CDD, cb=0, decoder=1, nrx=2, scaling=1.0, noise=0.0, null_plane=None, tb1=None, skip=(), dbg=False):
        k = _Grant(capi, 2)
        if null_plane == "symbols":
            k.sym[1] = None
        elif null_plane == "ce":
            k.ce[1][0] = None
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[None if i in skip else C.pointer(k.sbs[i]) for i in range(2)])
        dp = (C.c_void_p * 2)(k.out[0].ctypes.data, k.out[1].ctypes.data)
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(_tb(capi, nof_re), tb1 if tb1 is not None else _tb(capi, nof_re, seed=2)), nof_tb,
                                nof_tb if nof_layers is None else nof_layers, scheme, cb, decoder, nrx, scaling, noise)
        res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
        args = (C.byref(g), k.sym, k.ce, sbp, dp, res)
        rc = L.srsran_hip_pdsch_decode_mimo_csi_dbg(*args, None, None, None) if dbg else L.srsran_hip_pdsch_decode_mimo_csi(*args)
        assert k.untouched()
        return rc, res

    refused = [dict(nrx=1), dict(nof_tb=1, nof_layers=2), dict(nof_tb=2, nof_layers=1), dict(nof_tb=0, nof_layers=0), dict(scheme=CDD, nof_tb=1), dict(scheme=1),
               dict(scheme=MUX, cb=3), dict(scheme=MUX, nof_tb=1, cb=4), dict(scheme=CDD, nof_re=73), dict(decoder=2), dict(scaling=0.0), dict(scaling=float("nan")),
               dict(noise=-0.1), dict(noise=float("inf")), dict(null_plane="symbols"), dict(null_plane="ce"), dict(skip=(0, 1)), dict(tb1=_tb(capi, 72, llr_is_8bit=1)),
               dict(tb1=_tb(capi, 72, max_nof_iterations=5)), dict(tb1=_tb(capi, 74)), dict(tb1=_tb(capi, 72, tbs=41)), dict(tb1=_tb(capi, 72, mod=5))]
    for dbg in (False, True):
        for kw in refused:
            capfd.readouterr()
            rc, res = call(dbg=dbg, **kw)
            assert rc == INV, kw
            assert all(r.crc_ok == 0 and r.avg_iterations_block == 0.0 and np.isnan(r.epre) for r in res), kw
            _one_line(capfd, "srsran_hip_pdsch_decode_mimo", kw)
    assert L.srsran_hip_pdsch_decode_mimo_csi(None, None, None, None, None, None) == INV
    if L.srsran_hip_device_count() == 0:
        for kw in (dict(), dict(scheme=MUX, cb=2, nof_re=73), dict(scheme=MUX, decoder=0), dict(skip=(1,))):
            assert call(**kw)[0] == capi.SRSRAN_ERROR, kw
