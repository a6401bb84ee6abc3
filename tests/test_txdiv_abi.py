"""CPU-only checks of the transmit-diversity interface (include/srsran_amd/phy_modem_abi.h, phy_chan_abi.h): the library exports its entry points, a plain
C compiler sees the two structs as the ctypes mirror does and takes the reference's own objects (q->symbols, q->ce) for the plane arguments without a
cast, and every refusal comes before the device is looked for.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O

ROOT = O.ROOT

SYMBOLS = ["srsran_predecoding_diversity_multi", "srsran_precoding_diversity", "srsran_layermap_diversity", "srsran_layerdemap_diversity",
           "srsran_hip_predecoding_diversity_multi", "srsran_hip_precoding_diversity", "srsran_hip_layermap_diversity", "srsran_hip_layerdemap_diversity",
           "srsran_hip_pdsch_decode_txdiv", "srsran_hip_pdsch_decode_txdiv_dbg", "srsran_hip_pdsch_encode_txdiv", "srsran_hip_pdsch_encode_txdiv_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_transmit_diversity_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:  # and the mirror has bound them with argument types
        assert getattr(L, s).argtypes is not None, s


def test_struct_layout_matches_ctypes_mirror():
    """sizeof / offsetof of srsran_hip_pdsch_txdiv_rx_t and srsran_hip_pdsch_txdiv_tx_t as plain gcc sees the header = the ctypes mirror in capi.py; the same
    program passes the arrays a reference PDSCH object holds to the receive and transmit calls under -Wall -Werror (it is compiled, the calls are not run)"""
    from srslte_amd import capi

    fields = {"rx": ("srsran_hip_pdsch_txdiv_rx_t", capi.HipPdschTxdivRx), "tx": ("srsran_hip_pdsch_txdiv_tx_t", capi.HipPdschTxdivTx)}
    src = '#include "srsran_amd/phy_chan_abi.h"\n#include <stdio.h>\n#include <stddef.h>\n'
    src += ("struct pdsch_like { cf_t* symbols[SRSRAN_MAX_PORTS]; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; cf_t* x[SRSRAN_MAX_LAYERS]; float* csi[SRSRAN_MAX_CODEWORDS]; };\n"
            "int take(struct pdsch_like* q, srsran_hip_pdsch_txdiv_rx_t* r, srsran_hip_pdsch_txdiv_tx_t* t, srsran_softbuffer_rx_t* sr, srsran_softbuffer_tx_t* st,\n"
            "         uint8_t* data, srsran_hip_grant_res_t* res) {\n"
            "  return srsran_hip_pdsch_decode_txdiv(r, q->symbols, q->ce, sr, data, res) + srsran_hip_pdsch_encode_txdiv(t, st, data, q->symbols) +\n"
            "         srsran_predecoding_diversity_multi(q->symbols, q->ce, q->x, q->csi, 2, 2, 4, 1.0f); }\n")
    src += "int main(int argc, char** argv) {\n  if (argc > 7) { return take(0, 0, 0, 0, 0, 0, 0); }\n"
    for tag, (ctype, mirror) in fields.items():
        src += '  printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (tag, ctype)
        for name, _ in mirror._fields_:
            src += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (tag, name, ctype, name)
    src += '  printf("ports %d\\n", SRSRAN_MAX_PORTS);\n  return 0; }\n'
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "txdiv_layout.c"), os.path.join(d, "txdiv_layout")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())}
    for tag, (_, mirror) in fields.items():
        assert got[tag + ".sizeof"] == C.sizeof(mirror), tag
        for name, _ in mirror._fields_:
            assert got["%s.%s" % (tag, name)] == getattr(mirror, name).offset, (tag, name)
    assert got["ports"] == capi.SRSRAN_MAX_PORTS


def _rx_args(capi, nof_re=72, ports=2, nrx=1, scaling=1.0, null_plane=None):
    """a QPSK grant of one code block (tbs 40) with sentinels everywhere the call could write"""
    y = [np.zeros(nof_re, np.complex64) for _ in range(4)]
    h = [[np.ones(nof_re, np.complex64) for _ in range(4)] for _ in range(4)]
    sym = capi.PlaneArray(*[a.ctypes.data for a in y])
    ce = capi.PlaneMatrix(*[capi.PlaneArray(*[a.ctypes.data for a in row]) for row in h])
    if null_plane == "symbols":
        sym[nrx - 1] = None
    elif null_plane == "ce":
        ce[ports - 1][nrx - 1] = None
    rows = [np.full(18600, 0x11, np.int16)]
    keep = [np.full(18600 // 8, 0x22, np.uint8)]
    flags = np.zeros(1, np.bool_)
    sb = capi.SoftbufferRx(1, 18600, (C.c_void_p * 1)(rows[0].ctypes.data), (C.c_void_p * 1)(keep[0].ctypes.data), flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
    g = capi.HipPdschTxdivRx(capi.HipGrantTb(1, 40, 0, nof_re, 1, 4, 0, 2), ports, nrx, scaling, 0)
    return g, sym, ce, sb, (y, h, rows, keep, flags)


REFUSED = [dict(ports=3), dict(nrx=3), dict(nof_re=73), dict(ports=4, nof_re=74), dict(null_plane="symbols", nrx=2), dict(null_plane="ce", ports=4, nrx=2),
           dict(scaling=0.0), dict(scaling=float("inf")), dict(scaling=float("nan"))]


def test_receive_refusals_need_no_device(L):
    """3 ports, 3 receive antennas, an odd nof_re on 2 ports, nof_re = 74 on 4 ports, a NULL plane inside the used range, scaling 0 / not finite, NULL
    arguments and what every grant call refuses: SRSRAN_ERROR_INVALID_INPUTS with *res = {0, 0, .}, payload and soft buffer untouched"""
    from srslte_amd import capi

    for kw in REFUSED:
        g, sym, ce, sb, keepalive = _rx_args(capi, **kw)
        out = np.full(16, 0xEE, np.uint8)
        for call, extra in ((L.srsran_hip_pdsch_decode_txdiv, ()), (L.srsran_hip_pdsch_decode_txdiv_dbg, (None, None))):
            res = capi.HipGrantRes(7, 7.0, 7.0)
            assert call(C.byref(g), sym, ce, C.byref(sb), O.P(out), C.byref(res), *extra) == capi.SRSRAN_ERROR_INVALID_INPUTS, kw
            assert res.crc_ok == 0 and res.avg_iterations_block == 0.0, kw
            assert np.all(out == 0xEE) and np.all(keepalive[2][0] == 0x11) and np.all(keepalive[3][0] == 0x22) and not keepalive[4][0], kw
    g, sym, ce, sb, keepalive = _rx_args(capi)
    out = np.full(16, 0xEE, np.uint8)
    res = capi.HipGrantRes(7, 7.0, 7.0)
    for args in ((None, sym, ce, C.byref(sb), O.P(out), C.byref(res)), (C.byref(g), None, ce, C.byref(sb), O.P(out), C.byref(res)),
                 (C.byref(g), sym, None, C.byref(sb), O.P(out), C.byref(res)), (C.byref(g), sym, ce, None, O.P(out), C.byref(res)),
                 (C.byref(g), sym, ce, C.byref(sb), None, C.byref(res)), (C.byref(g), sym, ce, C.byref(sb), O.P(out), None)):
        assert L.srsran_hip_pdsch_decode_txdiv(*args) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert res.crc_ok == 0 and res.avg_iterations_block == 0.0
    for field, val in (("tbs", 0), ("tbs", 41), ("rv", 4), ("mod", 5), ("nof_re", 0)):  # tb_valid
        bad = capi.HipPdschTxdivRx.from_buffer_copy(g)
        setattr(bad.tb, field, val)
        assert L.srsran_hip_pdsch_decode_txdiv(C.byref(bad), sym, ce, C.byref(sb), O.P(out), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS, field
    assert np.all(out == 0xEE) and np.all(keepalive[2][0] == 0x11) and not keepalive[4][0]
    if L.srsran_hip_device_count() == 0:  # a valid grant without a device fails loudly: there is no CPU fallback
        assert L.srsran_hip_pdsch_decode_txdiv(C.byref(g), sym, ce, C.byref(sb), O.P(out), C.byref(res)) == capi.SRSRAN_ERROR
        assert np.all(out == 0xEE) and np.all(keepalive[2][0] == 0x11) and not keepalive[4][0]


def test_transmit_refusals_need_no_device(L):
    from srslte_amd import capi

    rows = [np.full(18600, 0x33, np.uint8)]
    sb = capi.SoftbufferTx(1, 18600, (C.c_void_p * 1)(rows[0].ctypes.data))
    planes = [np.full(80, 7, np.complex64) for _ in range(4)]
    pay = np.full(16, 0x5A, np.uint8)

    def call(ports=2, nof_re=72, scaling=1.0, null_plane=False, **tbkw):
        tb = capi.HipGrantTb(1, 40, 0, nof_re, 1, 0, 0, 2)
        for k, v in tbkw.items():
            setattr(tb, k, v)
        g = capi.HipPdschTxdivTx(tb, ports, scaling)
        sym = capi.PlaneArray(*[a.ctypes.data for a in planes])
        if null_plane:
            sym[ports - 1] = None
        one = L.srsran_hip_pdsch_encode_txdiv(C.byref(g), C.byref(sb), O.P(pay), sym)
        many = L.srsran_hip_pdsch_encode_txdiv_multi(1, C.byref(g), (C.POINTER(capi.SoftbufferTx) * 1)(C.pointer(sb)), (C.c_void_p * 1)(pay.ctypes.data),
                                                     (C.POINTER(C.c_void_p) * 1)(C.cast(sym, C.POINTER(C.c_void_p))))
        assert one == many
        return one

    for kw in (dict(ports=3), dict(ports=1), dict(nof_re=73), dict(ports=4, nof_re=74), dict(null_plane=True), dict(ports=4, null_plane=True), dict(scaling=0.0),
               dict(scaling=float("nan")), dict(tbs=41), dict(rv=4), dict(mod=5)):
        assert call(**kw) == capi.SRSRAN_ERROR_INVALID_INPUTS, kw
        assert all(np.all(p == 7) for p in planes) and np.all(rows[0] == 0x33), kw
    g = capi.HipPdschTxdivTx(capi.HipGrantTb(1, 40, 0, 72, 1, 0, 0, 2), 2, 1.0)
    assert L.srsran_hip_pdsch_encode_txdiv(C.byref(g), None, O.P(pay), capi.PlaneArray(*[a.ctypes.data for a in planes])) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert L.srsran_hip_pdsch_encode_txdiv(C.byref(g), C.byref(sb), O.P(pay), None) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert L.srsran_hip_pdsch_encode_txdiv_multi(0, None, None, None, None) == 0  # an empty TTI is a no-op
    if L.srsran_hip_device_count() == 0:
        assert call() == capi.SRSRAN_ERROR
        assert all(np.all(p == 7) for p in planes)


def test_per_stage_refusals_need_no_device(L):
    """the reference-named stages: -1 for a port count other than 2 / 4, more than 2 receive antennas, a symbol count that is not whole pairs / quads (the
    reference would leave the last two symbols of such a 4-port grant unwritten, precoding.c:715)"""
    from srslte_amd import capi

    a = [np.zeros(16, np.complex64) for _ in range(4)]
    arr = capi.PlaneArray(*[v.ctypes.data for v in a])
    mat = capi.PlaneMatrix(*[capi.PlaneArray(*[v.ctypes.data for v in a]) for _ in range(4)])
    x = [np.full(16, 7, np.complex64) for _ in range(4)]
    xs = capi.PlaneArray(*[v.ctypes.data for v in x])
    for nrx, ports, n in ((1, 3, 12), (3, 2, 12), (1, 2, 13), (1, 4, 14), (2, 4, 6), (0, 2, 12)):
        assert L.srsran_predecoding_diversity_multi(arr, mat, xs, None, nrx, ports, n, 1.0) == -1, (nrx, ports, n)
        assert L.srsran_hip_predecoding_diversity_multi(arr, mat, xs, None, nrx, ports, n, 1.0, None) == capi.SRSRAN_ERROR_INVALID_INPUTS, (nrx, ports, n)
    for ports in (1, 3, 5):
        assert L.srsran_precoding_diversity(arr, xs, ports, 4, 1.0) == -1
        assert L.srsran_hip_precoding_diversity(arr, xs, ports, 4, 1.0, None) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert L.srsran_layermap_diversity(O.P(a[0]), xs, 0, 16) == -1 and L.srsran_layermap_diversity(O.P(a[0]), xs, 5, 16) == -1
    assert L.srsran_layerdemap_diversity(xs, O.P(a[0]), 5, 4) == -1
    assert all(np.all(v == 7) for v in x)
    assert L.srsran_predecoding_diversity_multi(arr, mat, xs, None, 1, 2, 0, 1.0) == 0  # nothing to do
    if L.srsran_hip_device_count() == 0:
        assert L.srsran_predecoding_diversity_multi(arr, mat, xs, None, 1, 2, 12, 1.0) == -1
        assert all(np.all(v == 7) for v in x)
