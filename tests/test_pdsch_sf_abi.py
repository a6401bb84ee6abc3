"""CPU-only checks of the PDSCH receive calls that take the subframe grids (include/srsran_amd/phy_chan_abi.h: srsran_hip_pdsch_nof_re, srsran_hip_pdsch_get,
srsran_hip_pdsch_decode{,_txdiv,_mimo}_sf{,_dbg}): the library exports the eight entry points and the ctypes mirror binds them, a plain C compiler takes what a
caller of srsran_pdsch_decode holds (sf_symbols[], channel->ce[][]) for their arguments without a cast, and every refusal -- those of the twins and the ones the
subframe description adds -- comes before the device is looked for, with one line on stderr and nothing written.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import pdsch_map_model as PM

ROOT = O.ROOT

SYMBOLS = ["srsran_hip_pdsch_nof_re", "srsran_hip_pdsch_get", "srsran_hip_pdsch_decode_sf", "srsran_hip_pdsch_decode_sf_dbg", "srsran_hip_pdsch_decode_txdiv_sf",
           "srsran_hip_pdsch_decode_txdiv_sf_dbg", "srsran_hip_pdsch_decode_mimo_sf", "srsran_hip_pdsch_decode_mimo_sf_dbg"]
NOF_PRB = 15


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_sf_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:  # and the mirror has bound them with argument types
        assert getattr(L, s).argtypes is not None, s


def test_mirror_has_the_header_layout():
    from srslte_amd import capi

    # 7 words, nof_symb_slot[2], csi_enable, 2 x 110 bytes: no padding anywhere
    assert C.sizeof(capi.HipPdschSf) == 10 * 4 + 220 and capi.HipPdschSf.prb_idx.offset == 40 and capi.HipPdschSf.csi_enable.offset == 36


def test_header_declares_them_for_plain_c():
    """a C file that includes the header and passes what srsran_pdsch_decode's caller holds -- cf_t* sf_symbols[SRSRAN_MAX_PORTS] and the channel estimator's
    cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] -- and the arrays of a reference PDSCH object to the calls compiles under -Wall -Werror and links (not run)"""
    src = '#include "srsran_amd/phy_chan_abi.h"\n#include <stddef.h>\n'
    src += ("struct chest_like { cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; float noise_estimate; };\n"
            "struct pdsch_like { cf_t* symbols[SRSRAN_MAX_PORTS]; cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; cf_t* d[SRSRAN_MAX_CODEWORDS]; void* e[SRSRAN_MAX_CODEWORDS];\n"
            "  float* csi[SRSRAN_MAX_CODEWORDS]; srsran_softbuffer_rx_t* sr[SRSRAN_MAX_CODEWORDS]; uint8_t* data[SRSRAN_MAX_CODEWORDS]; };\n"
            "int take(struct pdsch_like* q, struct chest_like* channel, cf_t* sf_symbols[SRSRAN_MAX_PORTS], srsran_hip_pdsch_sf_t* sf, srsran_hip_pdsch_rx_t* a,\n"
            "         srsran_hip_pdsch_txdiv_rx_t* b, srsran_hip_pdsch_mimo_rx_t* c, srsran_hip_grant_res_t* res) {\n"
            "  const cf_t* grids[2] = {sf_symbols[0], channel->ce[0][0]};\n"
            "  return srsran_hip_pdsch_nof_re(sf) + srsran_hip_pdsch_get(sf, 2, grids, q->symbols) +\n"
            "         srsran_hip_pdsch_decode_sf(a, sf, sf_symbols[0], channel->ce[0][0], q->sr[0], q->data[0], res) +\n"
            "         srsran_hip_pdsch_decode_sf_dbg(a, sf, sf_symbols[0], channel->ce[0][0], q->sr[0], q->data[0], res, q->d[0], q->e[0], q->csi[0], q->symbols[0], q->ce[0][0]) +\n"
            "         srsran_hip_pdsch_decode_txdiv_sf(b, sf, sf_symbols, channel->ce, q->sr[0], q->data[0], res) +\n"
            "         srsran_hip_pdsch_decode_txdiv_sf_dbg(b, sf, sf_symbols, channel->ce, q->sr[0], q->data[0], res, q->d[0], q->e[0], q->csi[0], q->symbols, q->ce) +\n"
            "         srsran_hip_pdsch_decode_mimo_sf(c, sf, sf_symbols, channel->ce, q->sr, q->data, res) +\n"
            "         srsran_hip_pdsch_decode_mimo_sf_dbg(c, sf, sf_symbols, channel->ce, q->sr, q->data, res, q->d, q->e, q->csi, q->symbols, q->ce) +\n"
            "         srsran_hip_pdsch_decode_mimo_sf_dbg(c, sf, sf_symbols, channel->ce, q->sr, q->data, res, NULL, NULL, NULL, NULL, NULL); }\n"
            "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "pdsch_sf_abi.c"), os.path.join(d, "pdsch_sf_abi")
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, "-L", libdir, "-lsrsran_phy_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.call([exe]) == 0


def _sf(cell_ports, **kw):
    """one PRB of a 15-PRB cell in both slots, subframe 1, two control symbols"""
    prb = np.zeros((2, NOF_PRB), np.uint8)
    prb[:, 3] = 1
    sf = PM.make(NOF_PRB, cell_ports, 1, prb, lstart=2)
    sf.update(kw)
    return sf


def _tb(capi, nof_re, **kw):
    tb = capi.HipGrantTb(1, 40, 0, nof_re, 1, 4, 0, 1)  # QPSK, one code block
    for k, v in kw.items():
        setattr(tb, k, v)
    return tb


class _Grant:
    """soft buffers, payloads, grids and every _dbg output with sentinels everywhere a call could write"""

    def __init__(self, capi, n_sb=1):
        self.rows = [np.full(18600, 0x11, np.int16) for _ in range(n_sb)]
        self.keep = [np.full(18600 // 8, 0x22, np.uint8) for _ in range(n_sb)]
        self.flags = [np.zeros(1, np.bool_) for _ in range(n_sb)]
        self.sbs = [capi.SoftbufferRx(1, 18600, (C.c_void_p * 1)(self.rows[k].ctypes.data), (C.c_void_p * 1)(self.keep[k].ctypes.data),
                                      self.flags[k].ctypes.data_as(C.POINTER(C.c_bool)), False) for k in range(n_sb)]
        self.out = [np.full(16, 0xEE, np.uint8) for _ in range(n_sb)]
        pts = 14 * 12 * NOF_PRB
        self.y = [np.zeros(pts, np.complex64) for _ in range(4)]
        self.h = [[np.ones(pts, np.complex64) for _ in range(4)] for _ in range(4)]
        self.sym = capi.PlaneArray(*[a.ctypes.data for a in self.y])
        self.ce = capi.PlaneMatrix(*[capi.PlaneArray(*[a.ctypes.data for a in row]) for row in self.h])
        # the _dbg outputs
        self.d = [np.full(160, 5, np.complex64) for _ in range(n_sb)]
        self.e = [np.full(320, 0x77, np.int16) for _ in range(n_sb)]
        self.c = [np.full(160, 7, np.float32) for _ in range(n_sb)]
        self.so = [np.full(160, 3, np.complex64) for _ in range(4)]
        self.co = [[np.full(160, 4, np.complex64) for _ in range(4)] for _ in range(4)]
        self.sym_out = capi.PlaneArray(*[a.ctypes.data for a in self.so])
        self.ce_out = capi.PlaneMatrix(*[capi.PlaneArray(*[a.ctypes.data for a in row]) for row in self.co])

    def untouched(self):
        return (all(np.all(o == 0xEE) for o in self.out) and all(np.all(r == 0x11) for r in self.rows) and all(np.all(k == 0x22) for k in self.keep) and
                not any(f[0] for f in self.flags) and all(np.all(a == 5) for a in self.d) and all(np.all(a == 0x77) for a in self.e) and
                all(np.all(a == 7) for a in self.c) and all(np.all(a == 3) for a in self.so) and all(np.all(a == 4) for row in self.co for a in row))


def _one_line(capfd, who, tag):
    err = capfd.readouterr().err
    assert len(err.strip().splitlines()) == 1 and who in err, (tag, err)
    assert not any(w in err.lower() for w in ("hip error", "device", "illegal", "fault")), (tag, err)


def _bad_descriptions(ports):
    """(tag, description or None, what to poke into the ctypes struct afterwards): everything the subframe description is refused for"""
    bad = [("null", None, None), ("prb_5", _sf(ports, nof_prb=5), None), ("prb_111", _sf(ports), ("cell_nof_prb", 111)), ("ports_3", _sf(ports, ports=3), None),
           ("ports_0", _sf(ports, ports=0), None), ("id_504", _sf(ports, cell_id=504), None), ("cp_5", _sf(ports, cp_nsymb=5, nsymb=(5, 5)), None),
           ("cp_8", _sf(ports, cp_nsymb=8), None), ("frame_2", _sf(ports, frame_type=2), None), ("sf_10", _sf(ports, sf_idx=10), None),
           ("nsymb0_8", _sf(ports, nsymb=(8, 7)), None), ("nsymb1_7_ext", _sf(ports, cp_nsymb=6, nsymb=(6, 7)), None), ("lstart_7", _sf(ports, lstart=7), None),
           ("lstart_3_of_3", _sf(ports, lstart=3, nsymb=(3, 0)), None), ("prb_byte_2", _sf(ports), ("prb_byte", 2)), ("prb_byte_2_outside", _sf(ports), ("prb_byte_out", 2)),
           ("empty", _sf(ports, prb=np.zeros((2, NOF_PRB), np.uint8)), None), ("csi_2", _sf(ports), ("csi_enable", 2)),
           ("other_ports", _sf({1: 2, 2: 4, 4: 2}[ports]), None)]
    only1 = np.zeros((2, NOF_PRB), np.uint8)
    only1[1, 3] = 1
    bad.append(("empty_slot1_only_no_symbols", _sf(ports, prb=only1, nsymb=(7, 0)), None))
    return bad


def _struct(capi, sf, poke, csi_enable=0):
    if sf is None:
        return None
    c = PM.to_struct(capi, sf, csi_enable)
    if poke:
        name, v = poke
        if name == "prb_byte":
            c.prb_idx[1][7] = v
        elif name == "prb_byte_out":
            c.prb_idx[0][109] = v
        else:
            setattr(c, name, v)
    return c


def test_count_refuses_an_invalid_description(L):
    from srslte_amd import capi

    assert L.srsran_hip_pdsch_nof_re(None) == -1
    for tag, sf, poke in _bad_descriptions(1):
        if sf is None or tag in ("csi_2", "other_ports"):
            continue
        assert L.srsran_hip_pdsch_nof_re(C.byref(_struct(capi, sf, poke))) == -1, tag
    assert L.srsran_hip_pdsch_nof_re(C.byref(_struct(capi, _sf(1), None))) == PM.indices(_sf(1)).size == 138


def test_get_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    pts = 14 * 12 * NOF_PRB
    grids = [np.zeros(pts, np.complex64) for _ in range(2)]
    outs = [np.full(160, 3, np.complex64) for _ in range(2)]
    gp, op = (C.c_void_p * 2)(*[a.ctypes.data for a in grids]), (C.c_void_p * 2)(*[a.ctypes.data for a in outs])
    for tag, sf, poke in _bad_descriptions(1):
        if tag in ("csi_2", "other_ports"):  # (neither concerns the mapping; csi_enable above 1 is refused all the same)
            continue
        capfd.readouterr()
        c = _struct(capi, sf, poke)
        assert L.srsran_hip_pdsch_get(C.byref(c) if c is not None else None, 2, gp, op) == -1, tag
        _one_line(capfd, "srsran_hip_pdsch_get", tag)
    ok = _struct(capi, _sf(1), None)
    for args in ((2, None, op), (2, gp, None), (2, (C.c_void_p * 2)(grids[0].ctypes.data, None), op), (2, gp, (C.c_void_p * 2)(None, outs[1].ctypes.data))):
        capfd.readouterr()
        assert L.srsran_hip_pdsch_get(C.byref(ok), *args) == -1
        _one_line(capfd, "srsran_hip_pdsch_get", "null")
    assert all(np.all(a == 3) for a in outs)
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly
        assert L.srsran_hip_pdsch_get(C.byref(ok), 2, gp, op) == -1 and all(np.all(a == 3) for a in outs)
    assert L.srsran_hip_pdsch_get(C.byref(ok), 0, gp, op) == 138  # no plane: the count, nothing to do


def _check_refused(capfd, capi, who, call, bads, twins, ports):
    """call(sf_struct, dbg, **twin keywords) -> (rc, results); every entry of bads and twins is refused with one line, both with and without _dbg"""
    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    n = PM.indices(_sf(ports)).size
    for dbg in (False, True):
        for tag, sf, poke in bads:
            for csi in (0, 1):
                capfd.readouterr()
                rc, res = call(_struct(capi, sf, poke, csi), dbg)
                assert rc == INV, (tag, dbg)
                assert all(r.crc_ok == 0 and r.avg_iterations_block == 0.0 and np.isnan(r.epre) for r in res), (tag, dbg)
                _one_line(capfd, who, (tag, dbg))
        for kw in twins + [dict(nof_re=n + 4), dict(nof_re=n - 4)]:  # the twin's own refusals, and a count that is not the description's
            capfd.readouterr()
            rc, res = call(_struct(capi, _sf(ports), None), dbg, **kw)
            assert rc == INV, (kw, dbg)
            assert all(r.crc_ok == 0 and r.avg_iterations_block == 0.0 and np.isnan(r.epre) for r in res), (kw, dbg)
            _one_line(capfd, who, (kw, dbg))
    capfd.readouterr()
    rc, _ = call(_struct(capi, _sf(ports), None), False, nof_re=n + 4)
    assert "expecting %d symbols but got %d" % (n + 4, n) in capfd.readouterr().err


def test_single_port_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    n = PM.indices(_sf(1)).size

    def call(sf, dbg, nof_re=n, scaling=1.0, null=None, **tbkw):
        k = _Grant(capi)
        g = capi.HipPdschRx(_tb(capi, nof_re, **tbkw), scaling, 0.0)
        res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
        args = [C.byref(g), C.byref(sf) if sf is not None else None, k.y[0].ctypes.data, k.h[0][0].ctypes.data, C.pointer(k.sbs[0]), k.out[0].ctypes.data, res]
        if null is not None:
            args[null] = None
        if dbg:
            rc = L.srsran_hip_pdsch_decode_sf_dbg(*args, k.d[0].ctypes.data, k.e[0].ctypes.data, k.c[0].ctypes.data, k.so[0].ctypes.data, k.co[0][0].ctypes.data)
        else:
            rc = L.srsran_hip_pdsch_decode_sf(*args)
        assert k.untouched()
        return rc, res

    twins = [dict(tbs=41), dict(rv=4), dict(mod=5), dict(tbs=0), dict(nof_re=0), dict(scaling=0.0), dict(null=0), dict(null=2), dict(null=3), dict(null=4), dict(null=5)]
    _check_refused(capfd, capi, "srsran_hip_pdsch_decode_sf", call, _bad_descriptions(1), twins, 1)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_sf(None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS
    if L.srsran_hip_device_count() == 0:  # a valid grant gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for csi in (0, 1):
            for dbg in (False, True):
                assert call(_struct(capi, _sf(1), None, csi), dbg)[0] == capi.SRSRAN_ERROR


def test_transmit_diversity_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    def make_call(ports):
        n = PM.indices(_sf(ports)).size

        def call(sf, dbg, nof_re=n, nrx=2, scaling=1.0, g_ports=ports, null_plane=None, **tbkw):
            k = _Grant(capi)
            if null_plane == "symbols":
                k.sym[nrx - 1] = None
            elif null_plane == "ce":
                k.ce[ports - 1][0] = None
            g = capi.HipPdschTxdivRx(_tb(capi, nof_re, **tbkw), g_ports, nrx, scaling, 0)
            res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
            args = (C.byref(g), C.byref(sf) if sf is not None else None, k.sym, k.ce, C.pointer(k.sbs[0]), k.out[0].ctypes.data, res)
            if dbg:
                rc = L.srsran_hip_pdsch_decode_txdiv_sf_dbg(*args, k.d[0].ctypes.data, k.e[0].ctypes.data, k.c[0].ctypes.data, k.sym_out, k.ce_out)
            else:
                rc = L.srsran_hip_pdsch_decode_txdiv_sf(*args)
            assert k.untouched()
            return rc, res

        return call

    twins = [dict(g_ports=1), dict(g_ports=3), dict(nrx=0), dict(nrx=3), dict(nof_re=133), dict(scaling=0.0), dict(scaling=float("nan")), dict(null_plane="symbols"),
             dict(null_plane="ce"), dict(tbs=41), dict(rv=4), dict(mod=5)]
    for ports in (2, 4):
        _check_refused(capfd, capi, "srsran_hip_pdsch_decode_txdiv", make_call(ports), _bad_descriptions(ports), twins, ports)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_txdiv_sf(None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS
    if L.srsran_hip_device_count() == 0:
        for ports in (2, 4):
            for csi in (0, 1):
                assert make_call(ports)(_struct(capi, _sf(ports), None, csi), csi == 1)[0] == capi.SRSRAN_ERROR


def test_spatial_multiplexing_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    MUX, CDD = capi.TXSCHEME_SPATIALMUX, capi.TXSCHEME_CDD
    n = PM.indices(_sf(2)).size

    def call(sf, dbg, nof_re=n, nof_tb=2, nof_layers=None, scheme=CDD, cb=0, decoder=1, nrx=2, scaling=1.0, noise=0.0, null_plane=None, tb1=None, skip=()):
        k = _Grant(capi, 2)
        if null_plane == "symbols":
            k.sym[1] = None
        elif null_plane == "ce":
            k.ce[1][0] = None
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[None if i in skip else C.pointer(k.sbs[i]) for i in range(2)])
        dp = (C.c_void_p * 2)(k.out[0].ctypes.data, k.out[1].ctypes.data)
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(_tb(capi, nof_re), _tb(capi, **dict(dict(nof_re=nof_re, seed=2), **(tb1 or {})))), nof_tb,
                                nof_tb if nof_layers is None else nof_layers, scheme, cb, decoder, nrx, scaling, noise)
        res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
        args = (C.byref(g), C.byref(sf) if sf is not None else None, k.sym, k.ce, sbp, dp, res)
        if dbg:
            two = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])  # noqa: E731
            rc = L.srsran_hip_pdsch_decode_mimo_sf_dbg(*args, two(k.d), two(k.e), two(k.c), k.sym_out, k.ce_out)
        else:
            rc = L.srsran_hip_pdsch_decode_mimo_sf(*args)
        assert k.untouched()
        return rc, res

    twins = [dict(nrx=1), dict(nof_tb=1, nof_layers=2), dict(nof_tb=0, nof_layers=0), dict(scheme=CDD, nof_tb=1), dict(scheme=1), dict(scheme=MUX, cb=3), dict(decoder=2),
             dict(scaling=0.0), dict(noise=-0.1), dict(null_plane="symbols"), dict(null_plane="ce"), dict(skip=(0, 1)), dict(tb1=dict(llr_is_8bit=1)), dict(tb1=dict(nof_re=n + 2)),
             dict(tb1=dict(tbs=41)), dict(tb1=dict(mod=5))]
    _check_refused(capfd, capi, "srsran_hip_pdsch_decode_mimo", call, _bad_descriptions(2), twins, 2)
    capfd.readouterr()
    assert L.srsran_hip_pdsch_decode_mimo_sf(None, None, None, None, None, None, None) == capi.SRSRAN_ERROR_INVALID_INPUTS
    if L.srsran_hip_device_count() == 0:
        for kw in (dict(), dict(scheme=MUX, cb=2), dict(scheme=MUX, decoder=0), dict(skip=(1,))):
            for csi in (0, 1):
                assert call(_struct(capi, _sf(2), None, csi), csi == 1, **kw)[0] == capi.SRSRAN_ERROR, kw
