"""The PDSCH receive calls that take the subframe grids (include/srsran_amd/phy_chan_abi.h: srsran_hip_pdsch_get, srsran_hip_pdsch_decode{,_txdiv,_mimo}_sf{,_dbg};
csrc/pdsch_map_kernels.hip).  Grids are random EVERYWHERE, so an RE taken from a wrong place shows.

Which test holds what to what:
  test_get_is_the_gather            srsran_hip_pdsch_get to grid[indices] bit for bit on every case of the reference record (tests/golden/pdsch_map_ref.npz: the
                                    indices are srsran_pdsch_get's own), two planes per call, guard words behind every plane; and on a 110-PRB all-PRB 4-port
                                    subframe with 10 planes (97 workgroups per plane, the plane dimension of the launch)
  test_sf_call_is_its_twin          every path of test_gpu_pdsch_csi.py's PATHS that has estimates: the _sf_dbg call on the grids against the extracted-RE twin (_dbg with
                                    csi_enable 0, _csi_dbg with 1) on model(grid): sym_out and ce_out are the model's gather, e_out, csi_out and res are the twin's, bit
                                    for bit, both soft-bit widths.  Cells: 6 PRB subframe 0 (nearly everything is centre PRBs), 15 PRB subframe 5 (half PRBs), 25 PRB
                                    subframe 1 with a scattered mask, and -- see below -- 15 PRB subframe 0 for the paths that take an odd nof_re
  test_null_outputs_are_skipped     sym_out / ce_out: a NULL array and NULL entries
  test_sf_grant_decodes             one grant per scheme: transmit call -> planes put into random-filled grids through the model's indices, estimates likewise ->
                                    the _sf call returns crc_ok and the payload, and the _sf_dbg call the same result
An odd nof_re: every count a PRB gives on one symbol is even (12, 10 or 8; 6 or 4 for a half PRB) except a half PRB of a one-port cell on a symbol with reference
signals (5), and the synchronisation signals lie on such a symbol only in slot 1 of subframe 0 (the PBCH's l = 0).  So subframe 5 cannot give an odd count on
any path and a 2- or 4-port cell never can (there every count is a multiple of 4): the 15-PRB subframe-5 mask makes nof_re 2 mod 4 on one port, and the
one-port path gets a fourth cell, 15 PRB in subframe 0 with the lower half PRB allocated, whose count is odd.
The transport block of the twin comparison is one small code block that does not decode (random symbols, one iteration): only the front end is looked at."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_api as O
import pdsch_map_model as PM
import spmux_model as M
import test_gpu_pdsch_csi as T
from grant_helpers import _lib, _matrix, _planes, _rx_softbuffer

pytestmark = pytest.mark.gpu
GUARD = np.complex64(-7 + 7j)


def _grid(rng, pts):
    return np.ascontiguousarray(M.cn(rng, pts).astype(np.complex64))


# ---- 1. the stage by itself

def _get(lib, capi, sf, grids):
    n = PM.indices(sf).size
    outs = [np.full(n + 6, GUARD, np.complex64) for _ in grids]
    c = PM.to_struct(capi, sf)
    rc = lib.srsran_hip_pdsch_get(C.byref(c), len(grids), (C.c_void_p * len(grids))(*[g.ctypes.data for g in grids]), (C.c_void_p * len(grids))(*[o.ctypes.data for o in outs]))
    return rc, outs


def test_get_is_the_gather(hiplib):
    lib, capi = _lib()
    z = np.load(os.path.join(O.ROOT, "tests", "golden", "pdsch_map_ref.npz"))
    rng = np.random.default_rng(7)
    for i, row in enumerate(z["cases"]):
        nof_prb, ports, cell_id, cp, ft, sfi, lstart, n0, n1, nof_re = (int(v) for v in row)
        sf = PM.make(nof_prb, ports, cell_id, z["prb_%d" % i], cp, ft, sfi, lstart, (n0, n1))
        idx = np.cumsum(z["step_%d" % i])
        grids = [_grid(rng, PM.grid_points(sf)) for _ in range(2)]
        rc, outs = _get(lib, capi, sf, grids)
        assert rc == nof_re, (i, rc, capi.last_error())
        for g, o in zip(grids, outs):
            assert np.array_equal(o[:nof_re].view(np.uint64), g[idx].view(np.uint64)), (i, row)
            assert np.all(o[nof_re:] == GUARD), i


def test_get_on_the_widest_cell_with_ten_planes(hiplib):
    lib, capi = _lib()
    sf = PM.make(110, 4, 5, np.ones((2, 110), np.uint8), sf_idx=0, lstart=1)
    idx = PM.indices(sf)
    rng = np.random.default_rng(8)
    grids = [_grid(rng, PM.grid_points(sf)) for _ in range(10)]
    rc, outs = _get(lib, capi, sf, grids)
    assert rc == idx.size and idx.size > 96 * 16 * 8, capi.last_error()
    for p, (g, o) in enumerate(zip(grids, outs)):
        assert np.array_equal(o[:idx.size].view(np.uint64), g[idx].view(np.uint64)), p
        assert np.all(o[idx.size:] == GUARD), p


# ---- 2. the grant calls against their twins

SF_PATHS = [p for p in T.PATHS if p != "single_csi"]  # (the "already equalised" form has no grid)


def _mask_15(ports):
    """15 PRB, subframe 5: both half PRBs (4 and 10), a centre PRB and some outside, different in the two slots; nof_re = 2 mod 4 on one port (on 2 and 4 ports
    every count is a multiple of 4: 12 or 8 per symbol, 6 + 6 for a half PRB's two symbols)"""
    prb = np.zeros((2, 15), np.uint8)
    prb[0, [0, 4, 7, 10, 13]] = 1
    prb[1, [1, 4, 10, 14]] = 1
    return prb


@functools.lru_cache(maxsize=None)
def _cell(name, ports):
    rng = np.random.default_rng(len(name) + ports)
    if name == "prb6_sf0":
        return PM.make(6, ports, 13, np.ones((2, 6), np.uint8), sf_idx=0, lstart=2)
    if name == "prb15_sf5":
        return PM.make(15, ports, 8, _mask_15(ports), sf_idx=5, lstart=1)
    if name == "prb15_sf0_odd":
        prb = np.zeros((2, 15), np.uint8)
        prb[:, [2, 4, 5]] = 1  # PRB 4 is the lower half PRB: 5 REs on the PBCH's first symbol
        return PM.make(15, ports, 8, prb, sf_idx=0, lstart=3)
    prb = (rng.random((2, 25)) < 0.4).astype(np.uint8)
    prb[0, [0, 24]] = 1
    prb[1, [0, 24]] = (0, 1)
    return PM.make(25, ports, 302, prb, sf_idx=1, lstart=3)


def _cases():
    cases = []
    for path in SF_PATHS:
        cases += [(path, cell) for cell in ("prb6_sf0", "prb15_sf5", "prb25_sf1")]
    return cases + [("single_ce", "prb15_sf0_odd")]


def test_cells_have_the_counts_they_should():
    for path, cell in _cases():
        kind, ports, nrx, mimo, odd = T.PATHS[path]
        n = PM.indices(_cell(cell, ports)).size
        assert n % ports == 0 and n > 0, (path, cell, n)
        if cell == "prb15_sf5":
            assert n % 4 == (2 if ports == 1 else 0), (path, n)
        if cell == "prb15_sf0_odd":
            assert odd and n % 2 == 1, (path, n)


def _call_sf(lib, capi, path, sfd, csi, dbg, gy, gh, tbm, llr8, iters=1, null=None):
    """the _sf call of `path` on grids gy [nrx][pts], gh [ports][nrx][pts].  Returns ([(crc_ok, avg, data, e_out, csi_out) per codeword], sym_out [nrx][n], ce_out
    [ports][nrx][n]); the guard words behind every output are checked here.  null: "ce_out" (the array) or "entries" (sym_out[nrx - 1] and ce_out[0][0])"""
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    nof_re = PM.indices(sfd).size
    sf = PM.to_struct(capi, sfd, csi)
    dt = np.int8 if llr8 else np.int16
    sbs = [_rx_softbuffer(capi, O.cbsegm(tbs)["C"], dt) for _, tbs in tbm]
    data = [np.full(tbs // 8 + 16, 0xA5, np.uint8) for _, tbs in tbm]
    e_out = [np.full(nof_re * O.QM[mod] + 16, T.E_GUARD, dt) for mod, _ in tbm]
    c_out = [np.full(nof_re + 8, T.C_GUARD, np.float32) for _ in tbm]
    so = np.full((nrx, nof_re + 4), GUARD, np.complex64)
    co = np.full((ports, nrx, nof_re + 4), GUARD, np.complex64)
    tbs_ = [capi.HipGrantTb(mod, tbs, 0, nof_re, T._seed(k), iters, 1 if llr8 else 0, 2 if kind == "txdiv" else 1) for k, (mod, tbs) in enumerate(tbm)]
    sop, cop = _planes(capi, list(so)), _matrix(capi, co)
    if null == "entries":
        sop[nrx - 1] = None
        cop[0][0] = None
    if kind == "single":
        g = capi.HipPdschRx(tbs_[0], T.SCALING, 0.02)
        res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
        args = (C.byref(g), C.byref(sf), O.P(gy[0]), O.P(gh[0][0]), C.byref(sbs[0][0]), O.P(data[0]), res)
        if dbg:
            rc = lib.srsran_hip_pdsch_decode_sf_dbg(*args, None, O.P(e_out[0]), O.P(c_out[0]), None if null == "entries" else O.P(so[0]),
                                                    None if null else O.P(co[0][0]))
        else:
            rc = lib.srsran_hip_pdsch_decode_sf(*args)
    elif kind == "txdiv":
        g = capi.HipPdschTxdivRx(tbs_[0], ports, nrx, T.SCALING, 0)
        res = (capi.HipGrantRes * 1)(capi.HipGrantRes(7, 7.0, 7.0))
        args = (C.byref(g), C.byref(sf), _planes(capi, list(gy)), _matrix(capi, gh), C.byref(sbs[0][0]), O.P(data[0]), res)
        if dbg:
            rc = lib.srsran_hip_pdsch_decode_txdiv_sf_dbg(*args, None, O.P(e_out[0]), O.P(c_out[0]), sop, None if null == "ce_out" else cop)
        else:
            rc = lib.srsran_hip_pdsch_decode_txdiv_sf(*args)
    else:
        scheme, layers, cb, dec, noise = mimo
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), len(tbm), layers, scheme, cb, dec, 2, T.SCALING, noise)
        res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbs])
        args = (C.byref(g), C.byref(sf), _planes(capi, list(gy)), _matrix(capi, gh), sbp, (C.c_void_p * 2)(*[a.ctypes.data for a in data]), res)
        if dbg:
            ep, cp = (C.c_void_p * 2)(*[a.ctypes.data for a in e_out]), (C.c_void_p * 2)(*[a.ctypes.data for a in c_out])
            rc = lib.srsran_hip_pdsch_decode_mimo_sf_dbg(*args, None, ep, cp, sop, None if null == "ce_out" else cop)
        else:
            rc = lib.srsran_hip_pdsch_decode_mimo_sf(*args)
    assert rc == 0, (path, csi, dbg, capi.last_error())
    assert np.all(so[:, nof_re:] == GUARD) and np.all(co[:, :, nof_re:] == GUARD), path
    out = []
    for k, (mod, _) in enumerate(tbm):
        nbits = nof_re * O.QM[mod]
        assert np.all(e_out[k][nbits:] == T.E_GUARD) and np.all(c_out[k][nof_re:] == T.C_GUARD), (path, k)
        if not dbg:
            assert np.all(e_out[k] == T.E_GUARD) and np.all(so == GUARD) and np.all(co == GUARD), (path, k)
        if not (csi and dbg):
            assert np.all(c_out[k] == T.C_GUARD), (path, k)  # csi_out is only written with csi_enable
        out.append((res[k].crc_ok, res[k].avg_iterations_block, data[k], e_out[k][:nbits].copy(), c_out[k][:nof_re].copy()))
    return out, so[:, :nof_re], co[:, :, :nof_re]


def _grids_of(rng, path, sfd, y=None, h=None):
    """random grids; y [nrx][n] / h [ports][nrx][n], when given, are put at the grant's REs"""
    kind, ports, nrx, _, _ = T.PATHS[path]
    pts, idx = PM.grid_points(sfd), PM.indices(sfd)
    gy = np.ascontiguousarray(M.cn(rng, (nrx, pts)).astype(np.complex64))
    gh = np.ascontiguousarray((0.9 + 0.3 * M.cn(rng, (ports, nrx, pts))).astype(np.complex64))
    if y is not None:
        gy[:, idx] = y
        gh[:, :, idx] = h
    return gy, gh, idx


@pytest.mark.parametrize("path,cell", _cases(), ids=["%s_%s" % c for c in _cases()])
def test_sf_call_is_its_twin(hiplib, path, cell):
    lib, capi = _lib()
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    sfd = _cell(cell, ports)
    rng = np.random.default_rng(len(path) * 31 + len(cell))
    ncw = mimo[1] if mimo else 1
    for llr8 in (False, True):
        for csi in (0, 1):
            tbm = tuple(((len(path) + 2 * k + csi + (3 if llr8 else 0)) % 5, 328) for k in range(ncw))
            gy, gh, idx = _grids_of(rng, path, sfd)
            y, h = np.ascontiguousarray(gy[:, idx]), np.ascontiguousarray(gh[:, :, idx])
            got, so, co = _call_sf(lib, capi, path, sfd, csi, True, gy, gh, tbm, llr8)
            twin = T._call(lib, capi, path, bool(csi), True, y, h, None, tbm, idx.size, llr8, iters=1)
            assert np.array_equal(so.view(np.uint64), y.view(np.uint64)), (llr8, csi)
            assert np.array_equal(co.view(np.uint64), h.view(np.uint64)), (llr8, csi)
            for k in range(ncw):
                assert np.array_equal(got[k][3], twin[k][3]), (llr8, csi, k, int(np.count_nonzero(got[k][3] != twin[k][3])))
                assert np.any(got[k][3] != T.E_GUARD)
                if csi:
                    assert np.array_equal(got[k][4].view(np.uint32), twin[k][4].view(np.uint32)), (llr8, csi, k)
                assert got[k][0] == twin[k][0] and got[k][1] == twin[k][1] and np.array_equal(got[k][2], twin[k][2]), (llr8, csi, k)


@pytest.mark.parametrize("path", ["single_ce", "txdiv_4x2", "cdd"])
def test_null_outputs_are_skipped(hiplib, path):
    lib, capi = _lib()
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    sfd = _cell("prb15_sf5", ports)
    rng = np.random.default_rng(3 + ports)
    tbm = ((1, 328),) * (mimo[1] if mimo else 1)
    gy, gh, idx = _grids_of(rng, path, sfd)
    for null in ("ce_out", "entries"):
        _, so, co = _call_sf(lib, capi, path, sfd, 1, True, gy, gh, tbm, False, null=null)
        for r in range(nrx):
            want = GUARD if (null == "entries" and r == nrx - 1) else gy[r, idx]
            assert np.all(so[r] == want), (null, r)
        for k in range(ports):
            for r in range(nrx):
                skipped = null == "ce_out" or (k == 0 and r == 0)
                assert np.all(co[k, r] == (GUARD if skipped else gh[k, r, idx])), (null, k, r)


# ---- 3. loopback

@pytest.mark.parametrize("path", ["single_ce", "txdiv_2x2", "cdd"])
def test_sf_grant_decodes(hiplib, path):
    lib, capi = _lib()
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    prb = np.zeros((2, 25), np.uint8)
    prb[0, 3:17] = 1
    prb[1, 8:22] = 1
    sfd = PM.make(25, ports, 77, prb, sf_idx=5, lstart=2)
    nof_re = PM.indices(sfd).size
    (mod, tbs) = (1, 1000)  # QPSK on about 2000 REs: rate 0.25
    assert 1700 < nof_re < 2300
    tbm = ((mod, tbs),) * (mimo[1] if mimo else 1)
    rng = np.random.default_rng(len(path) + 11)
    pays = [rng.integers(0, 256, t // 8).astype(np.uint8) for _, t in tbm]
    p = T._transmit(lib, capi, path, tbm, nof_re, pays)
    h = T._channel(rng, path, nof_re)
    y = T._receive(rng, h, p, T.NOISE_DB)
    gy, gh, _ = _grids_of(rng, path, sfd, y, h)
    for csi in (0, 1):
        got, _, _ = _call_sf(lib, capi, path, sfd, csi, False, gy, gh, tbm, False, iters=T.ITERS)
        twin, _, _ = _call_sf(lib, capi, path, sfd, csi, True, gy, gh, tbm, False, iters=T.ITERS)
        for k, (_, t) in enumerate(tbm):
            print("%s csi_enable %d codeword %d: crc_ok %d avg_iterations_block %g" % (path, csi, k, got[k][0], got[k][1]))
            assert got[k][0] == 1 and np.array_equal(got[k][2][:t // 8], pays[k]), (csi, k)
            assert twin[k][0] == 1 and twin[k][1] == got[k][1] and np.array_equal(twin[k][2], got[k][2]), (csi, k)
