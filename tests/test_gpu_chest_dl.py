"""Downlink channel estimation on the device (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_dl_estimate, srsran_hip_pdsch_decode{,_txdiv,_mimo}_est{,_dbg};
srslte_amd/csrc/chest_dl_kernels.hip).

  test_stage_against_the_record_and_the_model   the stage on the inputs of every case of tests/golden/chest_dl_ref.npz: the ce grids to the grids the
                                                reference's srsran_chest_dl_estimate_cfg gave and to the float64 model (tests/chest_dl_model.py, which
                                                tests/test_chest_dl_golden.py holds to the same record) within 1e-4 of max |ce|; the per-pair values, what
                                                fill_res sets and the state out to both within 1e-5 relative (dB values as the power ratio they stand for),
                                                cfo within 4e-3 Hz -- the device bounds of test_gpu_chest_ul.py; NAN, +-inf and exact zeros exact
  test_stage_is_reproducible                    the same call twice gives the same bits (the reductions have a fixed order)
  test_null_ce_entries_give_the_same_measurements   ce == NULL and ce with NULL entries: the same res bit for bit, the entries that are there the same
                                                grids, nothing else written

  test_est_call_is_the_two_step_route, test_est_grant_decodes   the grant calls from the grids alone: see the second half of the file

Each case's device result is computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import chest_dl_model as M
import oracle_api as O
import pdsch_map_model as PM
import test_gpu_pdsch_csi as T
from grant_helpers import _lib, _matrix, _planes, _rx_softbuffer
from test_chest_dl_golden import record

pytestmark = pytest.mark.gpu

SENTINEL = np.complex64(11 - 13j)
GRID_BOUND, POWER_BOUND, CFO_BOUND = 1e-4, 1e-5, 4e-3
N_CASES = len(record()["cases"])


@pytest.fixture(scope="module")
def L(hiplib):
    return hiplib


@pytest.fixture(scope="module")
def D():
    return record()


def cfg_struct(capi, cfg, pilots, pss):
    """(srsran_hip_chest_dl_t, the arrays it points to)"""
    keep = [np.ascontiguousarray(pilots[0], np.complex64), np.ascontiguousarray(pilots[1], np.complex64), None if pss is None else np.ascontiguousarray(pss, np.complex64)]
    c = capi.HipChestDl()
    for k in ("nof_prb", "nof_ports", "id", "cp_nsymb", "nof_rx", "sf_idx", "estimator_alg", "noise_alg", "filter_type", "rsrp_neighbour", "cfo_estimate_enable",
              "cfo_estimate_sf_mask"):
        setattr(c, k, int(cfg[k]))
    c.filter_coef[0], c.filter_coef[1] = float(cfg["filter_coef"][0]), float(cfg["filter_coef"][1])
    c.pilots[0], c.pilots[1] = keep[0].ctypes.data, keep[1].ctypes.data
    c.pss_signal = None if keep[2] is None else keep[2].ctypes.data
    return c, keep


def state_struct(capi, state):
    s = capi.HipChestDlState()
    for a in range(4):
        for p in range(4):
            s.noise_estimate[a][p] = float(state["noise"][a][p])
    s.cfo = float(state["cfo"])
    return s


def res_named(r):
    """srsran_hip_chest_dl_res_t by the names of chest_dl_model.unpack"""
    arr = lambda a: np.array([list(row) for row in a], np.float32)  # noqa: E731
    d = {k: np.float32(getattr(r, k)) for k in M.RES_SCALARS}
    d["rsrp_port_dbm"] = np.array(list(r.rsrp_port_dbm), np.float32)
    for k in ("snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db", "rsrp_pair", "rssi_pair", "rsrp_corr_pair"):
        d[k] = arr(getattr(r, k))
    d["noise_pair"], d["cfo_state"] = arr(r.state.noise_estimate), np.float32(r.state.cfo)
    return d


def run_stage(L, cfg, state, grids, pilots, pss, want=None):
    """(ce [port][rx][2 cp_nsymb * 12 nof_prb] filled with SENTINEL where nothing is written, res).  want: None (every pair), "null" (ce == NULL), or
    [port][rx] booleans"""
    from srslte_amd import capi

    c, keep = cfg_struct(capi, cfg, pilots, pss)
    s = state_struct(capi, state)
    g = [np.ascontiguousarray(x, np.complex64) for x in grids]
    before = [x.copy() for x in g]
    gp = (C.c_void_p * 4)(*([x.ctypes.data for x in g] + [None] * (4 - len(g))))
    ports, nrx = cfg["nof_ports"], cfg["nof_rx"]
    ce = np.full((ports, nrx, g[0].size), SENTINEL, np.complex64)
    mat = capi.PlaneMatrix()
    for p in range(ports):
        for a in range(nrx):
            mat[p][a] = ce[p, a].ctypes.data if (want is None or (want != "null" and want[p][a])) else None
    res = capi.HipChestDlRes()
    rc = L.srsran_hip_chest_dl_estimate(C.byref(c), C.byref(s), gp, None if want == "null" else mat, C.byref(res))
    assert rc == 0, capi.last_error()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g, before))  # the grids are only read
    return ce, res


_cache = {}


def device_case(L, d, i):
    if i not in _cache:
        cfg, state, grids, pilots, pss = M.case_of(d, i)
        ce, res = run_stage(L, cfg, state, grids, pilots, pss)
        _cache[i] = (cfg, ce.reshape(cfg["nof_ports"], cfg["nof_rx"], 2 * cfg["cp_nsymb"], 12 * cfg["nof_prb"]), res, M.estimate(cfg, state, grids, pilots, pss))
    return _cache[i]


@pytest.mark.parametrize("i", range(N_CASES))
def test_stage_against_the_record_and_the_model(L, D, i):
    """Worst distances measured on an MI355X over the record's 21 cases: ce grids 3.1e-7 of max |ce| against the record and 2.6e-7 against the
    model (bound 1e-4); power-like values 1.8e-6 relative against either (bound 1e-5); cfo 3.8e-9 Hz (bound 4e-3 Hz); NAN, +-inf and exact zeros: none off."""
    cfg, ce, res, m = device_case(L, D, i)
    assert not np.any(ce == SENTINEL), i  # every point of every grid is written
    got = res_named(res)
    want = M.recorded_ce(D, i)
    dist_ref, dist_model = M.grid_distance(ce, want.astype(np.complex128)), M.grid_distance(ce, m["ce"])
    p_ref, cfo_ref, same_ref = M.scalar_distance(got, M.unpack(D["out_%d" % i], D["state_out_%d" % i]))
    p_mod, cfo_mod, same_mod = M.scalar_distance(got, M.named(m))
    print("case %d %s: grids %.3g (record) %.3g (model) of max|ce|; power-like %.3g (record) %.3g (model) relative; cfo %.3g (record) %.3g (model) Hz" %
          (i, list(D["cases"][i]), dist_ref, dist_model, p_ref, p_mod, cfo_ref, cfo_mod))
    assert np.array_equal(ce == 0, want == 0), i
    assert dist_ref <= GRID_BOUND and dist_model <= GRID_BOUND, (i, dist_ref, dist_model)
    assert p_ref <= POWER_BOUND and p_mod <= POWER_BOUND, (i, p_ref, p_mod)
    assert cfo_ref <= CFO_BOUND and cfo_mod <= CFO_BOUND, (i, cfo_ref, cfo_mod)
    assert same_ref and same_mod, i
    if cfg["estimator_alg"] == M.ALG_AVERAGE:  # one row for the subframe
        assert np.array_equal(ce.view(np.uint32), np.broadcast_to(ce[:, :, :1, :], ce.shape).view(np.uint32)), i


def test_stage_is_reproducible(L, D):
    for i in range(N_CASES):
        cfg, ce, res, _ = device_case(L, D, i)
        _, state, grids, pilots, pss = M.case_of(D, i)
        ce2, res2 = run_stage(L, cfg, state, grids, pilots, pss)
        assert np.array_equal(ce.reshape(-1).view(np.uint32), ce2.reshape(-1).view(np.uint32)), i
        assert bytes(res) == bytes(res2), i


def test_null_ce_entries_give_the_same_measurements(L, D):
    picked = [i for i in range(N_CASES) if D["cases"][i][0] <= 15]  # every small case: all three noise algorithms, subframes 0 and 5 among them
    assert {int(D["cases"][i][6]) for i in picked} == {0, 1, 2}
    for i in picked:
        cfg, ce, res, _ = device_case(L, D, i)
        _, state, grids, pilots, pss = M.case_of(D, i)
        ports, nrx = cfg["nof_ports"], cfg["nof_rx"]
        ce0, res0 = run_stage(L, cfg, state, grids, pilots, pss, want="null")
        assert np.all(ce0 == SENTINEL) and bytes(res0) == bytes(res), i
        want = [[(p + a) % 2 == 1 for a in range(nrx)] for p in range(ports)]  # pair (0, 0) is NULL
        ce1, res1 = run_stage(L, cfg, state, grids, pilots, pss, want=want)
        assert bytes(res1) == bytes(res), i
        for p in range(ports):
            for a in range(nrx):
                if want[p][a]:
                    assert np.array_equal(ce1[p, a].view(np.uint32), ce[p, a].reshape(-1).view(np.uint32)), (i, p, a)
                else:
                    assert np.all(ce1[p, a] == SENTINEL), (i, p, a)


# ---- the grant calls from the grids alone ----------------------------------------------------------------------------------------------------------------------
#   test_est_call_is_the_two_step_route   per grant form (one port, diversity on 2 and 4 ports, CDD with MMSE, one port with zero forcing) on a 15-PRB grant:
#                                         srsran_hip_pdsch_decode{,_txdiv,_mimo}_est_dbg on the received grids = the stage, then the _sf_dbg twin on the stage's ce
#                                         grids and noise_estimate -- soft bits, CSI row, extracted planes, payload, verdict, iterations, ce grids and est_out bit
#                                         for bit; both soft-bit widths, csi_enable 0 and 1
#   test_est_grant_decodes                a grant sent through the library's transmit call and a smooth channel, CRS rows in the grid: crc_ok and the payload from
#                                         the grids alone, and the plain _est call gives what _est_dbg gives

GUARD = np.complex64(-7 + 7j)
EST_PATHS = ["single_ce", "txdiv_2x2", "txdiv_4x1", "cdd"]
NOF_PRB, CELL_ID, SF_IDX = 15, 8, 5


@functools.lru_cache(maxsize=None)
def _scene(path):
    """(sfd, cfg, pilots, gy [nrx][points], tbm, payloads): an all-PRB grant of a 15-PRB cell in subframe 5 (half PRBs, PSS / SSS holes), sent by the library's
    transmit call through a channel that is smooth in frequency and constant in time, noise 25 dB down; the CRS rows of every port in the grid, random points on
    every RE that is neither (read only)"""
    lib, capi = _lib()
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    rng = np.random.default_rng(100 + len(path) + ports)
    sfd = PM.make(NOF_PRB, ports, CELL_ID, np.ones((2, NOF_PRB), np.uint8), sf_idx=SF_IDX, lstart=2)
    idx = PM.indices(sfd)
    tbm = ((1, 1000),) * (mimo[1] if mimo else 1)
    pays = [rng.integers(0, 256, t // 8).astype(np.uint8) for _, t in tbm]
    p = T._transmit(lib, capi, path, tbm, idx.size, pays)
    nre, k = 12 * NOF_PRB, np.arange(12 * NOF_PRB)
    h = np.zeros((ports, nrx, 14, nre), np.complex128)
    for port in range(ports):
        for a in range(nrx):
            taus = np.array([0.0, rng.uniform(0.1e-6, 0.2e-6), rng.uniform(0.2e-6, 0.4e-6)])
            amps = np.array([1.0, 0.4, 0.2]) * np.exp(2j * np.pi * rng.random(3))
            row = (amps[None, :] * np.exp(-2j * np.pi * 15e3 * k[:, None] * taus[None, :])).sum(axis=1)
            h[port, a] = (row / np.sqrt(np.mean(np.abs(row) ** 2)))[None, :]
    hf = h.reshape(ports, nrx, -1)
    sigma = 10 ** (T.NOISE_DB / 20) / np.sqrt(2)
    gy = (0.7 * (rng.standard_normal((nrx, 14 * nre)) + 1j * rng.standard_normal((nrx, 14 * nre)))).astype(np.complex64)
    gy[:, idx] = T._receive(rng, hf[:, :, idx].astype(np.complex64), p, T.NOISE_DB)
    pilots = [np.exp(2j * np.pi * rng.random(n * NOF_PRB)).astype(np.complex64) for n in (8, 4)]
    g3 = gy.reshape(nrx, 14, nre)
    for port in range(ports):
        rows = pilots[port // 2].reshape(M.nof_symbols(port), 2 * NOF_PRB)
        for l in range(M.nof_symbols(port)):
            sym, f0 = M.nsymbol(l, 7, port), M.fidx(CELL_ID, l, port)
            for a in range(nrx):
                g3[a, sym, f0::6] = h[port, a, sym, f0::6] * rows[l] + sigma * (rng.standard_normal(2 * NOF_PRB) + 1j * rng.standard_normal(2 * NOF_PRB))
    cfg = dict(nof_prb=NOF_PRB, nof_ports=ports, id=CELL_ID, cp_nsymb=7, nof_rx=nrx, sf_idx=SF_IDX, estimator_alg=M.ALG_AVERAGE, noise_alg=M.NOISE_REFS,
               filter_type=M.FILTER_GAUSS, filter_coef=np.array([4.0, 1.0], np.float32), rsrp_neighbour=0, cfo_estimate_enable=0, cfo_estimate_sf_mask=0x3FF)
    gy.setflags(write=False)
    return sfd, cfg, pilots, gy, tbm, pays


def _grant(lib, capi, path, sfd, csi, dbg, gy, tbm, llr8, iters, gh=None, noise=0.0, est=None, zf=0):
    """the _sf (gh [ports][nrx][points] and noise given) or the _est (est = (cfg, pilots, state) given) call of `path`, plain or _dbg.  Returns ([(crc_ok, avg,
    data, e_out, csi_out) per codeword], sym_out, ce_out, ce grids or None, est_out or None); guard words are checked here"""
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    nof_re, pts = PM.indices(sfd).size, PM.grid_points(sfd)
    sf = PM.to_struct(capi, sfd, csi)
    dt = np.int8 if llr8 else np.int16
    sbs = [_rx_softbuffer(capi, O.cbsegm(tbs)["C"], dt) for _, tbs in tbm]
    data = [np.full(tbs // 8 + 16, 0xA5, np.uint8) for _, tbs in tbm]
    e_out = [np.full(nof_re * O.QM[mod] + 16, T.E_GUARD, dt) for mod, _ in tbm]
    c_out = [np.full(nof_re + 8, T.C_GUARD, np.float32) for _ in tbm]
    so = np.full((nrx, nof_re + 4), GUARD, np.complex64)
    co = np.full((ports, nrx, nof_re + 4), GUARD, np.complex64)
    cg = np.full((ports, nrx, pts + 4), GUARD, np.complex64)
    tbs_ = [capi.HipGrantTb(mod, tbs, 0, nof_re, T._seed(k), iters, 1 if llr8 else 0, 2 if kind == "txdiv" else 1) for k, (mod, tbs) in enumerate(tbm)]
    gyc = [np.ascontiguousarray(x) for x in gy]
    keep, tail, eo = None, [], None
    if est is not None:
        cfg, pilots, state = est
        c, keep = cfg_struct(capi, cfg, pilots, None)
        c.decoder_zf = zf
        eo = capi.HipChestDlRes()
        mid = [C.byref(c), C.byref(state_struct(capi, state))]
        tail = [C.byref(eo)]
    n_cw = len(tbm)
    res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
    if kind == "single":
        g = capi.HipPdschRx(tbs_[0], T.SCALING, noise if est is None else 123.0)  # (the _est call does not read it)
        outs = [None, O.P(e_out[0]), O.P(c_out[0]), O.P(so[0]), O.P(co[0][0])]
        if est is None:
            fn = lib.srsran_hip_pdsch_decode_sf_dbg if dbg else lib.srsran_hip_pdsch_decode_sf
            args = [C.byref(g), C.byref(sf), O.P(gyc[0]), O.P(np.ascontiguousarray(gh[0][0])), C.byref(sbs[0][0]), O.P(data[0]), res]
        else:
            fn = lib.srsran_hip_pdsch_decode_est_dbg if dbg else lib.srsran_hip_pdsch_decode_est
            args = [C.byref(g), C.byref(sf)] + mid + [O.P(gyc[0]), C.byref(sbs[0][0]), O.P(data[0]), res] + tail
            outs.append(O.P(cg[0][0]))
    else:
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbs] + [None] * (2 - n_cw))
        if kind == "txdiv":
            g = capi.HipPdschTxdivRx(tbs_[0], ports, nrx, T.SCALING, 0)
            mine = [C.byref(sbs[0][0]), O.P(data[0]), res]
            outs = [None, O.P(e_out[0]), O.P(c_out[0]), _planes(capi, list(so)), _matrix(capi, co)]
            name = "srsran_hip_pdsch_decode_txdiv"
        else:
            scheme, layers, cb, dec, _ = mimo
            g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), n_cw, layers, scheme, cb, dec, 2, T.SCALING, noise if est is None else 123.0)
            mine = [sbp, (C.c_void_p * 2)(*[a.ctypes.data for a in data]), res]
            outs = [None, (C.c_void_p * 2)(*[a.ctypes.data for a in e_out]), (C.c_void_p * 2)(*[a.ctypes.data for a in c_out]), _planes(capi, list(so)), _matrix(capi, co)]
            name = "srsran_hip_pdsch_decode_mimo"
        if est is None:
            ghc = np.ascontiguousarray(gh)
            fn = getattr(lib, name + ("_sf_dbg" if dbg else "_sf"))
            args = [C.byref(g), C.byref(sf), _planes(capi, gyc), _matrix(capi, ghc)] + mine
        else:
            fn = getattr(lib, name + ("_est_dbg" if dbg else "_est"))
            args = [C.byref(g), C.byref(sf)] + mid + [_planes(capi, gyc)] + mine + tail
            outs.append(_matrix(capi, cg))
    rc = fn(*(args + (outs if dbg else [])))
    assert rc == 0, (path, csi, dbg, capi.last_error())
    assert np.all(so[:, nof_re:] == GUARD) and np.all(co[:, :, nof_re:] == GUARD) and np.all(cg[:, :, pts:] == GUARD), path
    out = []
    for k, (mod, _) in enumerate(tbm):
        nbits = nof_re * O.QM[mod]
        assert np.all(e_out[k][nbits:] == T.E_GUARD) and np.all(c_out[k][nof_re:] == T.C_GUARD), (path, k)
        if not dbg:
            assert np.all(e_out[k] == T.E_GUARD) and np.all(so == GUARD) and np.all(co == GUARD) and np.all(cg == GUARD), (path, k)
        out.append((res[k].crc_ok, res[k].avg_iterations_block, data[k], e_out[k][:nbits].copy(), c_out[k][:nof_re].copy()))
    return out, so[:, :nof_re], co[:, :, :nof_re], (cg[:, :, :pts] if est is not None else None), eo


ZERO_STATE = {"noise": np.zeros((4, 4), np.float32), "cfo": np.float32(0)}


@pytest.mark.parametrize("path", EST_PATHS + ["single_zf"])
def test_est_call_is_the_two_step_route(hiplib, path):
    lib, capi = _lib()
    zf, path = (1, "single_ce") if path == "single_zf" else (0, path)
    kind, ports, nrx, mimo, _ = T.PATHS[path]
    sfd, cfg, pilots, gy, tbm, _ = _scene(path)
    idx = PM.indices(sfd)
    ce, stage = run_stage(lib, cfg, ZERO_STATE, list(gy), pilots, None)
    noise = 0.0 if (zf or (mimo and mimo[3] != T.M.MMSE)) else float(stage.noise_estimate)
    assert stage.noise_estimate > 0
    for llr8 in (False, True):
        for csi in (0, 1):
            got, so, co, cg, eo = _grant(lib, capi, path, sfd, csi, True, gy, tbm, llr8, T.ITERS, est=(cfg, pilots, ZERO_STATE), zf=zf)
            two, so2, co2, _, _ = _grant(lib, capi, path, sfd, csi, True, gy, tbm, llr8, T.ITERS, gh=ce, noise=noise)
            assert bytes(eo) == bytes(stage), (llr8, csi)
            assert np.array_equal(cg.view(np.uint64), ce.view(np.uint64)), (llr8, csi)
            assert np.array_equal(so.view(np.uint64), so2.view(np.uint64)) and np.array_equal(so.view(np.uint64), np.ascontiguousarray(gy[:, idx]).view(np.uint64))
            assert np.array_equal(co.view(np.uint64), co2.view(np.uint64)) and np.array_equal(co.view(np.uint64), np.ascontiguousarray(ce[:, :, idx]).view(np.uint64))
            for k in range(len(tbm)):
                assert np.array_equal(got[k][3], two[k][3]), (llr8, csi, k, int(np.count_nonzero(got[k][3] != two[k][3])))
                assert np.any(got[k][3] != T.E_GUARD)
                if csi:
                    assert np.array_equal(got[k][4].view(np.uint32), two[k][4].view(np.uint32)), (llr8, csi, k)
                assert got[k][0] == two[k][0] and got[k][1] == two[k][1] and np.array_equal(got[k][2], two[k][2]), (llr8, csi, k)


@pytest.mark.parametrize("path", ["single_ce", "txdiv_2x2", "cdd"])
def test_est_grant_decodes(hiplib, path):
    lib, capi = _lib()
    sfd, cfg, pilots, gy, tbm, pays = _scene(path)
    for csi in (0, 1):
        got, _, _, _, eo = _grant(lib, capi, path, sfd, csi, False, gy, tbm, False, T.ITERS, est=(cfg, pilots, ZERO_STATE))
        dbg, _, _, _, eo2 = _grant(lib, capi, path, sfd, csi, True, gy, tbm, False, T.ITERS, est=(cfg, pilots, ZERO_STATE))
        assert bytes(eo) == bytes(eo2) and eo.noise_estimate > 0 and eo.snr_db > 15, (csi, eo.snr_db)
        for k, (_, t) in enumerate(tbm):
            print("%s csi_enable %d codeword %d: crc_ok %d avg_iterations_block %g, snr_db %.2f" % (path, csi, k, got[k][0], got[k][1], eo.snr_db))
            assert got[k][0] == 1 and np.array_equal(got[k][2][:t // 8], pays[k]), (csi, k)
            assert dbg[k][0] == 1 and dbg[k][1] == got[k][1] and np.array_equal(dbg[k][2], got[k][2]), (csi, k)
