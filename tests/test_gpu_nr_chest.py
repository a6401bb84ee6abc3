"""NR DMRS channel estimation and RE extraction on the device (include/srsran_amd/phy_nr_chan_abi.h: srsran_hip_nr_sch_get, srsran_hip_dmrs_sch_estimate,
srsran_hip_nr_cw_decode_grid{,_dbg,_multi}; srslte_amd/csrc/nr_chest_kernels.hip).

  test_demap_stage                       srsran_hip_nr_sch_get = the model's extraction on every configuration of tests/golden/nr_chest_ref.npz, bit for bit
  test_estimator_against_the_record      the stage on the record's grids: ce to the reference's, the measurements to the float64 model (tests/nr_chest_model.py,
                                         which tests/test_nr_chest_golden.py holds to the same record)
  test_estimator_is_reproducible         the same call twice gives the same bits (every reduction has a fixed order)
  test_grid_call_is_the_two_step_call    srsran_hip_nr_cw_decode_grid_dbg = srsran_hip_nr_cw_decode_dbg fed with what the two stages returned, bit for bit
  test_decodes_from_the_grid_alone       encoded codewords behind a two-tap channel at 20 dB decode from the grid
  test_multi_is_the_single_calls         three codewords on one grid in one call = the three single calls

Measurement bounds (test_estimator_against_the_record): ten times the reference's own worst distance to the model over the record, with a floor of 1e-6
relative (1e-3 Hz for the CFO) -- the reduction order differs between the device's fixed tree and the reference's SIMD accumulators, not the arithmetic.
The noiseless flat case is left out of the noise bound: there noise_estimate is epre * 1e-7 formed as a difference of two float32 numbers 1e-7 apart, one
unit of rsrp's last place is 19 % of it (the reference's own distance), and the device is held to two such units instead."""
import ctypes as C

import numpy as np
import pytest

import nr_chest_model as M
import oracle_api as O
from test_gpu_nr_cw import GUARD, NEW_DATA, QM, Softbuffer
from test_nr_chest_abi import grid_of
from test_nr_chest_golden import case_grid, case_model, distances, nof_cases, record

pytestmark = pytest.mark.gpu

SENTINEL = np.complex64(11 - 13j)
SCALING, MAX_ITER = 0.8, 6
_libm = C.CDLL("libm.so.6")
_libm.log10f.restype, _libm.log10f.argtypes = C.c_float, [C.c_float]


def _lib(hiplib):
    from srslte_amd import capi

    for name in ("srsran_hip_nr_sch_nof_re", "srsran_hip_nr_sch_get", "srsran_hip_dmrs_sch_estimate", "srsran_hip_nr_cw_decode_grid", "srsran_hip_nr_cw_decode_grid_dbg",
                 "srsran_hip_nr_cw_decode_grid_multi"):
        assert hasattr(hiplib, name), "%s is missing from the library" % name  # a missing symbol FAILS
    return hiplib, capi


def _eight(e):
    return np.array([e.noise_estimate, e.noise_estimate_dbm, e.rsrp, e.rsrp_dbm, e.snr_db, e.cfo, e.sync_error], np.float32), int(e.nof_re)


def _estimate(L, capi, g, grid, nof_re, with_ce=True):
    ce = np.full(nof_re + 1, SENTINEL, np.complex64)
    res = capi.HipNrChestRes()
    flat = np.ascontiguousarray(grid).reshape(-1)
    assert L.srsran_hip_dmrs_sch_estimate(C.byref(g), O.P(flat), O.P(ce) if with_ce else None, C.byref(res)) == 0, capi.last_error()
    assert ce[nof_re] == SENTINEL
    return ce[:nof_re], res


def _get(L, capi, g, grid, nof_re):
    out = np.full(nof_re + 1, SENTINEL, np.complex64)
    flat = np.ascontiguousarray(grid).reshape(-1)
    assert L.srsran_hip_nr_sch_get(C.byref(g), O.P(flat), O.P(out)) == nof_re, capi.last_error()
    assert out[nof_re] == SENTINEL  # one element behind the codeword: intact
    return out[:nof_re]


# ---- the stages against the record ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(nof_cases()))
def test_demap_stage(hiplib, i):
    L, capi = _lib(hiplib)
    cfg, grid = case_grid(i)
    want = M.get(grid, cfg)
    got = _get(L, capi, grid_of(capi, cfg), grid, want.size)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), record()["names"][i]


def _bounds(d):
    """ten times the reference's worst distance to the model over the record; floors 1e-6 relative, 1e-3 Hz.  (noise, rsrp, cfo Hz, sync_error)"""
    flat = np.isnan(d["snr_db"])
    dist = np.stack([d["dist_%d" % i] for i in range(len(flat))])
    noise = 10 * dist[~flat, 1].max()
    return max(noise, 1e-6), max(10 * dist[:, 2].max(), 1e-6), max(10 * dist[:, 3].max(), 1e-3), max(10 * dist[:, 4].max(), 1e-6)


def test_estimator_against_the_record(hiplib):
    """measured on an MI355X, worst over the record's 12 cases: ce 7.4e-6 of max |ce| from the reference's rows (bound 1e-4) and
    4.0e-7 from the float64 model; noise_estimate 1.2e-4 relative (bound 1.9e-3: ten times the reference's own 1.9e-4, a difference of two float32 numbers
    at 30 dB), rsrp 2.3e-6 (bound 6.0e-5), sync_error 4.4e-7 (bound 5.1e-6), cfo 3.4e-5 Hz (bound 2.4e-3 Hz); on the flat noiseless case noise_estimate is
    one unit of rsrp's last place from the model's, as the reference's is, and cfo and sync_error are exactly 0"""
    L, capi = _lib(hiplib)
    d = record()
    b_noise, b_rsrp, b_cfo, b_sync = _bounds(d)
    print("bounds: noise %.3g rsrp %.3g cfo %.3g Hz sync %.3g" % (b_noise, b_rsrp, b_cfo, b_sync))
    worst = np.zeros(6)
    for i in range(nof_cases()):
        cfg, grid = case_grid(i)
        m, want = case_model(i), d["ce_%d" % i]
        g = grid_of(capi, cfg)
        ce, res = _estimate(L, capi, g, grid, want.size)
        v, nof_re = _eight(res)
        assert nof_re == want.size == int(d["out_%d" % i][7]), d["names"][i]
        d_ref = np.max(np.abs(ce.astype(np.complex128) - want.astype(np.complex128))) / np.max(np.abs(want))
        out8 = np.array([v[0], v[1], v[2], v[3], v[4], v[5], v[6], nof_re], np.float32)
        dist = distances(m, ce, out8)
        print("%-18s ce %.3g of max|ce| from the reference, %.3g from the model; noise %.3g rsrp %.3g relative, cfo %.3g Hz, sync_error %.3g relative" %
              (d["names"][i], d_ref, dist[0], dist[1], dist[2], dist[3], dist[4]))
        flat = bool(np.isnan(d["snr_db"][i]))
        worst = np.maximum(worst, [d_ref, dist[0], 0.0 if flat else dist[1], dist[2], dist[3], dist[4]])
        assert d_ref <= 1e-4, (d["names"][i], d_ref)
        if flat:
            assert res.cfo == 0 and res.sync_error == 0, (res.cfo, res.sync_error)
            assert abs(float(v[0]) - float(m["noise_estimate"])) <= 2 * float(np.spacing(np.float32(v[2]))), (v[0], m["noise_estimate"])
        else:
            assert dist[1] <= b_noise, (d["names"][i], dist)
        assert dist[2] <= b_rsrp and dist[3] <= b_cfo and dist[4] <= b_sync, (d["names"][i], dist)
        # the dB values from the device's own linear values: exact
        rsrp_dbm = np.float32(np.float32(10.0) * np.float32(_libm.log10f(float(v[2]))))
        noise_dbm = np.float32(np.float32(10.0) * np.float32(_libm.log10f(float(v[0]))))
        assert v[3] == rsrp_dbm and v[1] == noise_dbm and v[4] == np.float32(rsrp_dbm - noise_dbm), (d["names"][i], v)
        # measurements only: the same bits
        _, res2 = _estimate(L, capi, g, grid, 0, with_ce=False)
        v2, nof_re2 = _eight(res2)
        assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and nof_re2 == nof_re, d["names"][i]
    print("worst: ce %.3g (reference) %.3g (model) of max|ce|, noise %.3g, rsrp %.3g, cfo %.3g Hz, sync_error %.3g" % tuple(worst))


def test_estimator_is_reproducible(hiplib):
    L, capi = _lib(hiplib)
    i = list(record()["names"]).index("t1_52of106_hole")
    cfg, grid = case_grid(i)
    g, n = grid_of(capi, cfg), M.nof_re(cfg)
    ce1, r1 = _estimate(L, capi, g, grid, n)
    ce2, r2 = _estimate(L, capi, g, grid, n)
    assert np.array_equal(ce1.view(np.uint32), ce2.view(np.uint32))
    assert np.array_equal(_eight(r1)[0].view(np.uint32), _eight(r2)[0].view(np.uint32))


# ---- codewords on a grid --------------------------------------------------------------------------------------------------------------------------------------

def _prbs(nof_prb, *spans):
    p = np.zeros(nof_prb, np.uint8)
    for a, b in spans:
        p[a:b] = 1
    return p


def _cfg(nof_prb, prb, dmrs_type=0, **kw):
    cfg = dict(nof_prb=nof_prb, scs=1, slot_idx=5, S=0, L=14, dmrs_type=dmrs_type, typeA_pos=2, additional_pos=1, length=1, n_id=77, n_scid=0, cdm=2, beta=1.0, rvd=[],
               prb=prb)
    cfg.update(kw)
    return cfg


def _tb(capi, cfg, mod, rate, rv=NEW_DATA):
    """(HipNrTb, oracle configuration, nof_re) of a codeword that fills the grant"""
    n = M.nof_re(cfg)
    tbs = max(24, int(n * QM[mod] * rate) // 8 * 8)
    blocks = O.sch_nr_tb_info(tbs, rate, mod, n * QM[mod], 1, 0).C
    tbs = (tbs + 24) // (8 * blocks) * (8 * blocks) - 24  # as every transport block size of TS 38.214 5.1.3.2: whole bytes per code block
    ocfg = O.sch_nr_tb_info(tbs, rate, mod, n * QM[mod], 1, 0)
    assert ocfg.C == blocks
    return capi.HipNrTb(rate, tbs, mod, rv, 1, n * QM[mod], 0, 0, 0, 0, 0), ocfg, n


def _channel(cfg, rng, tap=0.4):
    """two taps over the carrier's sub-carriers.  The estimator counts the channel's variation over the band as noise (noise = EPRE - |mean estimate|^2,
    dmrs_sch.c:835-851): about tap^2, which the equaliser then takes as its MMSE term -- the dense constellations get a nearly flat channel"""
    k = np.arange(12 * cfg["nof_prb"])
    return (1.0 + tap * np.exp(2j * np.pi * rng.random()) * np.exp(-2j * np.pi * k * 30e3 * 0.15e-6)) * np.exp(2j * np.pi * rng.random())


def _put_codeword(L, capi, grid, cfg, mod, rate, seed, payload_key, h, snr_db, rng):
    """encode with the library, place with the model's put, DMRS from the model, through h, noise on the grant's rows.  Returns (tb, oracle cfg, nof_re, payload)"""
    tb, ocfg, n = _tb(capi, cfg, mod, rate)
    payload = np.random.default_rng(payload_key).integers(0, 256, tb.tbs // 8).astype(np.uint8)
    x = np.zeros(n, np.complex64)
    tx = capi.HipNrCwTx(capi.HipNrTb(rate, tb.tbs, mod, 0, 1, n * QM[mod], 0, 0, 0, 0, 0), n, seed, 1.0, 0)
    assert L.srsran_hip_nr_cw_encode(C.byref(tx), O.P(payload), O.P(x)) == 0, capi.last_error()
    clean = np.zeros((14, 12 * cfg["nof_prb"]), np.complex128)
    M.put(clean, cfg, x)
    M.put_dmrs(clean, cfg)
    cols = np.repeat(np.flatnonzero(cfg["prb"]) * 12, 12) + np.tile(np.arange(12), int(np.sum(cfg["prb"])))
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    rows = np.arange(14)
    noise = sigma * (rng.standard_normal((14, cols.size)) + 1j * rng.standard_normal((14, cols.size)))
    grid[np.ix_(rows, cols)] = (clean[np.ix_(rows, cols)] * h[cols][None, :] + noise).astype(np.complex64)
    return tb, ocfg, n, payload


def _rx(capi, tb, n, seed, ne=0.0):
    return capi.HipNrCwRx(tb, n, seed, SCALING, MAX_ITER, ne, 0)


def _res4(r):
    return (r.crc_ok, r.all_decoded, r.avg_iter, r.nof_cb)


@pytest.mark.parametrize("mod,snr_db", [(1, 20.0), (1, -8.0), (4, 32.0)])
def test_grid_call_is_the_two_step_call(hiplib, mod, snr_db):
    """verdict, payload, avg_iter, soft bits, soft-buffer rows and measurements; QPSK also where nothing decodes, so that the rows are compared with content"""
    L, capi = _lib(hiplib)
    rng = np.random.default_rng(300 + mod)
    cfg = _cfg(25, _prbs(25, (0, 25)))
    grid = (0.05 * (rng.standard_normal((14, 300)) + 1j * rng.standard_normal((14, 300)))).astype(np.complex64)
    seed = L.srsran_hip_sequence_nr_seed(0x4601, 0, 77)
    tb, ocfg, n, payload = _put_codeword(L, capi, grid, cfg, mod, 0.5, seed, 9, _channel(cfg, rng, 0.4 if mod == 1 else 0.03), snr_db, rng)
    g = grid_of(capi, cfg)
    flat = grid.reshape(-1)
    # two steps
    sym = _get(L, capi, g, grid, n)
    ce, est = _estimate(L, capi, g, grid, n)
    sb1, out1, e1, res1 = Softbuffer(ocfg.C + 1), np.full(tb.tbs // 8 + GUARD, 0xEE, np.uint8), np.full(tb.nof_bits + GUARD, 0x55, np.int8), capi.HipNrTbResult()
    rx = _rx(capi, tb, n, seed, est.noise_estimate)
    assert L.srsran_hip_nr_cw_decode_dbg(C.byref(rx), O.P(sym), O.P(ce), C.byref(sb1.c), O.P(out1), C.byref(res1), O.P(e1)) == 0, capi.last_error()
    # one call; g->noise_estimate is ignored
    sb2, out2, e2, res2 = Softbuffer(ocfg.C + 1), np.full(tb.tbs // 8 + GUARD, 0xEE, np.uint8), np.full(tb.nof_bits + GUARD, 0x55, np.int8), capi.HipNrTbResult()
    est2 = capi.HipNrChestRes()
    rx2 = _rx(capi, tb, n, seed, 123.0)
    assert L.srsran_hip_nr_cw_decode_grid_dbg(C.byref(rx2), C.byref(g), O.P(flat), C.byref(sb2.c), O.P(out2), C.byref(res2), C.byref(est2), O.P(e2)) == 0, capi.last_error()
    print("mod", mod, "snr", snr_db, "result", _res4(res2), "noise", est2.noise_estimate, "snr_db", est2.snr_db)
    assert _res4(res1) == _res4(res2) and np.array_equal(out1, out2) and np.array_equal(e1, e2)
    assert sb2.same_as(sb1.snapshot())
    assert np.array_equal(_eight(est)[0].view(np.uint32), _eight(est2)[0].view(np.uint32)) and est.nof_re == est2.nof_re == n
    assert np.all(e2[tb.nof_bits:] == 0x55) and e2[:tb.nof_bits].any()
    if snr_db > 0:
        assert res2.crc_ok == 1 and np.array_equal(out2[:tb.tbs // 8], payload)
    else:
        assert res2.all_decoded == 0 and np.all(out2 == 0xEE) and any(r.any() for r in sb2.rows)
    # the plain call gives the same
    sb3, out3, res3, est3 = Softbuffer(ocfg.C + 1), np.full(tb.tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult(), capi.HipNrChestRes()
    assert L.srsran_hip_nr_cw_decode_grid(C.byref(rx2), C.byref(g), O.P(flat), C.byref(sb3.c), O.P(out3), C.byref(res3), C.byref(est3)) == 0
    assert _res4(res3) == _res4(res2) and np.array_equal(out3, out2) and sb3.same_as(sb2.snapshot())
    assert np.array_equal(_eight(est3)[0].view(np.uint32), _eight(est2)[0].view(np.uint32))


@pytest.mark.parametrize("dmrs_type", [0, 1])
@pytest.mark.parametrize("shape", ["6", "52"])
def test_decodes_from_the_grid_alone(hiplib, shape, dmrs_type):
    L, capi = _lib(hiplib)
    rng = np.random.default_rng(500 + dmrs_type)
    cfg = _cfg(6, _prbs(6, (0, 6)), dmrs_type, scs=0) if shape == "6" else _cfg(106, _prbs(106, (10, 36), (50, 76)), dmrs_type, S=1, L=12, additional_pos=2)
    w = 12 * cfg["nof_prb"]
    grid = (0.7 * (rng.standard_normal((14, w)) + 1j * rng.standard_normal((14, w)))).astype(np.complex64)  # other users' REs around the grant
    seed = L.srsran_hip_sequence_nr_seed(0x1234, 0, 77)
    tb, ocfg, n, payload = _put_codeword(L, capi, grid, cfg, 1, 0.4, seed, 21, _channel(cfg, rng), 20.0, rng)
    g = grid_of(capi, cfg)
    sb, out, res, est = Softbuffer(ocfg.C + 1), np.full(tb.tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult(), capi.HipNrChestRes()
    rx = _rx(capi, tb, n, seed)
    assert L.srsran_hip_nr_cw_decode_grid(C.byref(rx), C.byref(g), O.P(grid.reshape(-1)), C.byref(sb.c), O.P(out), C.byref(res), C.byref(est)) == 0, capi.last_error()
    print(shape, dmrs_type, _res4(res), "snr_db", est.snr_db, "sync_error", est.sync_error)
    assert res.crc_ok == 1 and res.all_decoded == 1 and np.array_equal(out[:tb.tbs // 8], payload) and np.all(out[tb.tbs // 8:] == 0xEE)
    # |mean of 1 + 0.4 e^(j phi_k)| >= 0.6 whatever the phases; the mean of >= 24 noise terms of variance 0.01 moves it by 0.02 (one sigma): rsrp > 0.52^2.
    # (No bound on snr_db: the estimator counts the channel's variation over the band as noise.)
    assert est.nof_re == n and est.rsrp > 0.27


def test_multi_is_the_single_calls(hiplib):
    """three codewords with disjoint PRB sets and different modulations (and DMRS types) on one grid"""
    L, capi = _lib(hiplib)
    rng = np.random.default_rng(900)
    grants = [(_cfg(106, _prbs(106, (0, 20))), 1, 20.0), (_cfg(106, _prbs(106, (20, 40), (60, 75)), 1, additional_pos=2), 2, 25.0),
              (_cfg(106, _prbs(106, (40, 60), (80, 106)), 0, S=2, L=9), 4, 33.0)]
    grid = np.zeros((14, 12 * 106), np.complex64)
    h = _channel(grants[0][0], rng, 0.03)
    n_cw = len(grants)
    rxs, grids, tbs = (capi.HipNrCwRx * n_cw)(), (capi.HipNrGrid * n_cw)(), []
    for k, (cfg, mod, snr_db) in enumerate(grants):
        seed = L.srsran_hip_sequence_nr_seed(0x2000 + k, 0, 77)
        tb, ocfg, n, payload = _put_codeword(L, capi, grid, cfg, mod, 0.45, seed, 40 + k, h, snr_db, rng)
        rxs[k], grids[k] = _rx(capi, tb, n, seed), grid_of(capi, cfg)
        tbs.append((tb, ocfg, n, payload))
    flat = grid.reshape(-1)
    single = []
    for k in range(n_cw):
        tb, ocfg, n, payload = tbs[k]
        sb, out, res, est = Softbuffer(ocfg.C + 1), np.full(tb.tbs // 8 + GUARD, 0xEE, np.uint8), capi.HipNrTbResult(), capi.HipNrChestRes()
        assert L.srsran_hip_nr_cw_decode_grid(C.byref(rxs[k]), C.byref(grids[k]), O.P(flat), C.byref(sb.c), O.P(out), C.byref(res), C.byref(est)) == 0, capi.last_error()
        assert res.crc_ok == 1 and np.array_equal(out[:tb.tbs // 8], payload), (k, _res4(res))
        single.append((sb, out, res, est))
    sbs = [Softbuffer(t[1].C + 1) for t in tbs]
    outs = [np.full(t[0].tbs // 8 + GUARD, 0xEE, np.uint8) for t in tbs]
    res, est = (capi.HipNrTbResult * n_cw)(), (capi.HipNrChestRes * n_cw)()
    rc = L.srsran_hip_nr_cw_decode_grid_multi(n_cw, rxs, grids, O.P(flat), (C.POINTER(capi.SoftbufferRx) * n_cw)(*[C.pointer(s.c) for s in sbs]),
                                              (C.c_void_p * n_cw)(*[o.ctypes.data for o in outs]), res, est)
    assert rc == 0, capi.last_error()
    for k in range(n_cw):
        sb, out, r, e = single[k]
        assert _res4(res[k]) == _res4(r) and np.array_equal(outs[k], out) and sbs[k].same_as(sb.snapshot()), k
        assert np.array_equal(_eight(est[k])[0].view(np.uint32), _eight(e)[0].view(np.uint32)) and est[k].nof_re == e.nof_re, k
