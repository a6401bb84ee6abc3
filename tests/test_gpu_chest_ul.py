"""PUSCH channel estimation on the device (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_ul_estimate_pusch{,_multi}, srsran_hip_pusch_decode_est{,_multi};
srslte_amd/csrc/chest_ul_kernels.hip).

  test_stage_against_the_reference_record   the stage on the inputs of tests/golden/chest_ul_ref.npz: the rows to the rows the reference's
                                            srsran_chest_ul_estimate_pusch gave, the measurements to the float64 model (tests/chest_ul_model.py, which
                                            tests/test_chest_ul_golden.py holds to the same record); single calls and one _multi call over all cases
  test_stage_is_reproducible                the same call twice gives the same bits (the reductions have a fixed order)
  test_est_call_is_the_two_step_call        srsran_hip_pusch_decode_est on the grid = srsran_hip_pusch_decode fed with the ce grid and the noise estimate the
                                            stage returned, bit for bit -- verdict, payload, iterations, EPRE, soft-buffer rows, measurements
  test_est_grant_decodes                    grants with a DMRS row in the grid decode to the payload from the grid alone
  test_est_multi_with_and_without_uci       a TTI in one _est_multi call = the single calls"""
import ctypes as C
import os

import numpy as np
import pytest

import chest_ul_model as M
import oracle_api as O
import test_gpu_chan as T
import test_gpu_pusch_uci as U
from grant_helpers import _rx_softbuffer
from test_chest_ul_golden import case_grid, record

pytestmark = pytest.mark.gpu

W = np.float32(0.3333)
FILTER = (W, np.float32(1) - np.float32(2) * W, W)
_libm = C.CDLL("libm.so.6")
_libm.log10f.restype, _libm.log10f.argtypes = C.c_float, [C.c_float]


def _est(capi, r, filter_on=True, meas_ta_en=1):
    return capi.HipChestUl(3 if filter_on else 0, (C.c_float * 3)(*(FILTER if filter_on else (0, 0, 0))), meas_ta_en, r.ctypes.data)


def _six(e):
    return np.array([e.noise_estimate, e.noise_estimate_dbm, e.snr, e.snr_db, e.cfo_hz, e.ta_us], np.float32)


def _geometry(capi, nof_prb, cp_nsymb, n_prb, L_prb):
    """a grant of which the stage reads the geometry only"""
    return capi.HipPuschRx(capi.HipGrantTb(), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, 0, 0.0, 0)


def _with_dmrs(rng, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, snr_db):
    """the DMRS of a grant put into the grid T._pusch_grid made (it leaves noise there): r through the channel of each slot's reference symbol; returns r"""
    n = 12 * L_prb
    r = np.exp(2j * np.pi * rng.random(2 * n)).astype(np.complex64)
    g, h = grid.reshape(2 * cp_nsymb, 12 * nof_prb), ce.reshape(2 * cp_nsymb, 12 * nof_prb)
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    for s in range(2):
        a, l = 12 * n_prb[s], M.ref_symbol(s, cp_nsymb)
        g[l, a:a + n] = (r[s * n:(s + 1) * n] * h[l, a:a + n] + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return r


# ---- the stage against the record ------------------------------------------------------------------------------------------------------------------------------

SENTINEL = np.complex64(11 - 13j)


def _check_against_record(d, i, ce, six, geometry, filt, meas_ta_en, model, worst):
    nof_prb, cp_nsymb, n_prb, L_prb = geometry
    sm, m = model
    a, n = 12 * n_prb, 12 * L_prb
    g = ce.reshape(2 * cp_nsymb, 12 * nof_prb)
    want = d["ce_%d" % i]
    inside = np.zeros(g.shape, bool)
    inside[:, a:a + n] = True
    assert np.all(g[~inside] == SENTINEL), i  # nothing outside the grant's columns
    for l in range(2 * cp_nsymb):
        assert np.array_equal(g[l, a:a + n].view(np.uint32), g[M.ref_symbol(l // cp_nsymb, cp_nsymb), a:a + n].view(np.uint32)), (i, l)
    rows = np.stack([g[M.ref_symbol(s, cp_nsymb), a:a + n] for s in range(2)])
    dist = [np.max(np.abs(rows.astype(np.complex128) - want.astype(np.complex128))) / np.max(np.abs(want)), 0.0, 0.0, 0.0]
    noise, noise_dbm, snr, snr_db, cfo_hz, ta_us = six
    if filt is None:
        assert noise == 0 and np.isnan(snr) and np.isnan(snr_db) and np.isneginf(noise_dbm), (i, six)
    else:
        dist[1] = abs(float(noise) - float(m["noise_estimate"])) / float(m["noise_estimate"])
        dist[2] = abs(float(snr) - float(m["snr"])) / float(m["snr"])
        # the dB values from the device's own linear values: exact
        assert noise_dbm == np.float32(np.float32(10.0) * np.float32(_libm.log10f(float(noise))) + np.float32(30.0)), (i, six)
        assert snr_db == np.float32(np.float32(10.0) * np.float32(_libm.log10f(float(snr)))), (i, six)
    dist[3] = abs(float(cfo_hz) - float(m["cfo_hz"]))
    print("case %d (L_prb %d, cp %d, filter %d): rows %.3g of max|ce|, noise %.3g, snr %.3g relative, cfo %.3g Hz; ta_us %s (model %s)" %
          (i, L_prb, cp_nsymb, 0 if filt is None else 3, dist[0], dist[1], dist[2], dist[3], ta_us, m["ta_us"]))
    worst[:] = np.maximum(worst, dist)
    assert dist[0] <= 1e-4 and dist[1] <= 1e-5 and dist[2] <= 1e-5 and dist[3] <= 4e-3, (i, dist)
    assert ta_us == m["ta_us"] and ta_us == np.float32(d["out_%d" % i][5]) and (meas_ta_en or ta_us == 0), (i, ta_us, m["ta_us"])


def test_stage_against_the_reference_record(hiplib):
    """measured on an MI355X, worst over the record's 31 cases: rows 1.3e-7 of max |ce| (bound 1e-4), noise_estimate 5.2e-7 and snr
    5.5e-7 relative (bound 1e-5), cfo_hz 4.6e-5 Hz (bound 4e-3), no ta_us off"""
    from srslte_amd import capi

    lib = hiplib
    d = record()
    rng = np.random.default_rng(77)
    nc = len(d["cases"])
    keep, models, worst = [], [], np.zeros(4)
    for i in range(nc):
        grid, r, geometry, filt, meas_ta_en = case_grid(d, i, rng)
        nof_prb, cp_nsymb, n_prb, L_prb = geometry
        sm, m, _ = M.estimate(grid, r, nof_prb, cp_nsymb, (n_prb, n_prb), L_prb, filt, meas_ta_en)
        g = _geometry(capi, nof_prb, cp_nsymb, (n_prb, n_prb), L_prb)
        est = _est(capi, r, filt is not None, meas_ta_en)
        ce = np.full(grid.size, SENTINEL, np.complex64)
        out = capi.HipChestUlRes()
        assert lib.srsran_hip_chest_ul_estimate_pusch(C.byref(g), C.byref(est), O.P(grid), O.P(ce), C.byref(out)) == 0, capi.last_error()
        _check_against_record(d, i, ce, _six(out), geometry, filt, meas_ta_en, (sm, m), worst)
        # measurements only: the same six values, no grid
        only = capi.HipChestUlRes()
        assert lib.srsran_hip_chest_ul_estimate_pusch(C.byref(g), C.byref(est), O.P(grid), None, C.byref(only)) == 0
        assert np.array_equal(_six(only).view(np.uint32), _six(out).view(np.uint32)), i
        keep.append((grid, r, geometry, filt, meas_ta_en, g, est, _six(out), ce))
        models.append((sm, m))
    print("worst: rows %.3g of max|ce|, noise %.3g, snr %.3g relative, cfo %.3g Hz" % tuple(worst))
    # all cases in one call
    gs, es = (capi.HipPuschRx * nc)(*[k[5] for k in keep]), (capi.HipChestUl * nc)(*[k[6] for k in keep])
    ces = [np.full(k[0].size, SENTINEL, np.complex64) for k in keep]
    outs = (capi.HipChestUlRes * nc)()
    assert lib.srsran_hip_chest_ul_estimate_pusch_multi(nc, gs, es, (C.c_void_p * nc)(*[k[0].ctypes.data for k in keep]), (C.c_void_p * nc)(*[c.ctypes.data for c in ces]),
                                                        outs) == 0, capi.last_error()
    for i, k in enumerate(keep):
        _check_against_record(d, i, ces[i], _six(outs[i]), k[2], k[3], k[4], models[i], worst)
        assert np.array_equal(_six(outs[i]).view(np.uint32), k[7].view(np.uint32)) and np.array_equal(ces[i].view(np.uint32), k[8].view(np.uint32)), i


def test_stage_is_reproducible(hiplib):
    from srslte_amd import capi

    lib = hiplib
    rng = np.random.default_rng(5)
    nof_prb, cp_nsymb, n_prb, L_prb = 100, 7, (3, 40), 60  # 720 references per slot: every lane of four waves has several, hopping
    grid = (rng.standard_normal(14 * 1200) + 1j * rng.standard_normal(14 * 1200)).astype(np.complex64)
    r = np.exp(2j * np.pi * rng.random(2 * 12 * L_prb)).astype(np.complex64)
    g, est = _geometry(capi, nof_prb, cp_nsymb, n_prb, L_prb), _est(capi, r)
    got = []
    for _ in range(2):
        ce, out = np.zeros(grid.size, np.complex64), capi.HipChestUlRes()
        assert lib.srsran_hip_chest_ul_estimate_pusch(C.byref(g), C.byref(est), O.P(grid), O.P(ce), C.byref(out)) == 0, capi.last_error()
        got.append((ce, _six(out)))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    # a hopping grant: each slot where the UE sent it, as the model places it
    sm, m, want = M.estimate(grid, r, nof_prb, cp_nsymb, n_prb, L_prb, FILTER, 1)
    assert np.max(np.abs(got[0][0] - want)) <= 1e-4 * np.max(np.abs(sm)) and got[0][1][5] == m["ta_us"]
    assert not got[0][0][want == 0].any()


# ---- the grant calls -----------------------------------------------------------------------------------------------------------------------------------------

TWO_STEP_CASES = [
    # nof_prb, cp_nsymb, n_prb_tilde, L_prb, shortened, mod, tbs, snr_db, llr8: T.PUSCH_CASES' shapes on cells of at most 25 PRB
    (25, 7, (0, 0), 25, 0, 3, 12960, 29.0, False),  # three code blocks
    (25, 7, (2, 13), 10, 0, 3, 4584, 29.0, False),  # hopping between the slots
    (25, 7, (0, 0), 25, 1, 2, 6200, 17.0, False),  # SRS in the last symbol: 11 columns
    (6, 7, (1, 1), 4, 0, 1, 328, 8.0, False),  # one scalar-decoder block
    (25, 6, (3, 3), 20, 0, 2, 4584, 17.0, False),  # extended cyclic prefix: 10 columns
    (25, 7, (0, 0), 25, 0, 3, 12960, 29.0, True),  # 8-bit soft bits
    (15, 7, (2, 5), 9, 0, 1, 1544, 11.0, True),  # hopping, 8-bit
]


def _two_step(lib, capi, g, est, grid, Cn, dt, tbs):
    """(est call, two-step call): each (res, data, rows, flags, six)"""
    sb1 = _rx_softbuffer(capi, Cn, dt)
    d1, r1, e1 = np.zeros(tbs // 8 + 16, np.uint8), capi.HipGrantRes(), capi.HipChestUlRes()
    assert lib.srsran_hip_pusch_decode_est(C.byref(g), C.byref(est), None, O.P(grid), C.byref(sb1[0]), O.P(d1), C.byref(r1), None, C.byref(e1)) == 0, capi.last_error()
    ce, e2 = np.zeros(grid.size, np.complex64), capi.HipChestUlRes()
    assert lib.srsran_hip_chest_ul_estimate_pusch(C.byref(g), C.byref(est), O.P(grid), O.P(ce), C.byref(e2)) == 0, capi.last_error()
    g2 = capi.HipPuschRx.from_buffer_copy(g)
    g2.noise_estimate = e2.noise_estimate
    sb2 = _rx_softbuffer(capi, Cn, dt)
    d2, r2 = np.zeros(tbs // 8 + 16, np.uint8), capi.HipGrantRes()
    assert lib.srsran_hip_pusch_decode(C.byref(g2), O.P(grid), O.P(ce), C.byref(sb2[0]), O.P(d2), C.byref(r2)) == 0, capi.last_error()
    return (r1, d1, sb1[1], sb1[3], _six(e1)), (r2, d2, sb2[1], sb2[3], _six(e2))


def _same(a, b):
    (r1, d1, rows1, f1, s1), (r2, d2, rows2, f2, s2) = a, b
    assert r1.crc_ok == r2.crc_ok and np.float32(r1.avg_iterations_block).view(np.uint32) == np.float32(r2.avg_iterations_block).view(np.uint32)
    assert np.float32(r1.epre).view(np.uint32) == np.float32(r2.epre).view(np.uint32) and r1.epre > 0
    assert np.array_equal(d1, d2) and np.array_equal(f1, f2)
    for x, y in zip(rows1, rows2):
        assert np.array_equal(x, y)
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32))


@pytest.mark.parametrize("case", TWO_STEP_CASES, ids=lambda c: "prb%d_cp%d_L%d_mod%d_tbs%d%s%s" % (c[0], c[1], c[3], c[5], c[6], "_srs" if c[4] else "", "_8bit" if c[8] else ""))
def test_est_call_is_the_two_step_call(hiplib, case):
    from srslte_amd import capi

    lib = hiplib
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, snr_db, llr8 = case
    rng = np.random.default_rng(3000 + tbs + L_prb)
    nsymb = 2 * (cp_nsymb - 1) - (1 if shortened else 0)
    nof_re = nsymb * 12 * L_prb
    dt = np.int8 if llr8 else np.int16
    Cn = O.cbsegm(tbs)["C"]
    payload = rng.integers(0, 2, tbs).astype(np.uint8)
    grid, ce, seed = T._pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, 0x61, 7, 150, snr_db, payload)
    r = _with_dmrs(rng, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, snr_db)
    for filter_on in (True, False):
        est = _est(capi, r, filter_on)
        # (noise_estimate is not read by the est call: a value that would show)
        g = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 8, 1 if llr8 else 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened, 1e9, 1)
        a, b = _two_step(lib, capi, g, est, grid, Cn, dt, tbs)
        _same(a, b)
        assert a[4][0] > 0 if filter_on else a[4][0] == 0
    # a grant that cannot decode (random bits, one iteration): every row comes back, bit for bit the two-step call's
    Qm = O.QM[mod]
    q = rng.integers(0, 2, nof_re * Qm).astype(np.uint8)
    grid, ce, seed = T._pusch_grid(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, q, 0x61, 7, 150, snr_db)
    r = _with_dmrs(rng, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, snr_db)
    g = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 1, 1 if llr8 else 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened, 1e9, 1)
    a, b = _two_step(lib, capi, g, _est(capi, r), grid, Cn, dt, tbs)
    _same(a, b)
    assert a[0].crc_ok == 0 and not a[3].any() and all(row.any() for row in a[2][:Cn])


@pytest.mark.parametrize("case", [(6, 7, (0, 0), 6, 0, 1, 600, 12.0), (25, 7, (0, 0), 25, 0, 2, 6200, 20.0)], ids=["6prb_qpsk", "25prb_16qam"])
def test_est_grant_decodes(hiplib, case):
    from srslte_amd import capi

    lib = hiplib
    nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, snr_db = case
    rng = np.random.default_rng(4000 + tbs)
    nof_re = 12 * 12 * L_prb
    payload = rng.integers(0, 2, tbs).astype(np.uint8)
    grid, ce, seed = T._pusch_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, shortened, mod, tbs, 0, 0x62, 3, 77, snr_db, payload)
    r = _with_dmrs(rng, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, snr_db)
    est = _est(capi, r)
    g = capi.HipPuschRx(capi.HipGrantTb(mod, tbs, 0, nof_re, seed, 8, 0, 1), nof_prb, cp_nsymb, (C.c_uint32 * 2)(*n_prb), L_prb, shortened, 0.0, 0)
    sb = _rx_softbuffer(capi, O.cbsegm(tbs)["C"], np.int16)
    data, res, eo = np.zeros(tbs // 8 + 16, np.uint8), capi.HipGrantRes(), capi.HipChestUlRes()
    assert lib.srsran_hip_pusch_decode_est(C.byref(g), C.byref(est), None, O.P(grid), C.byref(sb[0]), O.P(data), C.byref(res), None, C.byref(eo)) == 0, capi.last_error()
    assert res.crc_ok == 1 and np.array_equal(np.unpackbits(data[:tbs // 8]), payload) and np.isnan(res.epre)
    # the measurements are those of the signal: the SNR within 2 dB of the channel's, the noise estimate within 2 dB of the noise that was added
    assert abs(eo.snr_db - snr_db) < 2.0 and abs(eo.noise_estimate_dbm - 30.0 + snr_db) < 2.0, (eo.snr_db, eo.noise_estimate_dbm)


def test_est_multi_with_and_without_uci(hiplib):
    """a TTI of four grants (1, 6, 6 and 25 PRB; one with ACK + CQI, one 8-bit) in one srsran_hip_pusch_decode_est_multi call = the four single calls"""
    from srslte_amd import capi

    lib = hiplib
    rng = np.random.default_rng(808)
    nof_prb, cp_nsymb = 50, 7
    ues = [  # n_prb, L_prb, mod, tbs, snr, llr8, (Q'ack, Q'ri, Q'cqi)
        ((0, 0), 1, 1, 104, 9.0, False, (0, 0, 0)), ((1, 1), 6, 1, 600, 12.0, False, (16, 0, 30)), ((7, 20), 6, 2, 1544, 18.0, True, (0, 0, 0)),
        ((25, 25), 25, 2, 6200, 20.0, False, (0, 0, 0)),
    ]
    n = len(ues)
    grants, ucis, ests = (capi.HipPuschRx * n)(), (capi.HipPuschUci * n)(), (capi.HipChestUl * n)()
    grids, rs, single = [], [], []
    for i, (n_prb, L_prb, mod, tbs, snr, llr8, (Qa, Qr, Qc)) in enumerate(ues):
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        grid, ce, seed = U._uci_signal(rng, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, 0x200 + i, 4, 33, snr, bits, Qa, Qr, Qc)
        rs.append(_with_dmrs(rng, grid, ce, nof_prb, cp_nsymb, n_prb, L_prb, snr))
        grants[i] = U._grant(capi, nof_prb, cp_nsymb, n_prb, L_prb, 0, mod, tbs, 0, seed, 8, 0.0, llr8=llr8, epre=1)
        ucis[i], ests[i] = capi.HipPuschUci(Qa, Qr, Qc), _est(capi, rs[i], filter_on=(i != 2), meas_ta_en=1 if i != 3 else 0)
        grids.append(grid)
        sb1 = _rx_softbuffer(capi, O.cbsegm(tbs)["C"], np.int8 if llr8 else np.int16)
        d1, r1, o1, e1 = np.zeros(tbs // 8 + 16, np.uint8), capi.HipGrantRes(), U._UciOut(capi, O.QM[mod], Qa, Qr, Qc), capi.HipChestUlRes()
        assert lib.srsran_hip_pusch_decode_est(C.byref(grants[i]), C.byref(ests[i]), C.byref(ucis[i]), O.P(grid), C.byref(sb1[0]), O.P(d1), C.byref(r1), C.byref(o1.c),
                                               C.byref(e1)) == 0, capi.last_error()
        single.append((r1, d1, sb1, o1, _six(e1)))
    sbs = [_rx_softbuffer(capi, O.cbsegm(u[3])["C"], np.int8 if u[5] else np.int16) for u in ues]
    datas = [np.zeros(u[3] // 8 + 16, np.uint8) for u in ues]
    outs = [U._UciOut(capi, O.QM[u[2]], *u[6]) for u in ues]
    oc = (capi.HipPuschUciOut * n)(*[o.c for o in outs])
    res, eos = (capi.HipGrantRes * n)(), (capi.HipChestUlRes * n)()
    assert lib.srsran_hip_pusch_decode_est_multi(n, grants, ests, ucis, (C.c_void_p * n)(*[a.ctypes.data for a in grids]),
                                                 (C.POINTER(capi.SoftbufferRx) * n)(*[C.pointer(s[0]) for s in sbs]), (C.c_void_p * n)(*[a.ctypes.data for a in datas]),
                                                 res, oc, eos) == 0, capi.last_error()
    for i in range(n):
        r1, d1, sb1, o1, s1 = single[i]
        assert res[i].crc_ok == r1.crc_ok == 1 and res[i].avg_iterations_block == r1.avg_iterations_block and res[i].epre == r1.epre, i
        assert np.array_equal(datas[i], d1) and np.array_equal(sbs[i][3], sb1[3]), i
        for a, b in zip(sbs[i][1], sb1[1]):
            assert np.array_equal(a, b), i
        for a, b in zip(outs[i].arrays(), o1.arrays()):
            assert np.array_equal(a, b), i
        assert outs[i].guards_intact() and np.array_equal(_six(eos[i]).view(np.uint32), s1.view(np.uint32)), i
    assert eos[2].noise_estimate == 0 and np.isnan(eos[2].snr) and eos[3].ta_us == 0 and eos[0].noise_estimate > 0
