"""PDSCH spatial multiplexing and large-delay CDD on 2 ports, 2 receive antennas (include/srsran_amd/phy_modem_abi.h: srsran_hip_predecoding_mimo,
srsran_hip_precoding_mimo; phy_chan_abi.h: srsran_hip_pdsch_decode_mimo{,_dbg}, srsran_hip_pdsch_encode_mimo{,_multi}).

Which test holds what to what:
  test_equaliser_against_the_float64_model   the equalisers to the closed-form float64 model of tests/spmux_model.py (pinned to the reference's record by
                                             test_spmux_golden.py), within c x 2^-24 x S, c from the float32 emulation of the operation order (spmux_model.C_BOUND)
  test_*_against_the_reference_record        equaliser and precoder to what the reference's own functions gave (tests/golden/spmux_ref.npz)
  test_codewords_in_one_call                 the fused call to the SAME stages one call at a time (srsran_hip_predecoding_mimo, then srsran_hip_pdsch_decode per
                                             codeword on the equalised symbols): soft bits and equalised symbols bit for bit, payload, verdict, iterations
  test_grant_that_cannot_decode              every soft-buffer row of both codewords over two transmissions
  test_transmit_*                            the fused transmit call to srsran_hip_pdsch_encode per codeword + srsran_hip_precoding_mimo, equal as numbers
  test_loop_back, test_worker_threads        transmit into receive; four threads at once
test_codewords_in_one_call and test_grant_that_cannot_decode take their expected soft bits and rows from the library's own srsran_hip_pdsch_decode_dbg, at sizes that
are multiples of 4: they hold the fused call to its per-stage twin.  What holds this path's soft bits to the ORACLE's demodulator, at sizes that leave its scalar tail
something to decide (n % 4, n % 8 != 0), is tests/test_gpu_pdsch_softbits.py.
The received planes of the codeword tests come from the oracle's transmit bits through the oracle's modulator, the float64 precoder of spmux_model.py, a
well-conditioned channel and noise 30 dB below the signal."""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest

import oracle_api as O
import spmux_model as M
from grant_helpers import SB, _lib, _matrix, _planes, _rx_softbuffer, _tx_softbuffer

pytestmark = pytest.mark.gpu
ITERS = 10
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUX, CDD = M.TXSCHEME_SPATIALMUX, M.TXSCHEME_CDD
CASE_IDS = ["cdd", "mux2_cb0", "mux2_cb1", "mux2_cb2", "mux1_cb0", "mux1_cb1", "mux1_cb2", "mux1_cb3"]
SENT = -7.0


def _predecode(lib, capi, y, h, scheme, layers, cb, dec, noise, scaling, want_csi=True):
    """the library's srsran_hip_predecoding_mimo on host planes: (x [layers][n], csi [2][n] pre-filled with SENT, or None)"""
    n = y.shape[1]
    x = np.full((2, n + 2), 7, np.complex64)
    csi = np.full((2, n + 4), SENT, np.float32)
    cp = (C.c_void_p * 2)(csi[0].ctypes.data if want_csi else None, csi[1].ctypes.data)
    rc = lib.srsran_hip_predecoding_mimo(_planes(capi, list(y)), _matrix(capi, h), _planes(capi, list(x)), cp, 2, 2, layers, cb, n, scheme, scaling, noise, dec)
    assert rc == 0, capi.last_error()
    assert np.all(x[:, n:] == 7) and np.all(x[layers:] == 7) and np.all(csi[:, n:] == SENT) and (want_csi or np.all(csi == SENT))
    return np.ascontiguousarray(x[:layers, :n]), (csi[:, :n].copy() if want_csi else None)


def _precode(lib, capi, x, scheme, layers, cb, scaling):
    n = x.shape[1]
    y = np.full((2, n + 2), 7, np.complex64)
    assert lib.srsran_hip_precoding_mimo(_planes(capi, list(x)), _planes(capi, list(y)), layers, 2, cb, n, scaling, scheme) == 0, capi.last_error()
    assert np.all(y[:, n:] == 7)
    return np.ascontiguousarray(y[:, :n])


def _check_csi(csi, wcsi, layers, tag):
    """rows the model gives: within 64 x 2^-24 relative (MMSE: the chain of the bound's constant; ZF: exactly 1); the others keep the sentinel"""
    for k in range(2):
        if k >= layers or np.isnan(wcsi[k]).all():
            assert np.all(csi[k] == SENT), tag
        else:
            assert np.all(np.abs(csi[k] - wcsi[k]) <= 64 * M.EPS * np.abs(wcsi[k])), tag


# ---- 1. the equalisers against the float64 model

@pytest.mark.parametrize("scheme,layers,cb", M.CASES, ids=CASE_IDS)
def test_equaliser_against_the_float64_model(hiplib, scheme, layers, cb):
    """Per component |x - x64| <= c x 2^-24 x S, S = norm x sum_j |G_kj| |y_j| (the magnitudes of the terms that form x_k), c = spmux_model.C_BOUND of the
    equaliser: five times the worst factor of the float32 emulation of the fixed operation order on these very shapes (test_spmux_golden.py).  nof_re: one
    pair, below one wave, around the 256 REs of a workgroup of the per-stage kernel, around a 2048-RE tile, two tiles and a bit; odd 301 without CDD."""
    lib, capi = _lib()
    rng = np.random.default_rng(100 * scheme + 10 * layers + cb)
    worst = 0.0
    for n in (2, 6, 254, 258, 2046, 2050, 4100, 301):
        if scheme == CDD and n % 2:
            continue
        y = np.ascontiguousarray(M.cn(rng, (2, n)).astype(np.complex64))
        h = M.channel(rng, n)
        for dec, noise in (M.DECODERS[:1] if layers == 1 else M.DECODERS):
            c = M.C_BOUND[M.kind_of(layers, dec)]
            for scaling in M.SCALINGS:
                want, wcsi, S = M.model64(y, h, scheme, layers, cb, dec, noise, scaling)
                x, csi = _predecode(lib, capi, y, h, scheme, layers, cb, dec, noise, scaling)
                f = M.worst_factor(x, want, S)
                worst = max(worst, f / c)
                assert f <= c, (n, dec, noise, scaling, f, c)
                _check_csi(csi, wcsi, layers, (n, dec, noise, scaling))
                x2, _ = _predecode(lib, capi, y, h, scheme, layers, cb, dec, noise, scaling, want_csi=False)  # the same formulas whether or not csi is asked for
                assert np.array_equal(x2.view(np.uint32), x.view(np.uint32)), (n, dec, noise, scaling)
    print("worst error: %.3f of the bound" % worst)


# ---- 2. against the reference's recorded results

def test_equaliser_against_the_reference_record(hiplib):
    """x: per-RE vector error within 2^-11 |x| (the reference's reciprocal estimate, test_spmux_golden.py) plus the bound of test 1; csi within 2^-10 relative;
    the row the reference's two-layer ZF multiplex body leaves untouched keeps its sentinel here too"""
    lib, capi = _lib()
    d = np.load(os.path.join(G, "spmux_ref.npz"))
    assert [tuple(c) for c in d["cases"]] == M.CASES
    y, h = np.ascontiguousarray(d["y"]), np.ascontiguousarray(d["h"])
    for scheme, layers, cb in M.CASES:
        for di, (dec, noise) in enumerate(M.DECODERS):
            if layers == 1 and di > 0:
                continue
            for si, scaling in enumerate(M.SCALINGS):
                tag = "rx_%d_%d_%d_d%d_s%d" % (scheme, layers, cb, di, si)
                rx, rcsi = d[tag + "_x"], d[tag + "_csi"]
                _, _, S = M.model64(y, h, scheme, layers, cb, dec, noise, scaling)
                x, csi = _predecode(lib, capi, y, h, scheme, layers, cb, dec, noise, scaling)
                err = np.sqrt((np.abs(x - rx) ** 2).sum(0))
                allow = 2.0 ** -11 * np.sqrt((np.abs(rx) ** 2).sum(0)) + M.C_BOUND[M.kind_of(layers, dec)] * M.EPS * np.sqrt(2 * (S ** 2).sum(0))
                assert np.all(err <= allow), (tag, float((err / allow).max()))
                for k in range(rcsi.shape[0]):
                    if np.all(rcsi[k] == d["csi_sentinel"]):
                        assert layers == 2 and dec == M.ZF and scheme == MUX and k == 1 and np.all(csi[k] == SENT), tag
                    else:
                        assert np.all(np.abs(csi[k] - rcsi[k]) <= 2.0 ** -10 * np.abs(rcsi[k])), (tag, k)


def test_precoder_against_the_reference_record(hiplib):
    """equal as numbers (-0 equals 0): every output is one float sum or difference times the same float factor"""
    lib, capi = _lib()
    d = np.load(os.path.join(G, "spmux_ref.npz"))
    xl = np.ascontiguousarray(d["layers"])
    for scheme, layers, cb in M.CASES:
        for si, scaling in enumerate(M.SCALINGS):
            want = d["tx_%d_%d_%d_s%d" % (scheme, layers, cb, si)]
            got = _precode(lib, capi, xl[:layers], scheme, layers, cb, float(scaling))
            assert np.array_equal(got, want), (scheme, layers, cb, si, int(np.count_nonzero(got != want)))


# ---- 3. the codewords of a grant in one call

#            scheme layers cb dec   noise  llr8  (mod, tbs) per codeword   nof_re  skip
CW_CASES = [(CDD, 2, 0, M.MMSE, 0.0, 0, ((1, 328), (1, 328)), 300, None),
            (MUX, 2, 1, M.ZF, 0.0, 0, ((2, 3624), (3, 5160)), 2100, None),
            (MUX, 2, 2, M.MMSE, 0.05, 0, ((3, 12960), (3, 12960)), 4200, None),
            (MUX, 2, 0, M.MMSE, 0.0, 1, ((1, 328), (1, 328)), 300, None),
            (MUX, 1, 3, M.ZF, 0.0, 0, ((2, 328),), 300, None),
            (CDD, 2, 0, M.ZF, 0.0, 0, ((1, 328), (1, 328)), 300, 1),
            (MUX, 2, 1, M.ZF, 0.0, 0, ((4, 328), (0, 40)), 300, None)]  # the widest and the narrowest soft-bit store of the front end: 32 and 4 bytes per pair
CW_IDS = ["cdd_qpsk_qpsk", "mux_cb1_16qam_64qam_2100", "mux_cb2_64qam_64qam_3cb_mmse", "mux_cb0_qpsk_8bit", "one_layer_cb3_16qam", "cdd_second_codeword_skipped",
          "mux_cb1_256qam_bpsk"]
SCALING = 0.8


def _seed(k):
    return O.pdsch_seed(0x1234, k, 10, 301)


def _per_stage(lib, capi, y, h, scheme, layers, cb, dec, noise, llr8, tbs_mod, rvs, sbs, scaling=SCALING):
    """srsran_hip_predecoding_mimo, then srsran_hip_pdsch_decode on each layer's equalised symbols (ce == NULL), one call at a time:
    (x, [(crc_ok, avg, data, e bits) per codeword])"""
    n = y.shape[1]
    x, _ = _predecode(lib, capi, y, h, scheme, layers, cb, dec, noise, scaling)
    out = []
    for k, (mod, tbs) in enumerate(tbs_mod):
        if sbs[k] is None:
            out.append(None)
            continue
        g = capi.HipPdschRx(capi.HipGrantTb(mod, tbs, rvs[k], n, _seed(k), ITERS, llr8, 1), 1.0, 0.0)
        data = np.zeros(tbs // 8 + 16, np.uint8)
        e = np.zeros(n * O.QM[mod], np.int8 if llr8 else np.int16)
        res = capi.HipGrantRes(7, 7.0, 7.0)
        assert lib.srsran_hip_pdsch_decode_dbg(C.byref(g), O.P(x[k]), None, C.byref(sbs[k]), O.P(data), C.byref(res), None, O.P(e)) == 0, capi.last_error()
        out.append((res.crc_ok, res.avg_iterations_block, data, e))
    return x, out


@functools.lru_cache(maxsize=None)
def _cw_case(scheme, layers, cb, dec, noise, llr8, tbs_mod, nof_re, skip):
    """the received planes of one case and what the stages, one call at a time, make of them (computed once, shared by the tests; read only)"""
    lib, capi = _lib()
    rng = np.random.default_rng(nof_re + 10 * scheme + cb + sum(t for _, t in tbs_mod))
    cws, pays = [], []
    for k, (mod, tbs) in enumerate(tbs_mod):
        nbits = nof_re * O.QM[mod]
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        e, _ = O.tb_coded_bits(tbs, O.QM[mod], nbits, 0, None, payload=bits, tx_order=True)
        assert e.size == nbits
        cws.append(O.modulate_bytes(mod, np.packbits(e), nbits, seed=_seed(k), scramble=True))
        pays.append(bits)
    p = M.precode64(np.stack(cws), scheme, layers, cb, SCALING)
    h = M.channel(rng, nof_re)
    sigma = 10 ** (-30 / 20) / np.sqrt(2)
    y = np.einsum("krn,kn->rn", h.astype(np.complex128), p) + sigma * (rng.standard_normal((2, nof_re)) + 1j * rng.standard_normal((2, nof_re)))
    y = np.ascontiguousarray(y.astype(np.complex64))
    dt = np.int8 if llr8 else np.int16
    keep = [_rx_softbuffer(capi, O.cbsegm(tbs)["C"], dt) for _, tbs in tbs_mod]
    x, stages = _per_stage(lib, capi, y, h, scheme, layers, cb, dec, noise, llr8, tbs_mod, [0] * len(tbs_mod), [None if k == skip else keep[k][0] for k in range(len(tbs_mod))])
    for a in (y, h, x):
        a.setflags(write=False)
    return dict(y=y, h=h, x=x, stages=stages, pays=pays)


def _decode_one(lib, capi, case, scheme, layers, cb, dec, noise, llr8, tbs_mod, nof_re, skip, dbg):
    """the grant in one call: [(crc_ok, avg, data, d_out, e_out) per codeword, None for a skipped one]"""
    dt = np.int8 if llr8 else np.int16
    ntb = len(tbs_mod)
    tbs_ = [capi.HipGrantTb(mod, tbs, 0, nof_re, _seed(k), ITERS, llr8, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
    g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), ntb, layers, scheme, cb, dec, 2, SCALING, noise)
    sbs = [_rx_softbuffer(capi, O.cbsegm(tbs)["C"], dt) for _, tbs in tbs_mod]
    sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[None if k == skip else C.pointer(sbs[k][0]) for k in range(ntb)])
    data = [np.full(tbs // 8 + 16, 0xA5, np.uint8) for _, tbs in tbs_mod]
    dp = (C.c_void_p * 2)(*[a.ctypes.data for a in data])
    res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
    sym, ce = _planes(capi, list(case["y"])), _matrix(capi, case["h"])
    d_out = [np.full(nof_re + 4, 7, np.complex64) for _ in tbs_mod]
    e_out = [np.full(nof_re * O.QM[mod] + 8, 7, dt) for mod, _ in tbs_mod]
    if dbg:
        ep = (C.c_void_p * 2)(*[None if k == skip else e_out[k].ctypes.data for k in range(ntb)])
        rc = lib.srsran_hip_pdsch_decode_mimo_dbg(C.byref(g), sym, ce, sbp, dp, res, (C.c_void_p * 2)(*[a.ctypes.data for a in d_out]), ep)
    else:
        rc = lib.srsran_hip_pdsch_decode_mimo(C.byref(g), sym, ce, sbp, dp, res)
    assert rc == 0, capi.last_error()
    out = []
    for k in range(ntb):
        if k == skip:  # res = {0, 0, NAN}, the payload untouched
            assert res[k].crc_ok == 0 and res[k].avg_iterations_block == 0.0 and np.isnan(res[k].epre) and np.all(data[k] == 0xA5) and np.all(e_out[k] == 7)
            out.append((None, None, None, d_out[k] if dbg else None, None))
        else:
            out.append((res[k].crc_ok, res[k].avg_iterations_block, data[k], d_out[k] if dbg else None, e_out[k] if dbg else None))
    if ntb == 1:
        assert res[1].crc_ok == 0 and res[1].avg_iterations_block == 0.0 and np.isnan(res[1].epre)
    return out


@pytest.mark.parametrize("scheme,layers,cb,dec,noise,llr8,tbs_mod,nof_re,skip", CW_CASES, ids=CW_IDS)
def test_codewords_in_one_call(hiplib, scheme, layers, cb, dec, noise, llr8, tbs_mod, nof_re, skip):
    lib, capi = _lib()
    args = (scheme, layers, cb, dec, noise, llr8, tbs_mod, nof_re, skip)
    case = _cw_case(*args)
    plain = _decode_one(lib, capi, case, *args, False)
    dbg = _decode_one(lib, capi, case, *args, True)
    for k, (mod, tbs) in enumerate(tbs_mod):
        nbits = nof_re * O.QM[mod]
        # the equalised symbols of every layer, the skipped codeword's included: the per-stage kernel's, bit for bit
        d_out = dbg[k][3]
        assert np.array_equal(d_out[:nof_re].view(np.uint32), case["x"][k].view(np.uint32)) and np.all(d_out[nof_re:] == 7), k
        if k == skip:
            continue
        ok_s, avg_s, data_s, e_s = case["stages"][k]
        assert ok_s == 1  # the expected chain itself decodes: the test is only valid on such inputs
        ok, avg, data, _, _ = plain[k]
        print("codeword %d: crc_ok %d avg_iterations_block %g (per stage: %g)" % (k, ok, avg, avg_s))
        assert ok == 1 and avg == avg_s
        assert np.array_equal(data[:tbs // 8], data_s[:tbs // 8]) and np.array_equal(np.unpackbits(data[:tbs // 8]), case["pays"][k])
        ok2, avg2, data2, _, e_out = dbg[k]
        assert ok2 == 1 and avg2 == avg and np.array_equal(data2[:tbs // 8], data[:tbs // 8])
        assert np.array_equal(e_out[:nbits], e_s) and np.all(e_out[nbits:] == 7), k


# ---- 4. a grant that cannot decode

def test_grant_that_cannot_decode(hiplib):
    """random symbols (16-QAM with two code blocks + QPSK, codebook 1, MMSE): crc_ok == 0 for both codewords and every soft-buffer row of both is what the
    per-stage chain leaves; a second transmission (rv 1) into the same soft buffers combines as the per-stage chain does"""
    lib, capi = _lib()
    tbs_mod, nof_re = ((2, 6200), (1, 2792)), 2400
    rng = np.random.default_rng(77)
    nb = [O.cbsegm(tbs)["C"] for _, tbs in tbs_mod]
    one = [_rx_softbuffer(capi, nb[k] + 1, np.int16) for k in range(2)]
    ref = [_rx_softbuffer(capi, nb[k] + 1, np.int16) for k in range(2)]
    for rv in (0, 1):
        y = np.ascontiguousarray((rng.standard_normal((2, nof_re)) + 1j * rng.standard_normal((2, nof_re))).astype(np.complex64))
        h = M.channel(rng, nof_re)
        tbs_ = [capi.HipGrantTb(mod, tbs, rv, nof_re, _seed(k), ITERS, 0, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), 2, 2, MUX, 1, M.MMSE, 2, SCALING, 0.05)
        data = [np.full(tbs // 8 + 16, 0xA5, np.uint8) for _, tbs in tbs_mod]
        res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(C.pointer(one[0][0]), C.pointer(one[1][0]))
        assert lib.srsran_hip_pdsch_decode_mimo(C.byref(g), _planes(capi, list(y)), _matrix(capi, h), sbp, (C.c_void_p * 2)(*[a.ctypes.data for a in data]), res) == 0, \
            capi.last_error()
        _, stages = _per_stage(lib, capi, y, h, MUX, 2, 1, M.MMSE, 0.05, 0, tbs_mod, [rv, rv], [ref[0][0], ref[1][0]])
        for k, (mod, tbs) in enumerate(tbs_mod):
            assert stages[k][0] == 0 and not ref[k][3].any(), (rv, k)  # the precondition: every row comes back
            assert res[k].crc_ok == 0 and not one[k][0].tb_crc and not one[k][3].any(), (rv, k)
            assert res[k].avg_iterations_block == stages[k][1], (rv, k)
            for i in range(nb[k] + 1):
                assert np.array_equal(one[k][1][i], ref[k][1][i]), (rv, k, i)
            assert any(r.any() for r in one[k][1][:nb[k]]) and not one[k][1][nb[k]].any(), (rv, k)
            assert np.all(data[k][tbs // 8 + 6:] == 0xA5), (rv, k)


# ---- 5. transmit in one call

def _per_stage_tx(lib, capi, sbs, pays, tbs_mod, rv, nof_re, scheme, layers, cb, scaling):
    """srsran_hip_pdsch_encode per codeword (unscaled) -> srsran_hip_precoding_mimo, one call at a time: [2][nof_re]"""
    x = np.zeros((layers, nof_re), np.complex64)
    for k, (mod, tbs) in enumerate(tbs_mod):
        g = capi.HipPdschTx(capi.HipGrantTb(mod, tbs, rv, nof_re, _seed(k), 0, 0, 1), 1.0)
        assert lib.srsran_hip_pdsch_encode(C.byref(g), C.byref(sbs[k]), O.P(pays[k]) if pays[k] is not None else None, O.P(x[k])) == 0, capi.last_error()
    return _precode(lib, capi, x, scheme, layers, cb, scaling)


def _tx_grant(capi, tbs_mod, rv, nof_re, scheme, layers, cb, scaling):
    tbs_ = [capi.HipGrantTb(mod, tbs, rv, nof_re, _seed(k), 0, 0, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
    return capi.HipPdschMimoTx((capi.HipGrantTb * 2)(*tbs_), len(tbs_mod), layers, scheme, cb, scaling)


TX_SCALINGS = [1.0, float(np.float32(np.sqrt(2) * 0.7))]
TX_CASES = [(s, 2, c, n) for (s, c) in ((CDD, 0), (MUX, 0), (MUX, 1), (MUX, 2)) for n in (300, 2100)] + [(MUX, 2, 1, 301)] + [(MUX, 1, c, 300) for c in range(4)] + \
    [(MUX, 1, 2, 2051)]


@pytest.mark.parametrize("scheme,layers,cb,nof_re", TX_CASES, ids=["%s%d_cb%d_%d" % ("cdd" if s == CDD else "mux", l, c, n) for s, l, c, n in TX_CASES])
def test_transmit_in_one_call(hiplib, scheme, layers, cb, nof_re):
    """both port planes equal as numbers to the per-stage path's (16-QAM + 64-QAM, or 16-QAM alone), the sentinels behind each plane intact; then a
    retransmission (data == NULL, rv 2) from the same soft buffers"""
    lib, capi = _lib()
    tbs_mod = ((2, 328), (3, 328))[:layers] if nof_re < 2000 else ((2, 3624), (3, 5160))[:layers]
    rng = np.random.default_rng(nof_re + 10 * scheme + cb)
    pays = [rng.integers(0, 256, tbs // 8).astype(np.uint8) for _, tbs in tbs_mod]
    for scaling in TX_SCALINGS:
        sbs = [_tx_softbuffer(capi, 1) for _ in tbs_mod]
        sbs_ref = [_tx_softbuffer(capi, 1) for _ in tbs_mod]
        for rv, pay in ((0, pays), (2, [None] * layers)):
            g = _tx_grant(capi, tbs_mod, rv, nof_re, scheme, layers, cb, scaling)
            out = np.full((2, nof_re + 8), 7, np.complex64)
            sbp = (C.POINTER(capi.SoftbufferTx) * 2)(*[C.pointer(s[0]) for s in sbs])
            dp = (C.c_void_p * 2)(*[p.ctypes.data if p is not None else None for p in pay])
            assert lib.srsran_hip_pdsch_encode_mimo(C.byref(g), sbp, dp, _planes(capi, list(out))) == 0, capi.last_error()
            want = _per_stage_tx(lib, capi, [s[0] for s in sbs_ref], pay, tbs_mod, rv, nof_re, scheme, layers, cb, scaling)
            assert np.array_equal(out[:, :nof_re], want), (scaling, rv, int(np.count_nonzero(out[:, :nof_re] != want)))
            assert np.all(out[:, nof_re:] == 7) and np.abs(want).max() > 0.1, (scaling, rv)


def test_transmit_grants_of_a_tti_in_one_call(hiplib):
    """srsran_hip_pdsch_encode_mimo_multi: three grants of different schemes, codeword counts, modulations and sizes (the second ends a workgroup exactly, so a
    wrong first workgroup of the third would show) = the three single calls, sentinels behind every plane included"""
    lib, capi = _lib()
    rng = np.random.default_rng(31)
    ues = [(CDD, 2, 0, ((3, 5160), (1, 328)), 2100, 1.0), (MUX, 1, 2, ((2, 3624),), 2048, TX_SCALINGS[1]), (MUX, 2, 2, ((1, 328), (2, 328)), 301, 0.5)]
    n = len(ues)
    grants = (capi.HipPdschMimoTx * n)()
    singles, outs, keep = [], [], []
    sbpp, dpp = ((C.POINTER(capi.SoftbufferTx) * 2) * n)(), ((C.c_void_p * 2) * n)()
    for i, (scheme, layers, cb, tbs_mod, nof_re, scaling) in enumerate(ues):
        grants[i] = _tx_grant(capi, tbs_mod, 0, nof_re, scheme, layers, cb, scaling)
        pays = [rng.integers(0, 256, tbs // 8).astype(np.uint8) for _, tbs in tbs_mod]
        sb1 = [_tx_softbuffer(capi, 1) for _ in tbs_mod]
        one = np.full((2, nof_re + 8), 7, np.complex64)
        assert lib.srsran_hip_pdsch_encode_mimo(C.byref(grants[i]), (C.POINTER(capi.SoftbufferTx) * 2)(*[C.pointer(s[0]) for s in sb1]),
                                                (C.c_void_p * 2)(*[p.ctypes.data for p in pays]), _planes(capi, list(one))) == 0, capi.last_error()
        singles.append(one)
        sbm = [_tx_softbuffer(capi, 1) for _ in tbs_mod]
        for k in range(layers):
            sbpp[i][k] = C.pointer(sbm[k][0])
            dpp[i][k] = pays[k].ctypes.data
        keep.append((pays, sb1, sbm))
        outs.append(np.full((2, nof_re + 8), 7, np.complex64))
    planes = [_planes(capi, list(o)) for o in outs]
    assert lib.srsran_hip_pdsch_encode_mimo_multi(n, grants, sbpp, dpp, (C.POINTER(C.c_void_p) * n)(*[C.cast(p, C.POINTER(C.c_void_p)) for p in planes])) == 0, \
        capi.last_error()
    for i, ue in enumerate(ues):
        assert np.array_equal(outs[i].view(np.uint32), singles[i].view(np.uint32)), i
        assert np.all(outs[i][:, ue[4]:] == 7) and np.abs(outs[i][:, :ue[4]]).max() > 0.1, i


# ---- 6. loop back

@pytest.mark.parametrize("scheme,cb", [(CDD, 0), (MUX, 1)], ids=["cdd", "mux_cb1"])
def test_loop_back(hiplib, scheme, cb):
    """encode in one call, a known 2x2 channel without noise, decode in one call (ZF): both payloads return after one half iteration per block (the minimum)"""
    lib, capi = _lib()
    tbs_mod, nof_re = ((2, 6200), (3, 5160)), 2400
    rng = np.random.default_rng(scheme + cb)
    pays = [rng.integers(0, 256, tbs // 8).astype(np.uint8) for _, tbs in tbs_mod]
    nb = [O.cbsegm(tbs)["C"] for _, tbs in tbs_mod]
    sbt = [_tx_softbuffer(capi, nb[k]) for k in range(2)]
    scaling = TX_SCALINGS[1]
    gt = _tx_grant(capi, tbs_mod, 0, nof_re, scheme, 2, cb, scaling)
    p = np.zeros((2, nof_re), np.complex64)
    assert lib.srsran_hip_pdsch_encode_mimo(C.byref(gt), (C.POINTER(capi.SoftbufferTx) * 2)(*[C.pointer(s[0]) for s in sbt]),
                                            (C.c_void_p * 2)(*[a.ctypes.data for a in pays]), _planes(capi, list(p))) == 0, capi.last_error()
    h = M.channel(rng, nof_re)
    y = np.ascontiguousarray(np.einsum("krn,kn->rn", h.astype(np.complex128), p.astype(np.complex128)).astype(np.complex64))
    tbs_ = [capi.HipGrantTb(mod, tbs, 0, nof_re, _seed(k), ITERS, 0, 1) for k, (mod, tbs) in enumerate(tbs_mod)]
    gr = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), 2, 2, scheme, cb, M.ZF, 2, scaling, 0.0)
    sbr = [_rx_softbuffer(capi, nb[k], np.int16) for k in range(2)]
    data = [np.zeros(tbs // 8 + 16, np.uint8) for _, tbs in tbs_mod]
    res = (capi.HipGrantRes * 2)()
    assert lib.srsran_hip_pdsch_decode_mimo(C.byref(gr), _planes(capi, list(y)), _matrix(capi, h), (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbr]),
                                            (C.c_void_p * 2)(*[a.ctypes.data for a in data]), res) == 0, capi.last_error()
    for k, (_, tbs) in enumerate(tbs_mod):
        assert res[k].crc_ok == 1 and np.array_equal(data[k][:tbs // 8], pays[k]), k
        assert res[k].avg_iterations_block == 1.0, k


# ---- 7. worker threads

def test_worker_threads(hiplib):
    """four threads at once, each decoding its own case of test 3 twice: what the single-threaded call gives (one worker per subframe in flight is the
    reference's threading model; staging contexts are per thread)"""
    lib, capi = _lib()
    cases = CW_CASES[:4]
    want = [_decode_one(lib, capi, _cw_case(*c), *c, True) for c in cases]
    errors = []

    def worker(i):
        try:
            case = _cw_case(*cases[i])
            for _ in range(2):
                got = _decode_one(lib, capi, case, *cases[i], True)
                for a, b in zip(got, want[i]):
                    assert a[0] == b[0] == 1 and a[1] == b[1]
                    for u, v in zip(a[2:], b[2:]):
                        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(cases))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
