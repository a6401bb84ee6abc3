"""The frame the three PDSCH receive grant paths share (csrc/chan_internal.h: pdsch_decode_grant), through srsran_hip_pdsch_decode_csi_dbg (one port, with estimates),
srsran_hip_pdsch_decode_txdiv_csi_dbg (2 ports, 1 receive antenna) and srsran_hip_pdsch_decode_mimo_csi_dbg (spatial multiplexing, 2 layers, codebook 1, ZF).

  test_output_asked_for_and_not_produced_is_an_error   a codeword of two code blocks on a soft buffer of one row: the transport-block stage drops it in front of the
                                                       front end, so its d / e / csi never exist: SRSRAN_ERROR, the buffers untouched, res filled
  test_outputs_end_where_they_should                   the same calls on a buffer that fits: every output written over its whole length and not one entry further
The bit-exact comparisons of what the outputs hold are in test_gpu_chan.py, test_gpu_txdiv.py, test_gpu_spmux.py and test_gpu_pdsch_csi.py.

Grant: 16-QAM, tbs 6200 (two code blocks), 1800 REs, random symbols and estimates, int16 soft bits, one iteration; the MIMO call's codeword 1 is QPSK, tbs 2792 (one block).
Sentinels are values no output can hold: a CSI value is >= 0, an int16 soft bit of a unit-power symbol is orders of magnitude inside the type's range."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as O
import spmux_model as M
from grant_helpers import _lib, _matrix, _planes, _rx_softbuffer

pytestmark = pytest.mark.gpu
PATHS = ["single", "txdiv", "mimo"]
NOF_RE, SCALING, PAD = 1800, 0.8, 16
CW = [(2, 6200), (1, 2792)]  # (mod, tbs) of codeword 0 (every path) and codeword 1 (MIMO)
D_SENT, E_SENT, C_SENT = np.complex64(-7 - 7j), np.int16(-32768), np.float32(-7.0)
SRSRAN_ERROR = -1


@functools.lru_cache(maxsize=None)
def _call(path, rows0):
    """the path's _csi_dbg call with `rows0` rows in codeword 0's soft buffer (run once per case, shared, read only)"""
    lib, capi = _lib()
    rng = np.random.default_rng(PATHS.index(path))
    tbm = CW if path == "mimo" else CW[:1]
    ports, nrx = {"single": (1, 1), "txdiv": (2, 1), "mimo": (2, 2)}[path]
    y = np.ascontiguousarray(M.cn(rng, (nrx, NOF_RE)).astype(np.complex64))
    h = M.channel(rng, NOF_RE) if path == "mimo" else np.ascontiguousarray(np.repeat(0.9 + 0.1 * M.cn(rng, (ports, nrx, NOF_RE // 2)), 2, axis=2).astype(np.complex64))
    sbs = [_rx_softbuffer(capi, rows0 if k == 0 else O.cbsegm(tbs)["C"], np.int16) for k, (_, tbs) in enumerate(tbm)]
    data = [np.zeros(tbs // 8 + 16, np.uint8) for _, tbs in tbm]
    d_out = [np.full(NOF_RE + PAD, D_SENT, np.complex64) for _ in tbm]
    e_out = [np.full(NOF_RE * O.QM[mod] + PAD, E_SENT, np.int16) for mod, _ in tbm]
    c_out = [np.full(NOF_RE + PAD, C_SENT, np.float32) for _ in tbm]
    tbs_ = [capi.HipGrantTb(mod, tbs, 0, NOF_RE, O.pdsch_seed(0x1234, k, 10, 301), 1, 0, 2 if path == "txdiv" else 1) for k, (mod, tbs) in enumerate(tbm)]
    res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
    if path == "single":
        rc = lib.srsran_hip_pdsch_decode_csi_dbg(C.byref(capi.HipPdschRx(tbs_[0], SCALING, 0.0)), O.P(y[0]), O.P(h[0][0]), None, C.byref(sbs[0][0]), O.P(data[0]), res,
                                                 O.P(d_out[0]), O.P(e_out[0]), O.P(c_out[0]))
    elif path == "txdiv":
        rc = lib.srsran_hip_pdsch_decode_txdiv_csi_dbg(C.byref(capi.HipPdschTxdivRx(tbs_[0], ports, nrx, SCALING, 0)), _planes(capi, list(y)), _matrix(capi, h),
                                                       C.byref(sbs[0][0]), O.P(data[0]), res, O.P(d_out[0]), O.P(e_out[0]), O.P(c_out[0]))
    else:
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), 2, 2, capi.TXSCHEME_SPATIALMUX, 1, capi.MIMO_DECODER_ZF, 2, SCALING, 0.0)
        ptrs = [(C.c_void_p * 2)(*[a.ctypes.data for a in arrs]) for arrs in (data, d_out, e_out, c_out)]
        rc = lib.srsran_hip_pdsch_decode_mimo_csi_dbg(C.byref(g), _planes(capi, list(y)), _matrix(capi, h), (C.POINTER(capi.SoftbufferRx) * 2)(*[C.pointer(s[0]) for s in sbs]),
                                                      ptrs[0], res, ptrs[1], ptrs[2], ptrs[3])
    return dict(rc=rc, err=capi.last_error(), crc_ok=[res[k].crc_ok for k in range(len(tbm))], sbs=sbs, d=d_out, e=e_out, c=c_out,
                nbits=[NOF_RE * O.QM[mod] for mod, _ in tbm])


@pytest.mark.parametrize("path", PATHS)
def test_output_asked_for_and_not_produced_is_an_error(hiplib, path):
    r = _call(path, 1)
    print("%s: rc %d, last error: %s" % (path, r["rc"], r["err"]))
    assert r["rc"] == SRSRAN_ERROR
    assert "intermediate result" in r["err"] and "not produced" in r["err"]
    sb, rows, _, flags = r["sbs"][0]
    assert r["crc_ok"][0] == 0 and not sb.tb_crc
    assert not rows[0].any() and not flags.any()
    assert np.all(r["e"][0] == E_SENT) and np.all(r["c"][0] == C_SENT)
    if path != "mimo":
        assert np.all(r["d"][0] == D_SENT)
    else:  # codeword 1 went through the front end by itself: its outputs are those of the call in which both did
        full, n1 = _call(path, 2), r["nbits"][1]
        assert full["rc"] == 0, full["err"]
        assert np.array_equal(r["e"][1][:n1], full["e"][1][:n1]) and np.all(r["e"][1][n1:] == E_SENT)
        assert np.array_equal(r["c"][1][:NOF_RE].view(np.uint32), full["c"][1][:NOF_RE].view(np.uint32)) and np.all(r["c"][1][NOF_RE:] == C_SENT)


@pytest.mark.parametrize("path", PATHS)
def test_outputs_end_where_they_should(hiplib, path):
    r = _call(path, 2)
    assert r["rc"] == 0, r["err"]
    for k, nbits in enumerate(r["nbits"]):
        for name, out, n, sent in (("d", r["d"][k], NOF_RE, D_SENT), ("e", r["e"][k], nbits, E_SENT), ("csi", r["c"][k], NOF_RE, C_SENT)):
            assert not np.any(out[:n] == sent), (k, name, int(np.count_nonzero(out[:n] == sent)))
            assert np.all(out[n:] == sent), (k, name)
