#!/usr/bin/env python3
"""Record what the reference's spatial-multiplexing and CDD stages give on seeded inputs: tests/golden/spmux_ref.npz (needs oracle/_ref/libsrsran_ref.so, built
by `make -C oracle ref`; mimo/precoding.c and utils/mat.c are part of it).

    python tools/gen_golden_spmux.py

Receive: srsran_predecoding_set_mimo_decoder + srsran_predecoding_type WITH csi (the _csi variants, the ones srsran_pdsch_decode runs) on 2 ports and 2 receive
antennas for every (scheme, layers, codebook_idx) the library takes -- CDD; spatial multiplexing with 2 layers, codebook 0 .. 2; with 1 layer, codebook 0 .. 3 --
with ZF, MMSE at noise 0 and MMSE at noise 0.05 (one layer: the decoder plays no part, recorded once), at scaling 1.0 and 0.7.  n = 516 REs: the AVX2 body
(8 per step) covers 512 of them and the scalar tail the last 4, so both are on record.  y ~ CN(0,1); the channel is well conditioned by construction:
h[p][r] = (p == r ? 1 : 0.3 e^{j theta}) + 0.1 CN(0,1), theta uniform (the all-0.9 taps of the transmit-diversity fixture are nearly singular for a 2x2
inverse).  The csi rows are pre-filled with CSI_SENTINEL: the two-layer ZF multiplex body writes row 0 only (precoding.c:1292-1293, :1330-1331).
Transmit: srsran_precoding_type on layers of random complex points (no constellation), the same cases and scalings.
Every plane is 64-byte aligned: the reference's vector bodies use aligned loads and stores (an unaligned csi row faults).
tests/test_spmux_golden.py holds a float64 model to these; tests/test_gpu_spmux.py the library's kernels.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_api as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spmux_ref.npz")
MAX_PORTS = 4
Planes = C.c_void_p * MAX_PORTS
Matrix = Planes * MAX_PORTS
TXSCHEME_SPATIALMUX, TXSCHEME_CDD = 2, 3
DECODER_ZF, DECODER_MMSE = 0, 1

N = 516
CASES = [(TXSCHEME_CDD, 2, 0), (TXSCHEME_SPATIALMUX, 2, 0), (TXSCHEME_SPATIALMUX, 2, 1), (TXSCHEME_SPATIALMUX, 2, 2),
         (TXSCHEME_SPATIALMUX, 1, 0), (TXSCHEME_SPATIALMUX, 1, 1), (TXSCHEME_SPATIALMUX, 1, 2), (TXSCHEME_SPATIALMUX, 1, 3)]
DECODERS = [(DECODER_ZF, 0.0), (DECODER_MMSE, 0.0), (DECODER_MMSE, 0.05)]
SCALINGS = [1.0, 0.7]
CSI_SENTINEL = -7.0


def cn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def aligned(shape, dtype, fill=0):
    """an array of `shape` whose every row (last axis) starts on a 64-byte boundary"""
    rows = int(np.prod(shape[:-1]))
    item = np.dtype(dtype).itemsize
    stride = -(-shape[-1] * item // 64) * 64
    raw = np.zeros(rows * stride + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    view = np.ndarray(shape=(rows, shape[-1]), dtype=dtype, buffer=raw.data, offset=off, strides=(stride, item))
    view[...] = fill
    return view, raw


def main():
    ref = C.CDLL(O.REF_LIB)
    ref.srsran_predecoding_set_mimo_decoder.argtypes = [C.c_int]
    ref.srsran_predecoding_set_mimo_decoder.restype = None
    ref.srsran_predecoding_type.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Planes), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_float, C.c_float]
    ref.srsran_precoding_type.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
    rng = np.random.default_rng(1)
    theta = rng.uniform(0, 2 * np.pi, (2, 2, N))
    base = np.where(np.eye(2, dtype=bool)[:, :, None], 1.0, 0.3 * np.exp(1j * theta))
    h_in = (base + 0.1 * cn(rng, (2, 2, N))).astype(np.complex64)  # [port][rx][n]
    y_in = cn(rng, (2, N)).astype(np.complex64)
    xl_in = cn(rng, (2, N)).astype(np.complex64)  # transmit: the two layers
    hv, hraw = aligned((4, N), np.complex64)
    yv, yraw = aligned((2, N), np.complex64)
    lv, lraw = aligned((2, N), np.complex64)
    hv[...] = h_in.reshape(4, N)
    yv[...] = y_in
    lv[...] = xl_in
    d = {"cases": np.array(CASES, np.int32), "decoders": np.array(DECODERS, np.float32), "scalings": np.array(SCALINGS, np.float32),
         "csi_sentinel": np.float32(CSI_SENTINEL), "h": h_in, "y": y_in, "layers": xl_in}
    yp = Planes(yv[0].ctypes.data, yv[1].ctypes.data)
    hp = Matrix(Planes(hv[0].ctypes.data, hv[1].ctypes.data), Planes(hv[2].ctypes.data, hv[3].ctypes.data))
    worst_cn = 0.0
    for scheme, layers, cb in CASES:
        for di, (dec, noise) in enumerate(DECODERS):
            if layers == 1 and di > 0:
                continue
            for si, scaling in enumerate(SCALINGS):
                xv, xraw = aligned((2, N), np.complex64)
                cv, craw = aligned((2, N), np.float32, CSI_SENTINEL)
                xp = Planes(xv[0].ctypes.data, xv[1].ctypes.data)
                cp = (C.c_void_p * 2)(cv[0].ctypes.data, cv[1].ctypes.data)
                ref.srsran_predecoding_set_mimo_decoder(dec)
                assert ref.srsran_predecoding_type(yp, hp, xp, cp, 2, 2, layers, cb, N, scheme, scaling, noise) == 0
                tag = "rx_%d_%d_%d_d%d_s%d" % (scheme, layers, cb, di, si)
                d[tag + "_x"] = np.array(xv[:layers])
                d[tag + "_csi"] = np.array(cv[:layers] if layers == 1 else cv)
        for si, scaling in enumerate(SCALINGS):
            pv, praw = aligned((2, N), np.complex64)
            pv[...] = np.nan
            lp = Planes(lv[0].ctypes.data, lv[1].ctypes.data)
            pp = Planes(pv[0].ctypes.data, pv[1].ctypes.data)
            assert ref.srsran_precoding_type(lp, pp, layers, 2, cb, N, scaling, scheme) >= 0
            assert not np.isnan(pv).any()
            d["tx_%d_%d_%d_s%d" % (scheme, layers, cb, si)] = np.array(pv)
    ref.srsran_predecoding_set_mimo_decoder(DECODER_MMSE)  # the library's initial value
    # the condition number of every effective channel on record (for the docstring of the test that uses the bound)
    a, b = h_in[0].astype(np.complex128), h_in[1].astype(np.complex128)  # [rx][n] of port 0 / 1
    for cols in ((a, b), (a + b, a - b), (a + 1j * b, a - 1j * b)):
        m = np.stack([np.stack([cols[0][0], cols[1][0]], -1), np.stack([cols[0][1], cols[1][1]], -1)], -2)  # [n][rx][layer]
        worst_cn = max(worst_cn, float(np.linalg.cond(m).max()))
    print("worst condition number of an effective channel: %.2f" % worst_cn)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
