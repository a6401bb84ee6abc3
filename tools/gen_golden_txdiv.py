#!/usr/bin/env python3
"""Record what the reference's transmit-diversity stages give on seeded inputs: tests/golden/txdiv_ref.npz (needs oracle/_ref/libsrsran_ref.so, built by
`make -C oracle ref`; mimo/precoding.c is part of it).

    python tools/gen_golden_txdiv.py

Receive: srsran_predecoding_diversity_multi WITH csi (the _csi variant, precoding.c:673-778, the one srsran_pdsch_decode runs) for
(ports, rx, nof_re) = (2,1,72), (2,2,516), (4,1,72), (4,2,516) at scaling 1.0 and 0.7; y ~ CN(0,1), channel taps 0.9 + 0.1 (randn + j randn) per plane.
Transmit: srsran_precoding_diversity (precoding.c:1943-1992) on codewords of random complex points (no constellation) split into layers as
srsran_layermap_diversity does: 2 ports on 258 and 516 points, 4 ports on 516, at scaling 1.0 and 0.7.
tests/test_gpu_txdiv.py holds the library's entry points of the same names to these.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_api as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "txdiv_ref.npz")
MAX_PORTS = 4
Planes = C.c_void_p * MAX_PORTS
Matrix = Planes * MAX_PORTS

RX_CASES = [(2, 1, 72), (2, 2, 516), (4, 1, 72), (4, 2, 516)]
TX_CASES = [(2, 258), (2, 516), (4, 516)]
SCALINGS = [1.0, 0.7]


def cn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def main():
    ref = C.CDLL(O.REF_LIB)
    ref.srsran_predecoding_diversity_multi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Planes), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                                       C.c_int, C.c_float]
    ref.srsran_precoding_diversity.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float]
    rng = np.random.default_rng(36211)
    d = {"rx_cases": np.array(RX_CASES, np.int32), "tx_cases": np.array(TX_CASES, np.int32), "scalings": np.array(SCALINGS, np.float32)}
    for ports, nrx, n in RX_CASES:
        tag = "rx_%d_%d_%d" % (ports, nrx, n)
        y = np.ascontiguousarray(cn(rng, (nrx, n)).astype(np.complex64))
        h = np.ascontiguousarray((0.9 + 0.1 * (rng.standard_normal((ports, nrx, n)) + 1j * rng.standard_normal((ports, nrx, n)))).astype(np.complex64))
        d[tag + "_y"], d[tag + "_h"] = y, h
        for si, scaling in enumerate(SCALINGS):
            x = np.zeros((ports, n // ports), np.complex64)
            csi = np.zeros(n, np.float32)
            yp = Planes(*[y[r].ctypes.data for r in range(nrx)])
            hp = Matrix(*[Planes(*[h[k, r].ctypes.data for r in range(nrx)]) for k in range(ports)])
            xp = Planes(*[x[k].ctypes.data for k in range(ports)])
            cp = (C.c_void_p * 2)(csi.ctypes.data, None)
            assert ref.srsran_predecoding_diversity_multi(yp, hp, xp, cp, nrx, ports, n, scaling) == n // ports
            d["%s_x%d" % (tag, si)], d["%s_csi%d" % (tag, si)] = x, csi
    for ports, n in TX_CASES:
        tag = "tx_%d_%d" % (ports, n)
        cw = np.ascontiguousarray(cn(rng, n).astype(np.complex64))
        d[tag + "_d"] = cw
        x = np.ascontiguousarray(cw.reshape(n // ports, ports).T)  # x[j][i] = d[ports i + j]
        for si, scaling in enumerate(SCALINGS):
            y = np.full((ports, n), np.nan + 0j, np.complex64)
            xp = Planes(*[x[k].ctypes.data for k in range(ports)])
            yp = Planes(*[y[k].ctypes.data for k in range(ports)])
            assert ref.srsran_precoding_diversity(xp, yp, ports, n // ports, scaling) == n
            assert not np.isnan(y).any()
            d["%s_y%d" % (tag, si)] = y
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
