#!/usr/bin/env python3
"""Record what the reference's srsran_chest_dl_estimate_cfg (lib/src/phy/ch_estimation/chest_dl.c:1004) gives on seeded inputs:
tests/golden/chest_dl_ref.npz.

    python tools/gen_golden_chest_dl.py          (needs the reference tree)

tools/chest_dl_ref_wrap.c includes the reference's chest_dl.c where it lies and exports one wrapper.  It is compiled with the REF_FLAGS of oracle/Makefile,
together with the reference files the call binds into (REF_FILES below, where they lie), into a temporary directory (nothing compiled is kept) and loaded
lazily: the Wiener, sequence and FFT symbols they leave undefined are never bound.

Cases (CASES below): 6 PRB (12 pilots per symbol: both end rules of a 5-tap filter inside one quarter wave), 15 PRB (an odd cell), 25 PRB (300 columns: more
than one stride of 256 lanes) and one 100-PRB case with 1 port and 1 antenna; 1, 2 and 4 ports, 1 and 2 antennas; both cyclic prefixes, both estimator
algorithms; no filter, the triangle, Gauss with fixed taps (5, 4 and 9 taps) and with automatic taps (from the REFS estimate of the same call, from the
state's, and from a state of zero: a filter of length 0 and a ce of zeros); the three noise algorithms in subframes 0, 5 and others, with a non-zero state
in; cell ids with id % 6 in {0, 2, 5}; SNR 0, 10 and 30 dB on a frequency-selective channel per (antenna, port) pair with a carrier offset within +-300 Hz;
CFO estimate on and off; rsrp_neighbour on in three.  The pilot rows and the PSS are random unit-modulus points: the estimator never looks inside them.  The
grid outside the CRS is random; the PSS, with empty sub-carriers around it and around the SSS, is there in subframes 0 and 5.  Every ce grid is full of a
sentinel before the call.

A case is drawn again unless every pair's CFO phasor sum has at least 0.1 of the sum of its terms' magnitudes.

Per case the record holds the inputs (grids, pilot rows, PSS, state), the reference's ce grids (AVERAGE: row 0 of every pair and whether every row equals
it; INTERPOLATE: whole grids), whether any sentinel was left, its results (the 111 floats of the wrapper and the state out) and its own distance to the
float64 model (tests/chest_dl_model.py): grids relative to max |ce|, power-like values relative (dB values as the power ratio they stand for), cfo in Hz."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chest_dl_model as M  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "chest_dl_ref.npz")
SENTINEL = np.complex64(-7.5 + 3.25j)
REF_FILES = ["ch_estimation/chest_common.c", "ch_estimation/refsignal_dl.c", "utils/convolution.c", "resampling/interp.c", "sync/pss.c", "common/phy_common.c",
             "utils/vector.c", "utils/vector_simd.c", "utils/debug.c", "utils/phy_logger.c"]
A, I = M.ALG_AVERAGE, M.ALG_INTERPOLATE
R, P, E = M.NOISE_REFS, M.NOISE_PSS, M.NOISE_EMPTY
FILTERS = {"none": (M.FILTER_NONE, (0.0, 0.0)), "tri": (M.FILTER_TRIANGLE, (0.1, 0.0)), "gauss": (M.FILTER_GAUSS, (4.0, 1.0)), "gauss4": (M.FILTER_GAUSS, (3.0, 1.0)),
           "gauss9": (M.FILTER_GAUSS, (8.0, 1.5)), "auto": (M.FILTER_GAUSS, (0.0, 0.0))}
# nof_prb, ports, rx, cp_nsymb, estimator, filter, noise, sf_idx, cell id, snr dB, cfo estimate, rsrp_neighbour, state in (0: zeros, 1: non-zero)
CASES = [(6, 1, 1, 7, A, "gauss", R, 1, 0, 10.0, 1, 0, 1), (6, 1, 1, 7, A, "none", R, 0, 302, 30.0, 0, 0, 1), (6, 1, 2, 6, A, "tri", P, 0, 11, 10.0, 1, 0, 1),
         (6, 2, 1, 7, A, "auto", R, 5, 302, 0.0, 1, 0, 1), (6, 2, 2, 7, I, "gauss", E, 5, 11, 10.0, 0, 0, 1), (6, 2, 1, 6, I, "none", P, 5, 0, 30.0, 1, 0, 1),
         (6, 4, 1, 7, I, "tri", R, 3, 11, 10.0, 0, 0, 1), (6, 4, 2, 6, A, "gauss", E, 0, 302, 0.0, 0, 0, 1), (6, 1, 1, 7, I, "auto", P, 4, 0, 10.0, 1, 0, 1),
         (6, 1, 1, 6, I, "auto", R, 2, 302, 30.0, 1, 0, 1), (6, 2, 1, 7, A, "gauss9", R, 7, 11, 10.0, 1, 0, 1), (6, 1, 1, 7, A, "auto", E, 3, 0, 10.0, 0, 0, 0),
         (6, 4, 1, 6, I, "gauss4", P, 0, 302, 10.0, 0, 0, 1), (6, 2, 2, 7, A, "none", P, 5, 5, 30.0, 1, 1, 1),
         (15, 4, 1, 7, I, "gauss", R, 0, 11, 10.0, 0, 1, 1), (15, 2, 2, 6, A, "tri", R, 9, 302, 0.0, 1, 0, 1), (15, 1, 2, 7, I, "auto", R, 5, 0, 30.0, 1, 0, 1),
         (25, 2, 2, 7, A, "gauss", R, 1, 302, 10.0, 1, 1, 1), (25, 2, 1, 6, I, "tri", P, 0, 11, 30.0, 1, 0, 1), (25, 4, 2, 6, A, "none", E, 5, 0, 0.0, 0, 0, 1),
         (100, 1, 1, 6, I, "gauss", R, 0, 302, 10.0, 1, 0, 1)]
CFG_KEYS = ["nof_prb", "nof_ports", "id", "cp_nsymb", "nof_rx", "sf_idx", "estimator_alg", "noise_alg", "filter_type", "rsrp_neighbour", "cfo_estimate_enable",
            "cfo_estimate_sf_mask"]


def cfg_of(case):
    prb, ports, rx, cp, alg, filt, noise, sf, cid, _, cfo_en, neigh, _ = case
    ft, coef = FILTERS[filt]
    return dict(nof_prb=prb, nof_ports=ports, id=cid, cp_nsymb=cp, nof_rx=rx, sf_idx=sf, estimator_alg=alg, noise_alg=noise, filter_type=ft,
                filter_coef=np.array(coef, np.float32), rsrp_neighbour=neigh, cfo_estimate_enable=cfo_en, cfo_estimate_sf_mask=0x3FF if sf != 7 else 0x37F)


def draw(rng, cfg, snr_db):
    """(grids [rx], pilots [2], pss): unit-modulus pilots through a three-path channel per pair, a carrier offset that turns from symbol to symbol, noise"""
    prb, ports, cid, nsymb, nrx, sf = (cfg[k] for k in ("nof_prb", "nof_ports", "id", "cp_nsymb", "nof_rx", "sf_idx"))
    nre = 12 * prb
    pilots = [np.exp(2j * np.pi * rng.random(n * prb)).astype(np.complex64) for n in (8, 4)]
    pss = np.exp(2j * np.pi * rng.random(62)).astype(np.complex64)
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
    cfo = rng.uniform(-300.0, 300.0)
    k = np.arange(nre)
    noise = lambda n: sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))  # noqa: E731
    grids = []
    for _ in range(nrx):
        g = 0.7 * (rng.standard_normal((2 * nsymb, nre)) + 1j * rng.standard_normal((2 * nsymb, nre)))
        for port in range(ports):
            taus = rng.uniform(0.0, 1.0e-6) + np.array([0.0, rng.uniform(0.1e-6, 0.3e-6), rng.uniform(0.3e-6, 0.6e-6)])
            amps = np.array([1.0, 0.5, 0.3]) * np.exp(2j * np.pi * rng.random(3))
            h = (amps[None, :] * np.exp(-2j * np.pi * 15e3 * k[:, None] * taus[None, :])).sum(axis=1)
            h /= np.sqrt(np.mean(np.abs(h) ** 2))
            rows = pilots[port // 2].reshape(M.nof_symbols(port), 2 * prb)
            for l in range(M.nof_symbols(port)):
                sym, f0 = M.nsymbol(l, nsymb, port), M.fidx(cid, l, port)
                g[sym, f0::6] = h[f0::6] * rows[l] * np.exp(2j * np.pi * cfo * 0.0005 * sym / nsymb) + noise(2 * prb)
            if port == 0 and sf in (0, 5):
                c = nre // 2 - 31
                for sym in (nsymb - 2, nsymb - 1):
                    g[sym, c - 5:c + 67] = noise(72)
                g[nsymb - 1, c:c + 62] += h[c:c + 62] * pss
        grids.append(np.ascontiguousarray(g.reshape(-1).astype(np.complex64)))
    return grids, pilots, pss


def well_conditioned(cfg, grids, pilots):
    prb, cid, nsymb = cfg["nof_prb"], cfg["id"], cfg["cp_nsymb"]
    for g in grids:
        g2 = g.reshape(2 * nsymb, 12 * prb).astype(np.complex128)
        for port in range(min(cfg["nof_ports"], 2)):
            pe = np.stack([g2[M.nsymbol(l, nsymb, port), M.fidx(cid, l, port)::6] for l in range(4)]) * np.conj(pilots[0].reshape(4, 2 * prb).astype(np.complex128))
            t = pe.reshape(-1)[:4 * prb] * np.conj(pe.reshape(-1)[4 * prb:])
            if abs(t.sum()) < 0.1 * np.abs(t).sum():
                return False
    return True


def load_wrapper(tmp):
    rlib, flags = ref_flags()
    phy = os.path.join(rlib, "src", "phy")
    so = os.path.join(tmp, "libchest_dl_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ['-DREF_CHEST_DL_C="%s"' % os.path.join(phy, "ch_estimation", "chest_dl.c"), "-shared",
                           os.path.join(ROOT, "tools", "chest_dl_ref_wrap.c")] + [os.path.join(phy, f) for f in REF_FILES] + ["-o", so, "-lm"])
    fn = C.CDLL(so, mode=os.RTLD_LAZY).chest_dl_ref
    fn.argtypes = [C.c_void_p] * 10
    fn.restype = C.c_int
    return fn


def reference_args(cfg, state, grids, pilots, pss, want=None):
    """(the wrapper's arguments, the arrays they point to: ce [4][4][points] full of the sentinel, the grids as handed in, state out [17], out [111])"""
    prb, nsymb, nrx = cfg["nof_prb"], cfg["cp_nsymb"], cfg["nof_rx"]
    u = np.array([cfg[k] if k != "cp_nsymb" else int(cfg[k] == 6) for k in CFG_KEYS], np.uint32)
    ce = np.full((4, 4, 2 * nsymb * 12 * prb), SENTINEL, np.complex64)
    ptr = (C.c_void_p * 16)(*[ce[p, a].ctypes.data if (want is None or want[p][a]) else None for p in range(4) for a in range(4)])
    gin = [np.array(g) for g in grids]
    gp = (C.c_void_p * 4)(*([g.ctypes.data for g in gin] + [None] * (4 - nrx)))
    st_in = np.concatenate([np.asarray(state["noise"], np.float32).reshape(-1), [np.float32(state["cfo"])]]).astype(np.float32)
    st_out, out = np.zeros(17, np.float32), np.zeros(111, np.float32)
    coef, p0, p1, ps = np.array(cfg["filter_coef"], np.float32), np.array(pilots[0]), np.array(pilots[1]), np.array(pss)
    args = (u.ctypes.data, coef.ctypes.data, p0.ctypes.data, p1.ctypes.data, ps.ctypes.data, st_in.ctypes.data, C.addressof(gp), C.addressof(ptr), st_out.ctypes.data,
            out.ctypes.data)
    return args, (ce, gin, st_out, out, (u, ptr, gp, st_in, coef, p0, p1, ps))


def run_reference(fn, cfg, state, grids, pilots, pss, want=None):
    """(ce [ports][rx] grids, state out [17], out [111]); want[port][rx] False: a NULL ce entry"""
    prb, ports, nsymb, nrx = cfg["nof_prb"], cfg["nof_ports"], cfg["cp_nsymb"], cfg["nof_rx"]
    args, (ce, gin, st_out, out, _) = reference_args(cfg, state, grids, pilots, pss, want)
    rc = fn(*args)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(gin, grids))  # the grids are only read
    assert np.all(ce[ports:] == SENTINEL) and np.all(ce[:, nrx:] == SENTINEL)
    return ce[:ports, :nrx].reshape(ports, nrx, 2 * nsymb * 12 * prb), st_out, out


def state_of(rng, nonzero):
    if not nonzero:
        return {"noise": np.zeros((4, 4), np.float32), "cfo": np.float32(0)}
    return {"noise": rng.uniform(0.002, 0.02, (4, 4)).astype(np.float32), "cfo": np.float32(rng.uniform(-100, 100))}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_wrapper(tmp)
        rng = np.random.default_rng(47)
        d = {"cases": np.array([[c[0], c[1], c[2], c[3], c[4], FILTERS[c[5]][0], c[6], c[7], c[8], c[10], c[11], c[12]] for c in CASES], np.int32),
             "filter_coef": np.array([FILTERS[c[5]][1] for c in CASES], np.float32), "snr_db": np.array([c[9] for c in CASES], np.float32),
             "sentinel": np.array([SENTINEL])}
        worst = np.zeros(3)
        for i, case in enumerate(CASES):
            cfg = cfg_of(case)
            state = state_of(rng, case[12])
            while True:
                grids, pilots, pss = draw(rng, cfg, case[9])
                if well_conditioned(cfg, grids, pilots):
                    break
            ce, st_out, out = run_reference(fn, cfg, state, grids, pilots, pss)
            m = M.estimate(cfg, state, grids, pilots, pss)
            sd = M.scalar_distance(M.unpack(out, st_out), M.named(m))
            dist = np.array([M.grid_distance(ce, m["ce"]), sd[0], sd[1], float(sd[2])])
            worst = np.maximum(worst, dist[:3])
            print(i, case, dist)
            average = cfg["estimator_alg"] == A
            d["grids_%d" % i], d["pilots0_%d" % i], d["pilots1_%d" % i], d["pss_%d" % i] = np.stack(grids), pilots[0], pilots[1], pss
            d["state_%d" % i] = np.concatenate([state["noise"].reshape(-1), [state["cfo"]]]).astype(np.float32)
            d["ce_%d" % i] = ce[:, :, 0, :].copy() if average else ce
            d["flags_%d" % i] = np.array([not np.any(ce == SENTINEL), bool(np.all(ce == ce[:, :, :1, :]))])
            d["out_%d" % i], d["state_out_%d" % i], d["dist_%d" % i] = out, st_out, dist
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases; the reference's worst distance to the model (grids, power-like, cfo Hz):", worst)


if __name__ == "__main__":
    main()
