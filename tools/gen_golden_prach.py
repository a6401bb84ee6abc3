#!/usr/bin/env python3
"""Record what the reference's PRACH detector (lib/src/phy/phch/prach.c: srsran_prach_set_cfg, srsran_prach_gen, srsran_prach_detect_offset and
srsran_prach_process) gives on seeded occasions: tests/golden/prach_ref.npz.

    python tools/gen_golden_prach.py                  (needs the reference tree, oracle/liboracle.so and oracle/_ref/libsrsran_ref.so: `make -C oracle`)
    python tools/gen_golden_prach.py --check-sizes    (the same needs; the model against the reference at the stream counts the record does not hold; writes nothing)

tools/prach_ref_wrap.c includes the reference's prach.c where it lies and is compiled with the REF_FLAGS of oracle/Makefile into a temporary directory (nothing
compiled is kept).  The reference's transform backend is not available: the wrapper supplies the srsran_dft_* functions prach.c calls and routes a run to
orc_dft_c of oracle/liboracle.so (double precision, with the reference's mirror / dc / norm rules).

Preambles come from the reference's own srsran_prach_gen; the occasion is their N_ifft_prach samples behind the cyclic prefix, cyclically delayed by whole
samples, scaled, summed and noised.  Recorded per case: the configuration, what set_cell left (N_*, root_seqs_idx, the physical root of every used root), the
signal, prach_bins, per searched root corr_ave, the cross sum, the window peaks and offsets, the detection lists; the root spectra and corr of the roots in
`keep` (the first, the last and every root with a detection -- all 64 of a 64-root case would not fit a committed file).  The 838 physical roots in logical
order, as the running reference holds them, are recorded too (root_order, and their CRC32): the library has no such table, its caller hands it in.

TOLERANCES ARE MEASURED, NOT CHOSEN: the deviation of tests/prach_model.py (double precision) from the reference, max |a - b| over the row's largest magnitude,
for spectra, bins, corr, corr_ave, the cross sum, peak_values and peak_to_avg; four times the worst value over all cases is stored (the device may fuse a
multiply-add and sums in float).  So that a tolerance hides no wrong decision, it is asserted ON THE REFERENCE ALONE, for every case, that every window peak is
above the threshold by more than 100 tolerances or below it by as much, that every reported peak leads the runner-up of its window by more than 100
tolerances, that the unrounded sample count of the phase form lies more than 0.05 from a half-integer, and that the reference detects exactly the preambles sent."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_api as O  # noqa: E402
import prach_model as M  # noqa: E402
from prach_model import margins  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "prach_ref.npz")
ORACLE_LIB = os.path.join(ROOT, "oracle", "liboracle.so")

# cfg: nof_prb, config_idx, root_seq_idx, zero_corr_zone, num_ra_preambles, hs_flag, freq_domain_offset_calc
# tx: (preamble, delay in samples, gain in dB); ("root", i, ...) names the first preamble of used root i.  noise: rms relative to the strongest preamble's.
CASES = [
    dict(name="6prb_zcz0_roots_12db", cfg=(6, 0, 22, 0, 0, 0, 0), tx=[(5, 3, 0.0), (40, 11, -12.0)]),
    dict(name="6prb_zcz1_neighbours_first_last", cfg=(6, 0, 0, 1, 0, 0, 0), tx=[(10, 0, 0.0), (11, 22, 0.0)], offsets=[0, 12]),
    dict(name="6prb_zcz11", cfg=(6, 0, 100, 11, 0, 0, 0), tx=[(63, 20, 0.0), (12, 5, -3.0)]),
    dict(name="6prb_zcz15_phase", cfg=(6, 0, 7, 15, 0, 0, 1), tx=[(0, 17, 0.0), (3, 40, 0.0)]),
    dict(name="6prb_noise_only", cfg=(6, 0, 300, 8, 0, 0, 0), tx=[]),
    dict(name="6prb_nra4", cfg=(6, 0, 500, 0, 4, 0, 0), tx=[(2, 7, 0.0)]),
    dict(name="6prb_factor", cfg=(6, 0, 600, 12, 0, 0, 0), tx=[(9, 30, 0.0)], detect_factor=40.0, noise=0.5),
    dict(name="15prb_fo3_format1_phase", cfg=(15, 17, 50, 6, 0, 0, 1), fo=3, tx=[(20, 9, 0.0)]),
    dict(name="25prb_hs_fo2_format3", cfg=(25, 50, 200, 5, 0, 1, 0), fo=2, tx=[("root", 1, 6, 0.0), ("root", 7, 30, -6.0)]),
    dict(name="100prb_standard_fo40", cfg=(100, 0, 10, 12, 0, 0, 0), standard=True, fo=40, tx=[(30, 200, 0.0), (7, 50, -6.0)]),
]
QUANT = ["spec", "bins", "corr", "ave", "cross", "pv", "p2a"]


def dev(a, b):
    """max |a - b| over the largest magnitude of b"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))) if np.size(b) else 0.0


def load_wrap(tmp):
    rlib, flags = ref_flags()
    C.CDLL(O.REF_LIB, mode=os.RTLD_GLOBAL | os.RTLD_NOW)
    C.CDLL(ORACLE_LIB, mode=os.RTLD_GLOBAL | os.RTLD_NOW)
    so = os.path.join(tmp, "libprach_ref_wrap.so")
    subprocess.check_call(["gcc"] + flags + ["-I" + os.path.join(rlib, "src", "phy", "phch"), '-DREF_PRACH_C="%s"' % os.path.join(rlib, "src", "phy", "phch", "prach.c"),
                           "-shared", os.path.join(ROOT, "tools", "prach_ref_wrap.c"), "-o", so, "-lm"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def run_case(W, ref, case, rng):
    cfg = dict(zip(M.CFG_FIELDS, case["cfg"]))
    fo, factor, standard = case.get("fo", 0), case.get("detect_factor", 0.0), case.get("standard", False)
    ref.srsran_use_standard_symbol_size(C.c_bool(standard))
    d = np.array(case["cfg"], np.uint32)
    W.prach_ref_open.argtypes = [C.c_void_p, C.c_float]
    assert W.prach_ref_open(P(d), C.c_float(factor)) == 0, case["name"]
    info = np.zeros(9 + 64, np.uint32)
    W.prach_ref_info(P(info))
    N_zc, N_cs, N_ul, N, N_seq, N_cp, N_roots, n_wins, R = [int(v) for v in info[:9]]
    order = np.zeros(838, np.uint32)
    W.prach_ref_root_order(P(order))
    root_u = np.array([order[(cfg["root_seq_idx"] + i) % 838] for i in range(N_roots)], np.uint32)
    rsi = [int(v) for v in info[9:9 + N_roots]]
    # the occasion
    sig = np.zeros(N, np.complex128)
    sent, ref_rms = [], None
    for t in case["tx"]:
        if t[0] == "root":
            seq, (delay, gain) = rsi[t[1]], t[2:]
        else:
            seq, delay, gain = t
        i = max(k for k in range(N_roots) if rsi[k] <= seq)
        sent.append(i * n_wins + (seq - rsi[i]) if not cfg["hs_flag"] else i * n_wins)
        buf = np.zeros(N_cp + N_seq, np.complex64)
        assert W.prach_ref_gen(seq, fo, P(buf)) == 0
        x = np.roll(buf[N_cp:N_cp + N].astype(np.complex128), delay)
        ref_rms = ref_rms or float(np.sqrt(np.mean(np.abs(x) ** 2)))
        sig += x * 10.0 ** (gain / 20.0)
    ref_rms = ref_rms or 1.0 / np.sqrt(N)
    noise = case.get("noise", 0.05) * ref_rms / np.sqrt(2.0)
    sig = (sig + noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    pad = np.concatenate([sig, np.full(16, 7.0 + 7.0j, np.complex64)])  # sig_len may exceed N_ifft_prach: the tail is never read
    ind, toff, p2a, n = np.zeros(64 * 65, np.uint32), np.zeros(64 * 65, np.float32), np.zeros(64 * 65, np.float32), C.c_uint32(0)
    W.prach_ref_detect.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3 + [C.POINTER(C.c_uint32)]
    assert W.prach_ref_detect(fo, P(pad), pad.size, P(ind), P(toff), P(p2a), C.byref(n)) == 0
    n = n.value
    ind, toff, p2a = ind[:n].copy(), toff[:n].copy(), p2a[:n].copy()
    bins = np.zeros(N_zc, np.complex64)
    W.prach_ref_bins(P(bins))
    ave, cross = np.zeros(R, np.float32), np.zeros(R, np.complex64)
    pv, po, corr_all = np.zeros((R, n_wins), np.float32), np.zeros((R, n_wins), np.uint32), np.zeros((R, N_zc), np.float32)
    W.prach_ref_root.argtypes = [C.c_uint32] + [C.c_void_p] * 5
    for i in range(R):
        W.prach_ref_root(i, P(corr_all[i]), P(ave[i:]), P(cross[i:]), P(pv[i]), P(po[i]))
    keep = sorted({0, R - 1} | {int(k) // n_wins for k in ind})
    spec = np.zeros((len(keep), N_zc), np.complex64)
    for a, i in enumerate(keep):
        W.prach_ref_spectrum(rsi[i], P(spec[a]))
    f = np.float32(factor or 18.0)
    # ---- the model, and its deviation from the reference
    M._roots = order  # the model reads the order from the record, which is being made
    p, mb, mroots, (mind, mtoff, mp2a) = M.detect(cfg, fo, sig, float(f), n_ifft_ul=N_ul)
    assert [p[k] for k in ("N_zc", "N_cs", "N_ifft_ul", "N_ifft_prach", "N_seq", "N_cp", "N_roots", "n_wins", "num_ra_preambles")] == [int(v) for v in info[:9]], case["name"]
    assert p["root_seqs_idx"] == rsi and p["root_u"] == [int(u) for u in root_u], case["name"]
    assert np.array_equal(mind, ind) and np.array_equal(mtoff, toff), (case["name"], mind, ind, mtoff, toff)
    assert np.array_equal(np.array([r[4] for r in mroots]), po), case["name"]
    worst = dict(spec=max(dev(M.root_spectrum(int(root_u[i])), spec[a]) for a, i in enumerate(keep)), bins=dev(mb, bins),
                 corr=max(dev(mroots[i][0], corr_all[i]) for i in range(R)), ave=max(abs(mroots[i][1] - ave[i]) / ave[i] for i in range(R)),
                 cross=max(abs(mroots[i][2] - cross[i]) / ave[i] for i in range(R)),  # sum |corr_spec|^2 = corr_ave: the size of the terms of the cross sum
                 pv=max(float(np.max(np.abs(mroots[i][3] - pv[i])) / corr_all[i].max()) for i in range(R)),
                 p2a=float(np.max(np.abs(mp2a - p2a) / p2a)) if n else 0.0)
    rec = dict(cfg=d, fo=np.uint32(fo), factor=np.float32(factor), standard=np.uint8(standard), info=info[:9 + N_roots], root_u=root_u, sig=sig, bins=bins, keep=np.array(keep, np.uint32),
               spec=spec, corr=corr_all[keep], ave=ave, cross=cross, pv=pv, po=po, ind=ind, toff=toff, p2a=p2a, sent=np.array(sent, np.uint32))
    return rec, worst, dict(f=f, corr_all=corr_all, order=order, p=p, n_wins=n_wins, N_cs=N_cs)


def check_sizes():
    """--check-sizes: the reference on the occasions of tests/prach_sizes.py (D = 4, 6, 8, 8, 12, 12: stream counts the record does not hold), the model
    against it: equal detections, t_offsets and peak offsets, every deviation within the tolerance prach_ref.npz stores.  Prints, writes nothing."""
    import prach_sizes as Z

    tol = {q: float(np.load(OUT)["tol_" + q]) for q in QUANT}
    print("stored tolerances", {q: "%.3g" % tol[q] for q in QUANT})
    with tempfile.TemporaryDirectory() as tmp:
        W = load_wrap(tmp)
        ref = C.CDLL(O.REF_LIB)
        W.prach_ref_open.argtypes = [C.c_void_p, C.c_float]
        W.prach_ref_detect.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3 + [C.POINTER(C.c_uint32)]
        W.prach_ref_root.argtypes = [C.c_uint32] + [C.c_void_p] * 5
        over = []
        for size in Z.SIZES:
            cfg = Z.cfg_of(size)
            ref.srsran_use_standard_symbol_size(C.c_bool(size[1]))
            d = np.array([cfg[k] for k in M.CFG_FIELDS], np.uint32)
            assert W.prach_ref_open(P(d), C.c_float(0.0)) == 0, size
            info = np.zeros(9 + 64, np.uint32)
            W.prach_ref_info(P(info))
            N_ul, R, n_wins = int(info[2]), int(info[8]), int(info[7])
            assert N_ul == M.symbol_sz(*size)
            rsi = [int(v) for v in info[9:9 + int(info[6])]]
            for o, (fo, sig, sent) in enumerate(Z.occasions(size)):
                sig = np.array(sig)
                ind, toff, p2a, n = np.zeros(64 * 65, np.uint32), np.zeros(64 * 65, np.float32), np.zeros(64 * 65, np.float32), C.c_uint32(0)
                assert W.prach_ref_detect(fo, P(sig), sig.size, P(ind), P(toff), P(p2a), C.byref(n)) == 0
                ind, toff, p2a = ind[:n.value], toff[:n.value], p2a[:n.value]
                bins = np.zeros(839, np.complex64)
                W.prach_ref_bins(P(bins))
                ave, cross = np.zeros(R, np.float32), np.zeros(R, np.complex64)
                pv, po, corr = np.zeros((R, n_wins), np.float32), np.zeros((R, n_wins), np.uint32), np.zeros((R, 839), np.float32)
                for i in range(R):
                    W.prach_ref_root(i, P(corr[i]), P(ave[i:]), P(cross[i:]), P(pv[i]), P(po[i]))
                spec = np.zeros((R, 839), np.complex64)
                for i in range(R):
                    W.prach_ref_spectrum(rsi[i], P(spec[i]))
                p, mb, mroots, (mind, mtoff, mp2a) = M.detect(cfg, fo, sig, 18.0, n_ifft_ul=N_ul)
                assert [p[k] for k in ("N_zc", "N_cs", "N_ifft_ul", "N_ifft_prach", "N_seq", "N_cp", "N_roots", "n_wins", "num_ra_preambles")] == [int(v) for v in info[:9]]
                assert np.array_equal(mind, ind) and [int(v) for v in ind] == sent and np.array_equal(mtoff, toff), (size, o, mind, ind, mtoff, toff)
                assert np.array_equal(np.array([r[4] for r in mroots]), po), (size, o)
                w = dict(spec=max(dev(M.root_spectrum(p["root_u"][i]), spec[i]) for i in range(R)), bins=dev(mb, bins), corr=max(dev(mroots[i][0], corr[i]) for i in range(R)),
                         ave=max(abs(mroots[i][1] - ave[i]) / ave[i] for i in range(R)), cross=max(abs(mroots[i][2] - cross[i]) / ave[i] for i in range(R)),
                         pv=max(float(np.max(np.abs(mroots[i][3] - pv[i])) / corr[i].max()) for i in range(R)), p2a=float(np.max(np.abs(mp2a - p2a) / p2a)))
                over += [(Z.name(size), o, q) for q in QUANT if w[q] > tol[q]]
                print("%-22s fo %2d %s detections %s  deviation %s" % (Z.name(size), fo, "wraps" if Z.wraps(p, size[0], fo) else "     ", ind,
                                                                      {q: "%.2g" % w[q] for q in QUANT}), flush=True)
        ref.srsran_use_standard_symbol_size(C.c_bool(False))
        W.prach_ref_close()
    assert not over, ("deviations above the stored tolerance", over)
    print("every deviation lies within the stored tolerances")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        W = load_wrap(tmp)
        ref = C.CDLL(O.REF_LIB)
        rng = np.random.default_rng(839)
        d, worst, keep = {"names": np.array([c["name"] for c in CASES])}, {q: 0.0 for q in QUANT}, []
        for c, case in enumerate(CASES):
            rec, w, aux = run_case(W, ref, case, rng)
            for q in QUANT:
                worst[q] = max(worst[q], float(w[q]))
            keep.append((case, rec, aux))
            for k, v in rec.items():
                d["%s_%d" % (k, c)] = v
            print("%-36s detections %s  p2a %s  deviation %s" % (case["name"], rec["ind"], np.round(rec["p2a"], 1), {q: "%.2g" % w[q] for q in QUANT}), flush=True)
        ref.srsran_use_standard_symbol_size(C.c_bool(False))
        W.prach_ref_close()
        tol = {q: 4.0 * worst[q] for q in QUANT}
        for case, rec, aux in keep:
            margins(case, rec, aux, tol)
        for q in QUANT:
            d["tol_" + q] = np.float64(tol[q])
        d["root_order"] = keep[0][2]["order"].astype(np.uint16)
        d["root_order_crc"] = np.uint32(zlib.crc32(keep[0][2]["order"].astype("<u2").tobytes()))
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes,", len(CASES), "cases, tolerances", {q: "%.3g" % tol[q] for q in QUANT})
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    check_sizes() if "--check-sizes" in sys.argv[1:] else main()
