"""numpy restatement, in double precision, of PRACH detection as the reference does it (lib/src/phy/phch/prach.c): the plan of a cell
(srsran_prach_set_cell_, :528-654, and srsran_prach_gen_seqs, :359-460), the root spectra (prach_cexp through the forward 839-point DFT with norm), the 839
bins of an occasion (forward mirror DFT of N_ifft_prach points with norm, :890-900), and per searched root corr / corr_ave / the cross sum / the window peaks
(:787-829) and the decisions (:830-859).  tests/test_prach_golden.py holds it to the record of the reference itself; the device calls are held to both.

The logical root order (TS 36.211 Table 5.7.2-4) is not in the library; it is read from the record of the reference's run (root_order)."""
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ZC = 839
NCS_UNRESTRICTED = [0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419]
NCS_RESTRICTED = [15, 18, 22, 26, 32, 38, 46, 55, 68, 82, 100, 128, 158, 202, 237]
T_CP = [3168, 21024, 6240, 21024]
T_SEQ = [24576, 24576, 2 * 24576, 2 * 24576]
SYMBOL_SZ = {6: 128, 15: 256, 25: 384, 50: 768, 75: 1024, 100: 1536}
STANDARD_SZ = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
CFG_FIELDS =["nof_prb", "config_idx", "root_seq_idx", "zero_corr_zone", "num_ra_preambles", "hs_flag", "freq_domain_offset_calc"]

_roots = None


def root_order():
    """the 838 physical roots in logical order, as the reference's run recorded them"""
    global _roots
    if _roots is None:
        _roots = np.load(os.path.join(ROOT, "tests", "golden", "prach_ref.npz"))["root_order"].astype(np.uint32)
    return _roots


def root_order_crc():
    return zlib.crc32(root_order().astype("<u2").tobytes())


def symbol_sz(nof_prb, standard=False):
    """srsran_symbol_sz; standard: after srsran_use_standard_symbol_size(true)"""
    return STANDARD_SZ[nof_prb] if standard else SYMBOL_SZ[nof_prb]


def plan(cfg, n_ifft_ul=None):
    """None where the reference (or the call) refuses the configuration; n_ifft_ul: the symbol size where it is not the default one"""
    if cfg["nof_prb"] not in SYMBOL_SZ or cfg["config_idx"] >= 64 or cfg["root_seq_idx"] >= 838:
        return None
    if cfg["zero_corr_zone"] >= (15 if cfg["hs_flag"] else 16):
        return None
    n_ul = n_ifft_ul or SYMBOL_SZ[cfg["nof_prb"]]
    f = cfg["config_idx"] // 16
    n_cs = (NCS_RESTRICTED if cfg["hs_flag"] else NCS_UNRESTRICTED)[cfg["zero_corr_zone"]]
    order = root_order()
    idx, us = [], []
    v, v_max, n_shift, n_group, n_neg = 1, 0, 0, 0, 0
    for i in range(64):
        if v > v_max:
            u = int(order[(cfg["root_seq_idx"] + len(us)) % 838])
            us.append(u)
            idx.append(i)
            if cfg["hs_flag"]:
                p = next(q for q in range(1, N_ZC + 1) if (q * u) % N_ZC == 1)
                d_u = p if p < N_ZC // 2 else N_ZC - p
                if n_cs <= d_u < N_ZC // 3:
                    n_shift = d_u // n_cs
                    d_start = 2 * d_u + n_shift * n_cs
                    n_group = N_ZC // d_start
                    n_neg = (N_ZC - 2 * d_u - n_group * d_start) // n_cs if N_ZC > 2 * d_u + n_group * d_start else 0
                elif N_ZC // 3 <= d_u <= (N_ZC - n_cs) // 2:
                    n_shift = (N_ZC - 2 * d_u) // n_cs
                    d_start = N_ZC - 2 * d_u + n_shift * n_cs
                    n_group = d_u // d_start
                    n_neg = min((d_u - n_group * d_start) // n_cs if d_u > n_group * d_start else 0, n_shift)
                else:
                    n_shift = 0  # n_group and n_neg keep the last root's values, :420-423
                v_max = max(n_shift * n_group + n_neg - 1, 0)
            else:
                v_max = 0 if n_cs == 0 else N_ZC // n_cs - 1
            v = 0
        v += 1
    n_search = cfg["num_ra_preambles"]
    if n_search < 4 or n_search > len(us):
        n_search = len(us)
    return dict(N_zc=N_ZC, N_cs=n_cs, N_ifft_ul=n_ul, N_ifft_prach=12 * n_ul, N_seq=T_SEQ[f] * n_ul // 2048, N_cp=T_CP[f] * n_ul // 2048, N_roots=len(us),
                n_wins=N_ZC // (n_cs or N_ZC), num_ra_preambles=n_search, root_seqs_idx=idx, root_u=us)


def root_spectrum(u):
    j = np.arange(N_ZC, dtype=np.int64)
    seq = np.exp(-2j * np.pi * ((u * j * (j + 1)) % (2 * N_ZC)) / (2 * N_ZC))
    return np.fft.fft(seq) / np.sqrt(N_ZC)


def begin_of(p, nof_prb, freq_offset):
    k_0 = freq_offset * 12 - nof_prb * 12 // 2 + p["N_ifft_ul"] // 2
    return 7 + 12 * k_0 + 6


def preamble(p, nof_prb, freq_offset, u, shift, delay=0):
    """the N_ifft_prach samples of one preamble behind the cyclic prefix, as srsran_prach_gen makes them (:656-690): root u cyclically shifted by `shift`
    (C_v), the forward 839-point DFT with norm, placed at begin_of() in the mirrored spectrum, the backward mirror transform with norm; then a cyclic
    delay of whole samples"""
    n = p["N_ifft_prach"]
    j = (np.arange(N_ZC, dtype=np.int64) + shift) % N_ZC
    seq = np.exp(-2j * np.pi * ((u * j * (j + 1)) % (2 * N_ZC)) / (2 * N_ZC))
    spec = np.zeros(n, np.complex128)
    b = begin_of(p, nof_prb, freq_offset)
    spec[b:b + N_ZC] = np.fft.fft(seq) / np.sqrt(N_ZC)
    x = np.fft.ifft(np.roll(spec, -(n // 2))) * np.sqrt(n)  # copy_pre of a backward mirror plan: in[k] = spec[(k + n / 2) mod n]
    return np.roll(x, delay)


def bins(p, nof_prb, freq_offset, signal):
    n = p["N_ifft_prach"]
    x = np.fft.fft(np.asarray(signal[:n], np.complex128)) / np.sqrt(n)
    out = np.roll(x, -(n // 2))  # copy_post of a forward mirror plan, dft_fftw.c:310-320: out[j] = X[(j + n / 2) mod n]
    b = begin_of(p, nof_prb, freq_offset)
    return out[b:b + N_ZC]


def correlate(p, prach_bins, spec):
    """corr, corr_ave, the cross sum, peak_values, peak_offsets of one root"""
    cs = prach_bins * np.conj(spec)
    cross = np.sum(cs[:-1] * np.conj(cs[1:]))
    corr = np.abs(np.fft.ifft(cs) * N_ZC) ** 2
    n_cs, n_wins = p["N_cs"], p["n_wins"]
    win = n_cs or N_ZC
    pv, po = np.zeros(n_wins), np.zeros(n_wins, np.uint32)
    for j in range(n_wins):
        start = (N_ZC - j * n_cs) % N_ZC
        w = corr[start:start + win]
        k = int(np.argmax(w))
        if w[k] > 0:
            pv[j], po[j] = w[k], k
    return corr, corr.sum() / N_ZC, cross, pv, po


def phase_samples(p, cross):
    """the unrounded sample count of srsran_prach_calculate_time_offset_secs, :750-760"""
    ratio = p["N_ifft_ul"] * 15000 / (N_ZC * 1250)
    return ratio * np.angle(cross) * N_ZC / (2 * np.pi)


def decide(p, cfg, roots, detect_factor=18.0):
    """roots: the tuples of correlate() for the searched roots, in order -> indices, t_offsets (float32), peak_to_avg"""
    ind, t, pa = [], [], []
    for i, (_, ave, cross, pv, po) in enumerate(roots):
        if pv.max(initial=0.0) > detect_factor * ave:
            for j in range(p["n_wins"]):
                if pv[j] > detect_factor * ave:
                    ind.append(i * p["n_wins"] + j)
                    pa.append(pv[j] / ave)
                    if cfg["freq_domain_offset_calc"]:
                        t.append(np.float32(np.round(phase_samples(p, cross))) / (np.float32(p["N_ifft_ul"]) * np.float32(15000)))
                    else:
                        t.append(np.float32(po[j]) / np.float32(1250 * N_ZC))
    return np.array(ind, np.uint32), np.array(t, np.float32), np.array(pa, np.float64)


def detect(cfg, freq_offset, signal, detect_factor=18.0, n_ifft_ul=None):
    p = plan(cfg, n_ifft_ul)
    b = bins(p, cfg["nof_prb"], freq_offset, signal)
    roots = [correlate(p, b, root_spectrum(u)) for u in p["root_u"][:p["num_ra_preambles"]]]
    return p, b, roots, decide(p, cfg, roots, detect_factor)


def margins(case, rec, aux, tol):
    """the assertions tools/gen_golden_prach.py makes on the reference alone, so that a tolerance hides no wrong decision (tests/test_prach_sizes.py makes them
    on this model for the sizes the record does not hold).  case: name, cfg; rec: ind, sent, ave, pv, po, cross; aux: f, p, corr_all, n_wins, N_cs"""
    name, f, p = case["name"], aux["f"], aux["p"]
    assert sorted(int(v) for v in rec["ind"]) == sorted(int(v) for v in rec["sent"]), (name, rec["ind"], rec["sent"])
    win = aux["N_cs"] or 839
    for i in range(rec["ave"].size):
        corr, top = aux["corr_all"][i], float(aux["corr_all"][i].max())
        thr = float(f * rec["ave"][i])
        for j in range(aux["n_wins"]):
            m = 100.0 * max(tol["pv"], tol["ave"]) * top
            assert abs(float(rec["pv"][i, j]) - thr) > m + 100.0 * tol["ave"] * thr, (name, i, j)
            if rec["pv"][i, j] > thr:
                start = (839 - j * aux["N_cs"]) % 839
                w = np.sort(corr[start:start + win])
                assert w[-1] - w[-2] > 100.0 * tol["corr"] * top, (name, i, j)
        if case["cfg"][6] and i * aux["n_wins"] in set(int(v) // aux["n_wins"] * aux["n_wins"] for v in rec["ind"]):
            x = phase_samples(p, complex(rec["cross"][i]))
            assert abs(x - np.floor(x) - 0.5) > 0.05, (name, i, x)
    if "offsets" in case:  # the peak on the first and on the last sample of a window
        got = [int(rec["po"][int(k) // aux["n_wins"], int(k) % aux["n_wins"]]) for k in rec["ind"]]
        assert got == case["offsets"] and case["offsets"][-1] == aux["N_cs"] - 1, (name, got)
