"""tests/prach_model.py (numpy, double precision) held to the record of the reference's PRACH detector, tests/golden/prach_ref.npz (tools/gen_golden_prach.py:
srsran_prach_set_cfg, srsran_prach_gen, srsran_prach_detect_offset and srsran_prach_process of the reference itself, its transforms held by the oracle's
double-precision DFT).  The plan fields, the detection lists, their order, the peak offsets and both forms of t_offsets are exact; root spectra, prach_bins,
corr, corr_ave, the cross sum, peak_values and peak_to_avg lie within the tolerances the generator MEASURED (four times the worst deviation of this model from
the reference; the generator asserts, on the reference alone, that no decision lies within 100 tolerances of its threshold).  The recorded logical root order, which the library's callers hand in, is a
permutation with the recorded CRC.  Runs on the CPU."""
import os

import numpy as np
import pytest

import prach_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prach_ref.npz")
INFO = ["N_zc", "N_cs", "N_ifft_ul", "N_ifft_prach", "N_seq", "N_cp", "N_roots", "n_wins", "num_ra_preambles"]

_record = None


def record():
    global _record
    if _record is None:
        z = np.load(GOLD)
        _record = {k: z[k] for k in z.files}
    return _record


def names():
    return [str(n) for n in record()["names"]]


def case(c):
    """the record of case c as a dict, with cfg as the dict prach_model takes"""
    g = record()
    d = {k[:-len("_%d" % c)]: g[k] for k in g if k.endswith("_%d" % c) and not k.startswith("tol_")}
    d["cfg_dict"] = dict(zip(M.CFG_FIELDS, (int(v) for v in d["cfg"])))
    d["info_dict"] = dict(zip(INFO, (int(v) for v in d["info"][:9])))
    d["root_seqs_idx"] = [int(v) for v in d["info"][9:]]
    d["factor_used"] = float(d["factor"]) or 18.0
    return d


def tol(q):
    return float(record()["tol_" + q])


def rel(a, b, scale):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / float(scale) if np.size(b) else 0.0


def test_the_record_has_the_cases_the_tests_stand_on():
    n = names()
    assert len(n) == 10 and os.path.getsize(GOLD) < 1000000
    cells = {int(case(c)["info_dict"]["N_ifft_prach"]) // 1536 for c in range(len(n))}
    assert cells == {1, 2, 3, 16}  # no combine, the first with one, odd D, the 20 MHz cell
    zones = {(int(case(c)["cfg"][0]), int(case(c)["cfg"][3])) for c in range(len(n))}
    assert {(6, 0), (6, 1), (6, 11), (6, 15)} <= zones
    assert any(case(c)["ind"].size == 0 for c in range(len(n))) and any(case(c)["ind"].size and case(c)["ind"].max() > 63 for c in range(len(n)))
    assert any(case(c)["cfg"][5] for c in range(len(n))) and any(case(c)["cfg"][6] and case(c)["ind"].size for c in range(len(n)))
    assert any(case(c)["cfg"][4] == 4 and case(c)["info_dict"]["num_ra_preambles"] == 4 < case(c)["info_dict"]["N_roots"] for c in range(len(n)))
    assert {int(case(c)["cfg"][1]) // 16 for c in range(len(n))} == {0, 1, 3} and any(case(c)["fo"] for c in range(len(n)))
    for q in ("spec", "bins", "corr", "ave", "cross", "pv", "p2a"):
        assert 0 < tol(q) < 1e-5, q


def test_recorded_root_order_is_a_permutation_with_its_crc():
    order = M.root_order()
    assert sorted(int(u) for u in order) == list(range(1, 839))
    assert M.root_order_crc() == int(record()["root_order_crc"]) and np.all(order[0::2] + order[1::2] == 839)


@pytest.mark.parametrize("c", range(10))
def test_model_against_the_record(c):
    g = case(c)
    cfg = g["cfg_dict"]
    p, bins, roots, (ind, toff, p2a) = M.detect(cfg, int(g["fo"]), g["sig"], g["factor_used"], n_ifft_ul=g["info_dict"]["N_ifft_ul"])
    assert {k: p[k] for k in INFO} == g["info_dict"] and p["root_seqs_idx"] == g["root_seqs_idx"] and p["root_u"] == [int(u) for u in g["root_u"]]
    assert p["N_ifft_ul"] == M.symbol_sz(cfg["nof_prb"], bool(g["standard"]))
    # exact: the lists, their order, the offsets, both forms of t_offsets
    assert np.array_equal(ind, g["ind"]) and np.array_equal(toff, g["toff"]) and toff.dtype == g["toff"].dtype
    assert np.array_equal(np.array([r[4] for r in roots]), g["po"])
    assert sorted(int(v) for v in g["ind"]) == sorted(int(v) for v in g["sent"])
    # within the measured tolerances
    assert rel(bins, g["bins"], np.abs(g["bins"]).max()) <= tol("bins")
    for a, i in enumerate(g["keep"]):
        assert rel(M.root_spectrum(p["root_u"][i]), g["spec"][a], np.abs(g["spec"][a]).max()) <= tol("spec"), i
        assert rel(roots[i][0], g["corr"][a], g["corr"][a].max()) <= tol("corr"), i
    for i, r in enumerate(roots):
        assert abs(r[1] - g["ave"][i]) / g["ave"][i] <= tol("ave"), i
        assert abs(r[2] - g["cross"][i]) / g["ave"][i] <= tol("cross"), i
    top = {int(i): float(g["corr"][a].max()) for a, i in enumerate(g["keep"])}
    for i in top:  # peak_values are compared over the root's largest corr, which the record holds for the kept roots
        assert rel(roots[i][3], g["pv"][i], top[i]) <= tol("pv"), i
    if ind.size:
        assert float(np.max(np.abs(p2a - g["p2a"]) / g["p2a"])) <= tol("p2a")


def test_index_may_exceed_63_and_clamp_counts_roots():
    """i * n_wins + j with the last root partly used, and num_ra_preambles compared with the number of ROOTS (prach.c:602)"""
    p = M.plan(dict(zip(M.CFG_FIELDS, (6, 0, 100, 11, 0, 0, 0))))
    assert (p["N_cs"], p["n_wins"], p["N_roots"], p["num_ra_preambles"]) == (93, 9, 8, 8) and (p["N_roots"] - 1) * p["n_wins"] + p["n_wins"] - 1 == 71
    p = M.plan(dict(zip(M.CFG_FIELDS, (6, 0, 0, 1, 52, 0, 0))))
    assert (p["n_wins"], p["N_roots"], p["num_ra_preambles"]) == (64, 1, 1) and 839 - 64 * 13 == 7  # 52 "preambles" > 1 root: clamped; 7 samples in no window
    p = M.plan(dict(zip(M.CFG_FIELDS, (6, 0, 0, 0, 10, 0, 0))))
    assert (p["n_wins"], p["N_roots"], p["num_ra_preambles"]) == (1, 64, 10)
