"""The float64 model of the PUCCH receive side (tests/pucch_model.py) against the record of the reference (tests/golden/pucch_ref.npz, tools/gen_golden_pucch.py):
every plan integer exact, decisions, bits, DRS bits and the 20 soft bits exact, floats within the stored tolerances, the recorded tables well-formed.  No
device, no library."""
import numpy as np
import pytest

import pucch_model as M

OUTF = ("detected", "correlation", "dmrs_correlation", "ack_valid", "noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "rsrp", "rsrp_dBfs", "epre", "epre_dBfs",
        "ta_us")
DB = {"noise_estimate_dbm": "noise_estimate", "snr_db": "snr", "rsrp_dBfs": "rsrp", "epre_dBfs": "epre"}


def tol(name):
    r = M.record()
    return float(r["tol"][list(r["tol_names"]).index(name)])


def ref(c):
    r = M.record()
    return {k: r[k][c] for k in ("plan", "ce", "pe", "z", "llr", "outf", "outb", "max_corr", "early", "noise_only", "sent", "sent_drs")}


def close(got, want, rel):
    got, want = float(got), float(want)
    return (np.isnan(got) and np.isnan(want)) or got == want or abs(got - want) <= rel * abs(want)


def check_record(e, j, p, g, name, tol, arrays=True):
    """e: one job's record (outf, outb, and for the arrays llr, ce and -- where it holds them -- pe, z, early); g: what the model or the device gives for that
    job (pucch_model.decode's keys); tol: name -> tolerance.  arrays=False: the results of a plain call, which returns no arrays"""
    o = dict(zip(OUTF, e["outf"]))
    n_rs, nof_re = int(p["n_rs"]), 12 * int(p["N_sf"].sum())
    assert bool(g["detected"]) == bool(o["detected"]) and bool(g["ack_valid"]) == bool(o["ack_valid"]), name
    assert np.array_equal(np.asarray(g["pucch_bits"], np.uint8), e["outb"][:13]) and [g["drs"] % 2, g["drs"] // 2] == list(e["outb"][13:]), name
    assert abs(float(g["ta_us"]) - float(o["ta_us"])) < 0.01, name  # a multiple of 0.1
    for k in M.FLOATS:
        assert close(g[k], o[k], tol(k)), (name, k, g[k], o[k])
    for k, src in DB.items():  # 10 log10: d(dB) = 4.35 d(x) / x, plus the float rounding of the logarithm and of the + 30
        assert (np.isnan(g[k]) and np.isnan(o[k])) or abs(float(g[k]) - float(o[k])) <= 4.35 * tol(src) + 2e-6 * max(1.0, abs(float(o[k])), 30.0), (name, k, g[k], o[k])
    if not arrays:
        return
    assert np.array_equal(np.asarray(g["llr"], np.int16), e["llr"]), name
    assert np.max(np.abs(np.asarray(g["ce"]).astype(np.complex128) - e["ce"])) <= tol("ce") * np.max(np.abs(e["ce"])), name
    if "pe" in e:
        pe = e["pe"][:2 * n_rs * 12].reshape(-1, 12)
        assert np.max(np.abs(np.asarray(g["pe"]).reshape(-1, 12)[:2 * n_rs].astype(np.complex128) - pe)) <= tol("pe") * np.max(np.abs(pe)), name
    if "z" in e:
        lo = 10 if j["format"] >= M.F2 and not e["early"] else 0  # formats 2x: the reference's z[0 .. 9] were overwritten by the symbol averages
        zg, zr = np.asarray(g["z"]).reshape(-1)[:nof_re].astype(np.complex128), e["z"][:nof_re].astype(np.complex128)
        assert np.max(np.abs(zg[lo:] - zr[lo:])) <= tol("z") * np.max(np.abs(zr[lo:])), name


def check_against_record(c, g, name):
    """g: what the model or the device gives for case c (pucch_model.decode's keys); asserts everything the record holds"""
    cell, sf, j, _ = M.case(c)
    check_record(ref(c), j, M.plan(cell, sf, j), g, name, tol)


@pytest.mark.parametrize("c", range(M.n_cases()))
def test_model_equals_the_record(c):
    cell, sf, j, grid = M.case(c)
    p = M.plan(cell, sf, j)
    w = M.plan_words(p)
    if j["format"] >= M.F2:
        w[37:47] = 0  # n' of formats 2x is not exposed by the reference
    assert np.array_equal(w, ref(c)["plan"])
    m = M.decode(grid, cell, sf, j, p)
    assert m["max_corr"] == int(ref(c)["max_corr"]) and bool(m["early"]) == bool(ref(c)["early"])
    check_against_record(c, m, "case %d" % c)


def test_the_cases_cover_what_they_should():
    r = M.record()
    job, cell, sf, plan = r["job"].astype(int), r["cell"].astype(int), r["sf"].astype(int), r["plan"].astype(int)
    fmt = job[:, 0]
    assert set(fmt) == set(range(6)) and {tuple(c) for c in cell} == {(6, 0, 1), (6, 1, 77), (25, 0, 150)} and set(sf[:, 0]) == {0, 7} and set(sf[:, 1]) == {0, 1}
    f1 = fmt <= M.F1B
    assert set(job[f1, 3]) == {1, 2, 3} and 0 in job[f1, 2] and np.any(job[f1, 2] > 0)
    n_oc, n_pr = plan[f1, 27:37], plan[f1, 37:47]
    assert {(int(a), int(b) % 2) for a, b in zip(n_oc.reshape(-1), n_pr.reshape(-1))} >= {(o, q) for o in range(3) for q in range(2)}
    assert np.any(plan[f1, 6] == 3)  # N_sf = 3 rows
    sel = f1 & (job[:, 2] > 0) & (cell[:, 1] == 0)  # n_pucch on both sides of c N_cs / delta (c = 3 on the normal prefix)
    edge = 3 * job[sel, 2] // job[sel, 3]
    assert np.any(job[sel, 1] < edge) and np.any(job[sel, 1] >= edge)
    f2 = fmt >= M.F2
    assert set(job[fmt == M.F2, 7]) == {1, 4, 11, 12} and np.any(job[f2, 1] < 12 * job[f2, 4]) and np.any(job[f2, 1] >= 12 * job[f2, 4])
    assert {tuple(d) for d in r["outb"][fmt == M.F2A][:, 13:]} == {(0, 0), (1, 0)} and {tuple(d) for d in r["outb"][fmt == M.F2B][:, 13:]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert {int(b[0]) for b in r["outb"][(fmt == M.F1A) & (r["noise_only"] == 0)]} == {0, 1}
    assert {(int(b[0]), int(b[1])) for b in r["outb"][(fmt == M.F1B) & (r["noise_only"] == 0)]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    noise = r["noise_only"] == 1
    assert np.any(noise & f1) and np.any(noise & f2) and not np.any(r["outf"][noise, 0])  # noise alone is not detected
    assert np.any(r["early"] == 1) and np.any((r["th"][:, 3] > 0) & (r["early"] == 0)) and np.any(job[:, 9] == 0) and np.any(job[:, 8] == 0)
    assert np.any(job[:, 5] == 1) and np.all(r["ref_ce_elsewhere_untouched"] == 1)


def test_recorded_tables_are_well_formed():
    base, basis = M.tables()
    assert base.shape == (30, 12) and base.dtype == np.complex64 and basis.shape == (13, 20) and basis.dtype == np.uint8
    assert np.max(np.abs(np.abs(base) - 1)) < 1e-6 and set(np.unique(M.phi_of(base))) == {-3, -1, 1, 3}
    assert np.max(np.abs(np.angle(base.astype(np.complex128) * np.exp(-1j * np.pi / 4 * M.phi_of(base))))) < 1e-6
    assert set(np.unique(basis)) == {0, 1} and len({tuple(b) for b in basis}) == 13
    r = M.record()
    for i, (nof_prb, cp, cid) in enumerate(r["cells"].astype(int)):  # the library's own Gold sequence gives the reference's cell sequences
        n_cs, f_gh = M.cell_seq({"nof_prb": nof_prb, "cp": cp, "id": cid})
        assert np.array_equal(n_cs, r["n_cs_cell"][i]) and np.array_equal(f_gh, r["f_gh"][i])
    assert all(0 < float(t) < 1e-5 for t in r["tol"])
