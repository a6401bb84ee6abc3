"""CPU-only checks of the PDCCH search's model and REG map against what the reference gave (tests/golden/pdcch_sf_ref.npz, written by
tools/gen_golden_pdcch_sf.py): the model's index tables (tests/pdcch_map_model.py) and the library's (srsran_hip_regs_pdcch_table, host code: no device) equal
the recorded ones exactly; the model's soft bits lie within llr_tol / 4 of the reference's (llr_tol is four times the deviation the generator measured on its
CPU, relative to the region's rms); every DCI-carrying candidate decodes from the model's soft bits to the reference's payload and CRC remainder.
The loaders are shared with tests/test_gpu_pdcch_sf.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import pdcch_map_model as PM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdcch_sf_ref.npz")


@functools.lru_cache(maxsize=None)
def record():
    return dict(np.load(GOLDEN))


def llr_tol():
    return float(record()["llr_tol"])


def map_cases():
    r = record()
    return [dict(name=str(n), sf=PM.from_row(r["m_sf"][i]), table=r["m_table_%d" % i]) for i, n in enumerate(r["m_names"])]


def signal_cases():
    r = record()
    keys = ["sf", "table", "rx", "ce", "noise", "llr", "d", "cand", "carry", "bits", "crc", "mean", "dec"]
    out = []
    for i, n in enumerate(r["s_names"]):
        c = {k: r["s_%s_%d" % (k, i)] for k in keys}
        c.update(name=str(n), sf=PM.from_row(c["sf"]), noise=float(c["noise"]))
        out.append(c)
    return out


def all_tables():
    return map_cases() + [dict(name="s_" + c["name"], sf=c["sf"], table=c["table"]) for c in signal_cases()]


@functools.lru_cache(maxsize=None)
def model_of(name):
    """the model's front end on a recorded signal case, computed once"""
    c = next(c for c in signal_cases() if c["name"] == name)
    return PM.extract_llr(c["sf"], c["rx"], c["ce"], c["noise"], c["table"])


def rel_dev(a, b):
    """max |a - b| / rms(b)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.sqrt(np.mean(b * b)))


def sf_struct(capi, sf):
    return capi.HipPdcchSf(*[sf[f] for f in PM.FIELDS])


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_the_record_holds_the_cases_it_should():
    m, s = map_cases(), signal_cases()
    assert len(m) >= 15 and len(s) == 8 and 0 < llr_tol() < 1e-4
    assert m[0]["table"].size == 4 * 18  # 6 PRB, cfi 1: 23 free REGs, 18 after the cut
    assert {(c["sf"]["cell_nof_ports"], c["sf"]["nof_rx"]) for c in s} == {(p, a) for p in (1, 2, 4) for a in (1, 2)}
    assert any(c["noise"] > 0 and c["sf"]["cell_nof_ports"] == 1 for c in s) and any(c["noise"] == 0 and c["sf"]["cell_nof_ports"] == 1 for c in s)
    for c in s:
        nof_cce = c["table"].size // 36
        assert c["carry"].sum() >= 3 and np.all(c["dec"][c["carry"] == 1] == 1), c["name"]
        assert np.any((c["dec"] == 0) & (c["mean"] == 0)), c["name"]  # the candidate over REs that are all zero
        assert c["rx"].shape == (c["sf"]["nof_rx"], PM.nof_ctrl_symbols(c["sf"]) * 12 * c["sf"]["cell_nof_prb"])
        assert nof_cce < 8 or any(int(k[1]) == 3 and int(k[0]) + 8 == nof_cce for k in c["cand"]), c["name"]
    wide = next(c for c in s if c["name"].endswith("wide"))
    ncce, lev, _ = [int(v) for v in wide["cand"][-2]]
    w = np.abs(wide["llr"][72 * ncce:72 * ncce + (72 << lev)])
    assert np.log2(w.max() / w.min()) > 38  # the double sum of the mean rule rounds: its order shows


@pytest.mark.parametrize("c", all_tables(), ids=lambda c: c["name"])
def test_model_and_library_tables_equal_the_recorded_ones(L, c):
    from srslte_amd import capi

    assert np.array_equal(PM.reg_table(c["sf"]), c["table"])
    sf = sf_struct(capi, c["sf"])
    nregs = c["table"].size // 4
    assert nregs % 9 == 0 and L.srsran_hip_regs_pdcch_nregs(C.byref(sf)) == nregs
    got = np.full(c["table"].size + 4, 0xEEEEEEEE, np.uint32)
    assert L.srsran_hip_regs_pdcch_table(C.byref(sf), got.ctypes.data) == nregs
    assert np.array_equal(got[:-4], c["table"]) and np.all(got[-4:] == 0xEEEEEEEE)
    assert c["table"].max() < PM.nof_ctrl_symbols(c["sf"]) * 12 * c["sf"]["cell_nof_prb"] and np.unique(c["table"]).size == c["table"].size


@pytest.mark.parametrize("c", signal_cases(), ids=lambda c: c["name"])
def test_model_soft_bits_are_the_reference_to_the_measured_tolerance(c):
    m = model_of(c["name"])
    dev = rel_dev(m["llr"], c["llr"])
    print("%s: soft bits %.3g of the rms (llr_tol / 4 = %.3g)" % (c["name"], dev, llr_tol() / 4))
    assert dev <= llr_tol() / 4


@pytest.mark.parametrize("c", signal_cases(), ids=lambda c: c["name"])
def test_model_search_gives_the_reference_payloads(c):
    m = model_of(c["name"])
    res = PM.search(m["llr"], [tuple(int(v) for v in k) for k in c["cand"]])
    for i, r in enumerate(res):
        if c["carry"][i]:
            nof_bits = int(c["cand"][i][2])
            assert r["decoded"] and r["crc_rem"] == c["crc"][i] and np.array_equal(r["bits"], c["bits"][i][:nof_bits + 16]), (c["name"], i)
        if c["mean"][i] == 0:
            assert not r["decoded"] and r["mean"] == 0, (c["name"], i)
