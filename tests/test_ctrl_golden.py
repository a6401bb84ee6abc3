"""CPU-only checks of the PCFICH / PHICH model and map against what the reference gave (tests/golden/ctrl_ref.npz, written by tools/gen_golden_ctrl.py): the
model's index tables and group counts (tests/ctrl_model.py) and the library's (srsran_hip_regs_pcfich_table / _phich_ngroups / _phich_table, host code: no
device) equal the recorded ones exactly; the model's cfi and ack_value equal the reference's in every case; its floats lie within a quarter of the stored
tolerances (each is four times the deviation the generator measured on its CPU: data_f against the case's rms, corr against |corr|, data_rx and distance against
the rms over the case's resources).  The loaders are shared with tests/test_gpu_ctrl.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ctrl_model as KM
import pdcch_map_model as PM
from test_pdcch_sf_golden import sf_struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctrl_ref.npz")
S_KEYS = ["sf", "pcfich_table", "phich_table", "rx", "ce", "noise", "cfi_sent", "cfi", "corr", "corr3", "data_f", "d", "res", "sent", "ack", "distance", "bits", "z"]
E_KEYS = ["sf", "cfi3_to_2", "rx", "pilots0", "pilots1", "cfi", "corr", "noise", "nof_cce", "cand", "bits", "crc", "res", "sent", "ack", "distance"]


@functools.lru_cache(maxsize=None)
def record():
    return dict(np.load(GOLDEN))


def tol(what):
    return float(record()["%s_tol" % what])


def rms(v):
    return float(np.sqrt(np.mean(np.abs(np.asarray(v, np.float64)) ** 2)))


def map_cases():
    r = record()
    return [dict(name=str(n), sf=PM.from_row(r["m_sf"][i]), pcfich_table=r["m_pcfich_%d" % i], phich_table=r["m_phich_%d" % i]) for i, n in enumerate(r["m_names"])]


def _cases(prefix, keys):
    r = record()
    out = []
    for i, n in enumerate(r["%s_names" % prefix]):
        c = {k: r["%s_%s_%d" % (prefix, k, i)] for k in keys}
        c.update(name=str(n), sf=PM.from_row(c["sf"]), noise=float(c["noise"]))
        out.append(c)
    return out


def signal_cases():
    return _cases("s", S_KEYS)


def est_cases():
    return _cases("e", E_KEYS)


def all_tables():
    return map_cases() + [dict(name="s_" + c["name"], sf=c["sf"], pcfich_table=c["pcfich_table"], phich_table=c["phich_table"]) for c in signal_cases()]


def float_devs(c, data_f, corr, bits, distance):
    """the four deviations of one signal case from the reference, in the units of the stored tolerances"""
    ref_corr = float(c["corr"])
    return dict(data_f=float(np.abs(np.asarray(data_f, np.float64) - c["data_f"]).max()) / rms(c["data_f"]),
                corr=abs(float(corr) - ref_corr) / abs(ref_corr) if ref_corr != 0 else float(float(corr) != 0),
                bits=float(np.abs(np.asarray(bits, np.float64) - c["bits"]).max()) / rms(c["bits"]),
                distance=float(np.abs(np.asarray(distance, np.float64) - c["distance"]).max()) / rms(c["distance"]))


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_the_record_holds_the_cases_it_should():
    m, s, e = map_cases(), signal_cases(), est_cases()
    assert len(m) >= 11 and len(s) == 8 and 2 <= len(e) <= 3
    assert all(0 < tol(k) < 1e-5 for k in ("data_f", "corr", "bits", "distance"))
    sfs = [c["sf"] for c in m]
    assert {6, 15, 25} <= {f["cell_nof_prb"] for f in sfs} and any(f["cell_id"] >= 2 * f["cell_nof_prb"] for f in sfs if f["cell_nof_prb"] == 15)
    assert any(f["cp_nsymb"] == 6 for f in sfs) and {0, 2} <= {f["phich_mi"] for f in sfs} and {0, 3} <= {f["phich_resources"] for f in sfs}
    assert {f["mbsfn_or_sf1_6_tdd"] for f in sfs if f["phich_length"] == 1} == {0, 1}
    assert any(c["phich_table"].shape[0] == 0 for c in m) and any((c["phich_table"] // (12 * c["sf"]["cell_nof_prb"])).max(initial=0) == 2 for c in m)
    assert {(c["sf"]["cell_nof_ports"], c["sf"]["nof_rx"]) for c in s} == {(p, a) for p in (1, 2, 4) for a in (1, 2)}
    assert any(c["noise"] > 0 and c["sf"]["cell_nof_ports"] == 1 for c in s) and {int(c["cfi"]) for c in s if c["cfi_sent"]} == {1, 2, 3}
    nonpos = [c for c in s if not c["cfi_sent"]]
    assert len(nonpos) == 1 and nonpos[0]["cfi"] == 1 and nonpos[0]["corr"] == 0 and np.all(nonpos[0]["corr3"] < 0)
    for c in s:
        sent = c["sent"] >= 0
        assert np.array_equal(c["ack"][sent], c["sent"][sent]) and {0, 1} <= set(c["sent"][sent]) and np.any(~sent), c["name"]
        groups = c["res"][sent][:, 0]
        assert max(np.sum(groups == g) for g in set(groups)) >= 2, c["name"]  # several sequences of one group at once
        lead = np.abs(c["distance"]) / (tol("distance") * rms(c["distance"]))
        assert np.all(lead[sent] > 100) and np.all(lead > 2), c["name"]
        if c["cfi_sent"]:
            best, second = np.sort(c["corr3"].astype(np.float64))[::-1][:2]
            assert c["cfi"] == c["cfi_sent"] and best - second > 100 * tol("corr") * abs(best), c["name"]
    assert {c["sf"]["cell_nof_prb"] for c in e} >= {6, 15} and {c["sf"]["cell_nof_ports"] for c in e} >= {1, 2}
    rule = [c for c in e if c["cfi3_to_2"]]
    assert len(rule) == 1 and rule[0]["sf"]["cfi"] == 3 and rule[0]["cfi"] == 2
    assert all(len(c["cand"]) >= 2 and np.all(c["crc"] != 0) for c in e)


@pytest.mark.parametrize("c", all_tables(), ids=lambda c: c["name"])
def test_model_and_library_tables_equal_the_recorded_ones(L, c):
    from srslte_amd import capi

    ngroups = c["phich_table"].shape[0]
    assert np.array_equal(KM.pcfich_table(c["sf"]), c["pcfich_table"]) and KM.phich_ngroups(c["sf"]) == ngroups
    sf = sf_struct(capi, c["sf"])
    got = np.full(16 + 4, 0xEEEEEEEE, np.uint32)
    assert L.srsran_hip_regs_pcfich_table(C.byref(sf), got.ctypes.data) == 16
    assert np.array_equal(got[:16], c["pcfich_table"]) and np.all(got[16:] == 0xEEEEEEEE)
    assert L.srsran_hip_regs_phich_ngroups(C.byref(sf)) == ngroups
    for g in range(ngroups):
        assert np.array_equal(KM.phich_table(c["sf"], g), c["phich_table"][g]), g
        got = np.full(12 + 4, 0xEEEEEEEE, np.uint32)
        assert L.srsran_hip_regs_phich_table(C.byref(sf), g, got.ctypes.data) == 12
        assert np.array_equal(got[:12], c["phich_table"][g]) and np.all(got[12:] == 0xEEEEEEEE), g
    assert L.srsran_hip_regs_phich_table(C.byref(sf), ngroups, got.ctypes.data) == -1
    for cfi in (1, 2, 3):  # the cfi is not read
        other = sf_struct(capi, dict(c["sf"], cfi=cfi))
        got = np.zeros(16, np.uint32)
        assert L.srsran_hip_regs_pcfich_table(C.byref(other), got.ctypes.data) == 16 and np.array_equal(got, c["pcfich_table"])
        assert L.srsran_hip_regs_phich_ngroups(C.byref(other)) == ngroups
    if c["sf"]["cp_nsymb"] == 6:
        assert np.array_equal(c["phich_table"][0::2], c["phich_table"][1::2])  # group g reads mapping unit g / 2


@functools.lru_cache(maxsize=None)
def model_of(name):
    """the model's two receivers on a recorded signal case, computed once"""
    c = next(c for c in signal_cases() if c["name"] == name)
    p = KM.pcfich_decode(c["sf"], c["rx"], c["ce"], c["noise"], c["pcfich_table"])
    r = [KM.phich_decode(c["sf"], c["rx"], c["ce"], c["noise"], int(g), int(s), c["phich_table"][int(g)]) for g, s in c["res"]]
    return p, r


@pytest.mark.parametrize("c", signal_cases(), ids=lambda c: c["name"])
def test_model_decisions_equal_the_reference(c):
    p, r = model_of(c["name"])
    assert p["cfi"] == c["cfi"] and [x["ack_value"] for x in r] == list(c["ack"])
    if not c["cfi_sent"]:
        assert p["corr"] == 0 and np.all(p["corr3"] < 0)


@pytest.mark.parametrize("c", signal_cases(), ids=lambda c: c["name"])
def test_model_floats_are_the_reference_to_the_measured_tolerance(c):
    p, r = model_of(c["name"])
    dev = float_devs(c, p["data_f"], p["corr"], [x["bits"] for x in r], [x["distance"] for x in r])
    print("%s: %s" % (c["name"], "  ".join("%s %.3g (tol / 4 = %.3g)" % (k, v, tol(k) / 4) for k, v in dev.items())))
    for k, v in dev.items():
        assert v <= tol(k) / 4, k
