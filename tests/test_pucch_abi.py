"""CPU-only checks of the PUCCH entry points (include/srsran_amd/phy_pucch_abi.h), in the manner of test_prach_abi.py: the library exports them and the ctypes
mirror binds them, the structs have the declared sizes in the header and in the mirror, a plain C caller compiles under -Wall -Werror,
srsran_hip_pucch_set_tables refuses what it should, takes what it is handed and NULL removes it, srsran_hip_pucch_plan (pure host code) equals both records of
the reference (pucch_ref.npz, pucch_sweep_ref.npz) and tests/pucch_model.py over the sweep of the reference's pucch_test.c (:214-217: formats x delta 1 .. 3 x N_cs step delta x n_pucch 1, 51, 101)
on both prefixes, every refusal that needs no device comes with one line on stderr and zeroed results, and a valid call without a device fails loudly.  No
kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import pucch_model as M
from test_conv_abi import _compile_run, _one_line

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_pucch_set_tables", "srsran_hip_pucch_plan", "srsran_hip_pucch_decode_multi", "srsran_hip_pucch_decode", "srsran_hip_pucch_decode_dbg",
           "srsran_hip_chest_ul_estimate_pucch"]


def set_tables(lib, base=None, basis=None):
    """hand the recorded tables (or others) to the library"""
    b = np.ascontiguousarray(M.tables()[0] if base is None else base, np.complex64)
    m = np.ascontiguousarray(M.tables()[1] if basis is None else basis, np.uint8)
    return lib.srsran_hip_pucch_set_tables(b.ctypes.data, m.ctypes.data)


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    lib = capi.lib()
    assert set_tables(lib) == 0
    return lib


def structs(capi, cell, sf, j):
    job = capi.HipPucchJob(*([j[k] for k in M.JOB_FIELDS] + [(C.c_float * 3)(*j["filter"])] + [j[k] for k in M.TH_FIELDS]))
    return capi.HipPucchCell(*[cell[k] for k in M.CELL_FIELDS]), capi.HipPucchSf(sf["tti"], sf["shortened"]), job


def plan_of(L, capi, cell, sf, j):
    p = capi.HipPucchPlan()
    c, s, job = structs(capi, cell, sf, j)
    rc = L.srsran_hip_pucch_plan(C.byref(c), C.byref(s), C.byref(job), C.byref(p))
    return rc, np.frombuffer(bytes(p), np.uint32).astype(np.int64)


def a_job(**kw):
    j = dict(zip(M.JOB_FIELDS, (M.F1A, 7, 0, 1, 0, 0, 0x1234, 0, 1, 3)))
    j["filter"] = [0.3333, 0.3334, 0.3333]
    j.update(zip(M.TH_FIELDS, (0.5, 0.5, 0.5, 0.0)))
    j.update(kw)
    return j


CELL, SF = {"nof_prb": 25, "cp": 0, "id": 150}, {"tti": 7, "shortened": 0}


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_struct_sizes_in_header_and_mirror():
    from srslte_amd import capi

    items = ["sizeof(srsran_hip_pucch_cell_t)", "sizeof(srsran_hip_pucch_sf_t)", "sizeof(srsran_hip_pucch_job_t)", "sizeof(srsran_hip_pucch_plan_t)",
             "sizeof(srsran_hip_pucch_res_t)", "sizeof(srsran_hip_pucch_dbg_t)", "offsetof(srsran_hip_pucch_job_t, filter)",
             "offsetof(srsran_hip_pucch_job_t, threshold_dmrs_detection)", "offsetof(srsran_hip_pucch_plan_t, n_cs)", "offsetof(srsran_hip_pucch_plan_t, dmrs_n_oc)",
             "offsetof(srsran_hip_pucch_res_t, pucch_bits)", "offsetof(srsran_hip_pucch_res_t, ack_valid)", "offsetof(srsran_hip_pucch_res_t, noise_estimate)",
             "offsetof(srsran_hip_pucch_res_t, ta_us)", "offsetof(srsran_hip_pucch_dbg_t, pilot_estimates)", "SRSRAN_HIP_PUCCH_MAX_JOBS", "SRSRAN_HIP_PUCCH_MAX_SYMBOLS"]
    src = ('#include "srsran_amd/phy_pucch_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("pucch_layout", src, os.path.join(ROOT, "include")).split()]
    assert got == [12, 8, 68, 260, 64, 32, 40, 64, 68, 236, 12, 27, 28, 60, 24, 256, 120]
    assert [C.sizeof(capi.HipPucchCell), C.sizeof(capi.HipPucchSf), C.sizeof(capi.HipPucchJob), C.sizeof(capi.HipPucchPlan), C.sizeof(capi.HipPucchRes),
            C.sizeof(capi.HipPucchDbg), capi.HipPucchJob.filter.offset, capi.HipPucchJob.threshold_dmrs_detection.offset, capi.HipPucchPlan.n_cs.offset,
            capi.HipPucchPlan.dmrs_n_oc.offset, capi.HipPucchRes.pucch_bits.offset, capi.HipPucchRes.ack_valid.offset, capi.HipPucchRes.noise_estimate.offset,
            capi.HipPucchRes.ta_us.offset, capi.HipPucchDbg.pilot_estimates.offset] == got[:-2]


def test_header_takes_a_plain_c_callers_arrays():
    """a C caller that holds what a caller of get_pucch holds compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_pucch_abi.h"\n#include <stddef.h>\n'
           "int take(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* jobs, const cf_t* grid, cf_t* ce) {\n"
           "  static cf_t base[30][12], z[SRSRAN_HIP_PUCCH_MAX_SYMBOLS]; static uint8_t basis[13][20]; int16_t llr[SRSRAN_HIP_PUCCH2_NOF_BITS];\n"
           "  srsran_hip_pucch_res_t res[4]; srsran_hip_pucch_plan_t plan; srsran_hip_pucch_dbg_t dbg = {z, llr, NULL, NULL};\n"
           "  int rc = srsran_hip_pucch_set_tables(base, basis) + srsran_hip_pucch_plan(cell, sf, jobs, &plan);\n"
           "  rc += srsran_hip_pucch_decode_multi(cell, sf, 4, jobs, grid, res) + srsran_hip_pucch_decode(cell, sf, jobs, grid, res);\n"
           "  rc += srsran_hip_pucch_decode_dbg(cell, sf, jobs, grid, res, &dbg) + srsran_hip_chest_ul_estimate_pucch(cell, sf, jobs, grid, ce, res);\n"
           "  return rc + (int)res[0].detected + (int)plan.n_rs; }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0) : 0; }\n")
    assert _compile_run("pucch_abi", src, os.path.join(ROOT, "include"), link=True) == ""


# ---- the tables are the caller's
def test_tables_are_the_callers(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    base, basis = M.tables()
    try:
        assert L.srsran_hip_pucch_set_tables(None, None) == 0 and capfd.readouterr().err == ""
        assert plan_of(L, capi, CELL, SF, a_job())[0] == INV  # no tables: refused
        _one_line(capfd, "srsran_hip_pucch_plan", "no tables")
        c, s, job = structs(capi, CELL, SF, a_job())
        grid, res = np.zeros((14, 300), np.complex64), capi.HipPucchRes()
        assert L.srsran_hip_pucch_decode(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, C.byref(res)) == INV  # before the device is looked for
        _one_line(capfd, "srsran_hip_pucch_decode", "no tables")
        for spoil, tag in ((lambda b, m: b.__setitem__((3, 4), 0.5 * b[3, 4]), "modulus"), (lambda b, m: b.__setitem__((3, 4), 1.0), "phi = 0"),
                           (lambda b, m: b.__setitem__((0, 0), np.exp(0.3j)), "off the lattice"), (lambda b, m: b.__setitem__((29, 11), np.nan), "nan"),
                           (lambda b, m: m.__setitem__((12, 19), 2), "basis entry")):
            b, m = base.copy(), basis.copy()
            spoil(b, m)
            assert set_tables(L, b, m) == INV, tag
            _one_line(capfd, "srsran_hip_pucch_set_tables", tag)
            assert plan_of(L, capi, CELL, SF, a_job())[0] == INV  # a refusal leaves the state as it was: unset
            capfd.readouterr()
        assert set_tables(L) == 0
        assert set_tables(L, base[::-1].copy(), basis) == 0  # another well-formed table is taken as it is
        assert set_tables(L, base * np.complex64(1 + 2e-7), basis) == 0  # a few float roundings off is the same table
        assert L.srsran_hip_pucch_set_tables(base.ctypes.data, None) == 0 and plan_of(L, capi, CELL, SF, a_job())[0] == INV  # NULL for either removes both
        capfd.readouterr()
    finally:
        assert set_tables(L) == 0
    assert plan_of(L, capi, CELL, SF, a_job())[0] == 0 and capfd.readouterr().err == ""


# ---- the plan: pure host code
def test_plan_equals_the_record_of_the_reference(L, capfd):
    from srslte_amd import capi

    for c in range(M.n_cases()):
        cell, sf, j, _ = M.case(c)
        rc, w = plan_of(L, capi, cell, sf, j)
        assert rc == 0 and np.array_equal(w, M.plan_words(M.plan(cell, sf, j))), c
        if j["format"] >= M.F2:
            w[37:47] = 0  # n' of formats 2x is not exposed by the reference
        assert np.array_equal(w, M.record()["plan"][c]), c
    assert capfd.readouterr().err == ""


def test_plan_equals_the_reference_over_the_sweep(L, capfd):
    """tests/golden/pucch_sweep_ref.npz holds the reference's OWN plan of every job: six cell sizes, both prefixes, 30 and more cell ids, every subframe"""
    import pucch_sweep as S
    from srslte_amd import capi

    seen = 0
    for g in range(S.n_groups()):
        cell, sf, jobs, _, rows = S.group(g)
        for j, i in zip(jobs, rows):
            rc, w = plan_of(L, capi, cell, sf, j)
            assert rc == 0, (g, j)
            if j["format"] >= M.F2:
                w[37:47] = 0  # n' of formats 2x is not exposed by the reference
            assert np.array_equal(w, S.record()["plan"][i]), (g, j)
            seen += 1
    assert seen == S.record()["job"].shape[0] >= 150 and capfd.readouterr().err == ""


def test_plan_equals_the_model_over_the_reference_tests_sweep(L, capfd):
    from srslte_amd import capi

    seen = refused = 0
    for cell in ({"nof_prb": 50, "cp": 0, "id": 1}, {"nof_prb": 6, "cp": 1, "id": 503}, {"nof_prb": 110, "cp": 0, "id": 299}):
        for fmt in range(6):
            for d in (1, 2, 3):
                for N_cs in range(0, 8, d):
                    for n_pucch in (1, 51, 101):
                        for sf in ({"tti": 3, "shortened": 0}, {"tti": 19, "shortened": 1}):
                            j = a_job(format=fmt, n_pucch=n_pucch, N_cs=N_cs, delta_pucch_shift=d, n_rb_2=2, group_hopping_en=n_pucch == 51, nof_uci_bits=4 if fmt >= M.F2 else 0)
                            want = M.plan(cell, sf, j)
                            rc, w = plan_of(L, capi, cell, sf, j)
                            if want is None:
                                assert rc == capi.SRSRAN_ERROR_INVALID_INPUTS and not w.any(), (cell, j)
                                refused += 1
                            else:
                                assert rc == 0 and np.array_equal(w, M.plan_words(want)), (cell, sf, j)
                            seen += 1
    capfd.readouterr()
    assert seen == 3 * 6 * (8 + 4 + 3) * 3 * 2 and 0 < refused < seen // 2


REFUSED = [("cell", dict(nof_prb=5)), ("cell", dict(nof_prb=111)), ("cell", dict(cp=2)), ("cell", dict(id=504)), ("job", dict(format=6)), ("job", dict(format=7)),
           ("job", dict(delta_pucch_shift=0)), ("job", dict(delta_pucch_shift=4)), ("job", dict(N_cs=8)), ("job", dict(N_cs=3, delta_pucch_shift=2)),
           ("job", dict(n_rb_2=26)), ("job", dict(n_pucch=2048)), ("job", dict(n_pucch=2000)), ("job", dict(format=M.F2, n_pucch=12 * 50, nof_uci_bits=4))]


def _spoiled(what):
    cell, j = dict(CELL), a_job()
    (cell if what[0] == "cell" else j).update(what[1])
    return cell, j


def test_plan_refusals(L, capfd):
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_pucch_plan"
    for what in REFUSED + [("cell", dict(cp=1, fmt2a=1))]:
        cell, j = _spoiled(what)
        if cell.pop("fmt2a", 0):
            j.update(format=M.F2A, nof_uci_bits=4)
        assert M.plan(cell, SF, j) is None, what
        capfd.readouterr()
        rc, w = plan_of(L, capi, cell, SF, j)
        assert rc == INV and not w.any(), what
        _one_line(capfd, who, what)
    c, s, job = structs(capi, CELL, SF, a_job())
    p = capi.HipPucchPlan()
    C.memset(C.byref(p), 0x77, C.sizeof(p))
    assert L.srsran_hip_pucch_plan(None, C.byref(s), C.byref(job), C.byref(p)) == INV and bytes(p) == bytes(C.sizeof(p))
    _one_line(capfd, who, "cell")
    assert L.srsran_hip_pucch_plan(C.byref(c), C.byref(s), C.byref(job), None) == INV
    _one_line(capfd, who, "plan")


# ---- refusals that need no device, and the loud failure without one
SETTINGS = [dict(filter_len=1), dict(filter_len=5), dict(filter=[0.3, float("nan"), 0.3]), dict(format=M.F2, nof_uci_bits=13), dict(rnti=0x10000)]


def test_call_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    grid, ce = np.zeros((14, 300), np.complex64), np.full((14, 300), 5.0, np.complex64)
    for what in REFUSED + [("job", s) for s in SETTINGS]:
        cell, j = _spoiled(what)
        c, s, job = structs(capi, cell, SF, j)
        for who in SYMBOLS[2:]:
            res = (capi.HipPucchRes * 2)()
            C.memset(res, 0x77, C.sizeof(res))
            capfd.readouterr()
            if who.endswith("_multi"):
                jobs = (capi.HipPucchJob * 2)(structs(capi, CELL, SF, a_job())[2], job)  # the second job of two is the bad one
                rc, zeroed = L.srsran_hip_pucch_decode_multi(C.byref(c), C.byref(s), 2, jobs, grid.ctypes.data, res), 2
            elif who.endswith("_dbg"):
                rc, zeroed = L.srsran_hip_pucch_decode_dbg(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, res, C.byref(capi.HipPucchDbg())), 1
            elif who.endswith("_decode"):
                rc, zeroed = L.srsran_hip_pucch_decode(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, res), 1
            else:
                rc, zeroed = L.srsran_hip_chest_ul_estimate_pucch(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, ce.ctypes.data, res), 1
            assert rc == INV and bytes(res)[:64 * zeroed] == bytes(64 * zeroed) and bytes(res)[64 * zeroed:] == b"\x77" * (64 * (2 - zeroed)) and np.all(ce == 5.0), (who, what)
            _one_line(capfd, who, what)
    c, s, job = structs(capi, CELL, SF, a_job())
    res = (capi.HipPucchRes * 2)()
    for who, call in (("srsran_hip_pucch_decode", lambda: L.srsran_hip_pucch_decode(C.byref(c), C.byref(s), C.byref(job), None, res)),
                      ("srsran_hip_pucch_decode", lambda: L.srsran_hip_pucch_decode(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, None)),
                      ("srsran_hip_pucch_decode_dbg", lambda: L.srsran_hip_pucch_decode_dbg(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, res, None)),
                      ("srsran_hip_chest_ul_estimate_pucch", lambda: L.srsran_hip_chest_ul_estimate_pucch(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, None, res)),
                      ("srsran_hip_pucch_decode_multi", lambda: L.srsran_hip_pucch_decode_multi(C.byref(c), C.byref(s), 2, None, grid.ctypes.data, res))):
        capfd.readouterr()
        assert call() == INV, who
        _one_line(capfd, who, "NULL")
    many = (capi.HipPucchRes * 257)()
    C.memset(many, 0x77, C.sizeof(many))
    jobs = (capi.HipPucchJob * 257)(*[job] * 257)
    assert L.srsran_hip_pucch_decode_multi(C.byref(c), C.byref(s), 257, jobs, grid.ctypes.data, many) == INV and bytes(many) == b"\x77" * C.sizeof(many)  # nothing touched
    _one_line(capfd, "srsran_hip_pucch_decode_multi", "n")
    assert L.srsran_hip_pucch_decode_multi(None, None, 0, None, None, None) == 0 and capfd.readouterr().err == ""  # an empty call is a no-op


def test_a_valid_call_without_a_device_fails_loudly(L, capfd):
    from srslte_amd import capi

    c, s, job = structs(capi, CELL, SF, a_job())
    grid, res = np.zeros((14, 300), np.complex64), capi.HipPucchRes()
    capfd.readouterr()
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device (there is no CPU fallback); with one it runs: test_gpu_pucch.py
        assert L.srsran_hip_pucch_decode(C.byref(c), C.byref(s), C.byref(job), grid.ctypes.data, C.byref(res)) == capi.SRSRAN_ERROR and bytes(res) == bytes(64)
        assert "no cpu fallback" in capfd.readouterr().err.lower()
