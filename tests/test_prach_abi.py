"""CPU-only checks of the PRACH entry points (include/srsran_amd/phy_prach_abi.h), in the manner of test_ctrl_abi.py: the library exports them and the ctypes
mirror binds them, the structs have the declared sizes in the header and in the mirror, a plain C caller compiles under -Wall -Werror, srsran_hip_prach_plan
(pure host code) equals the record of the reference and tests/prach_model.py over all 16 zones, the restricted set and a sweep of root_seq_idx, every refusal
that needs no handle comes before the device is looked for with one line on stderr and nothing written but zeroed results, and a valid create without a device
fails loudly.  The refusals of the detection calls that need a handle (a handle needs a device) are in test_gpu_prach.py.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O
import prach_model as M
from test_conv_abi import _compile_run, _one_line
from test_prach_golden import INFO, case, names

ROOT = O.ROOT
SYMBOLS = ["srsran_hip_prach_set_root_order", "srsran_hip_prach_plan", "srsran_hip_prach_create", "srsran_hip_prach_destroy", "srsran_hip_prach_info", "srsran_hip_prach_root_spectrum",
           "srsran_hip_prach_detect_offset", "srsran_hip_prach_detect_offset_dbg", "srsran_hip_prach_detect_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    lib = capi.lib()
    assert set_order(lib) == 0
    return lib


def set_order(lib, order=None):
    """hand the recorded root order (or another table, or None) to the library"""
    o = np.ascontiguousarray(M.root_order() if order is None else order, np.uint32)
    return lib.srsran_hip_prach_set_root_order(o.ctypes.data)


def cfg_struct(capi, cfg, detect_factor=0.0):
    return capi.HipPrachCfg(*[cfg[k] for k in M.CFG_FIELDS], detect_factor)


def plan_of(L, capi, cfg):
    info = capi.HipPrachInfo()
    rc = L.srsran_hip_prach_plan(C.byref(cfg_struct(capi, cfg)), C.byref(info))
    return rc, info


def same_plan(info, p):
    return ({k: getattr(info, k) for k in INFO} == {k: p[k] for k in INFO} and list(info.root_seqs_idx)[:p["N_roots"]] == p["root_seqs_idx"] and
            list(info.root_u)[:p["N_roots"]] == p["root_u"] and not any(list(info.root_seqs_idx)[p["N_roots"]:]) and not any(list(info.root_u)[p["N_roots"]:]))


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_struct_sizes_in_header_and_mirror():
    from srslte_amd import capi

    items = ["sizeof(srsran_hip_prach_cfg_t)", "sizeof(srsran_hip_prach_info_t)", "sizeof(srsran_hip_prach_occ_t)", "sizeof(srsran_hip_prach_res_t)",
             "sizeof(srsran_hip_prach_dbg_t)", "offsetof(srsran_hip_prach_cfg_t, detect_factor)", "offsetof(srsran_hip_prach_info_t, root_seqs_idx)",
             "offsetof(srsran_hip_prach_info_t, root_u)", "offsetof(srsran_hip_prach_occ_t, signal)", "offsetof(srsran_hip_prach_res_t, t_offsets)",
             "offsetof(srsran_hip_prach_res_t, peak_to_avg)", "offsetof(srsran_hip_prach_dbg_t, peak_offsets)", "SRSRAN_HIP_PRACH_MAX_OCC", "SRSRAN_HIP_PRACH_MAX_DET"]
    src = ('#include "srsran_amd/phy_prach_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("prach_layout", src, os.path.join(ROOT, "include")).split()]
    assert got == [32, 548, 16, 1540, 48, 28, 36, 292, 8, 516, 1028, 40, 8, 128]
    assert [C.sizeof(capi.HipPrachCfg), C.sizeof(capi.HipPrachInfo), C.sizeof(capi.HipPrachOcc), C.sizeof(capi.HipPrachRes), C.sizeof(capi.HipPrachDbg),
            capi.HipPrachCfg.detect_factor.offset, capi.HipPrachInfo.root_seqs_idx.offset, capi.HipPrachInfo.root_u.offset, capi.HipPrachOcc.signal.offset,
            capi.HipPrachRes.t_offsets.offset, capi.HipPrachRes.peak_to_avg.offset, capi.HipPrachDbg.peak_offsets.offset] == got[:-2]


def test_header_takes_a_plain_c_callers_arrays():
    """a C caller that holds what a caller of srsran_prach_detect_offset holds compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_prach_abi.h"\n#include <stddef.h>\n'
           "int take(const srsran_hip_prach_cfg_t* cfg, cf_t* signal, const srsran_hip_prach_occ_t* occ, srsran_hip_prach_res_t* res) {\n"
           "  srsran_hip_prach_t* h = NULL; srsran_hip_prach_info_t info; uint32_t indices[64], n = 0; float t_offsets[64], peak_to_avg[64];\n"
           "  cf_t spec[SRSRAN_HIP_PRACH_N_ZC]; srsran_hip_prach_dbg_t dbg = {spec, NULL, NULL, NULL, NULL, NULL};\n"
           "  int rc = srsran_hip_prach_plan(cfg, &info) + srsran_hip_prach_create(&h, cfg) + srsran_hip_prach_info(h, &info);\n"
           "  rc += srsran_hip_prach_root_spectrum(h, 0, spec);\n"
           "  rc += srsran_hip_prach_detect_offset(h, 0, signal, info.N_ifft_prach, indices, t_offsets, peak_to_avg, 64, &n);\n"
           "  rc += srsran_hip_prach_detect_offset_dbg(h, 0, signal, info.N_ifft_prach, indices, NULL, NULL, 64, &n, &dbg);\n"
           "  rc += srsran_hip_prach_detect_multi(h, 2, occ, res);\n"
           "  srsran_hip_prach_destroy(h);\n"
           "  return rc + (int)res[0].n_indices; }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0) : 0; }\n")
    assert _compile_run("prach_abi", src, os.path.join(ROOT, "include"), link=True) == ""


# ---- the plan: pure host code
def test_plan_equals_the_record_of_the_reference(L):
    from srslte_amd import capi

    for c, name in enumerate(names()):
        g = case(c)
        L.srsran_use_standard_symbol_size(bool(g["standard"]))
        try:
            rc, info = plan_of(L, capi, g["cfg_dict"])
        finally:
            L.srsran_use_standard_symbol_size(False)
        assert rc == 0 and {k: getattr(info, k) for k in INFO} == g["info_dict"], name
        n = g["info_dict"]["N_roots"]
        assert list(info.root_seqs_idx)[:n] == g["root_seqs_idx"] and list(info.root_u)[:n] == [int(u) for u in g["root_u"]], name


def test_plan_equals_the_model_over_zones_roots_and_cells(L, capfd):
    from srslte_amd import capi

    seen = 0
    for hs in (0, 1):
        for zcz in range(15 if hs else 16):
            for rsi in (0, 1, 22, 137, 419, 500, 777, 836, 837):  # 836, 837: the used roots wrap around the table
                cfg = dict(zip(M.CFG_FIELDS, (6, 0, rsi, zcz, 0, hs, 0)))
                rc, info = plan_of(L, capi, cfg)
                assert rc == 0 and same_plan(info, M.plan(cfg)), cfg
                seen += 1
    for nof_prb in M.SYMBOL_SZ:
        for config_idx, nra in ((0, 0), (15, 3), (16, 4), (35, 5), (63, 64), (40, 65)):
            cfg = dict(zip(M.CFG_FIELDS, (nof_prb, config_idx, 300, 0, nra, 0, 1)))
            rc, info = plan_of(L, capi, cfg)
            assert rc == 0 and same_plan(info, M.plan(cfg)) and info.N_ifft_prach == 12 * M.SYMBOL_SZ[nof_prb], cfg
    assert seen == 9 * 31 and capfd.readouterr().err == ""


REFUSED = [("nof_prb", 0), ("nof_prb", 7), ("nof_prb", 110), ("config_idx", 64), ("config_idx", 80), ("root_seq_idx", 838), ("zero_corr_zone", 16),
           ("hs zone", 15)]


def _spoiled(what):
    cfg = dict(zip(M.CFG_FIELDS, (25, 3, 10, 5, 0, 0, 0)))
    if what[0] == "hs zone":
        cfg.update(hs_flag=1, zero_corr_zone=what[1])
    else:
        cfg[what[0]] = what[1]
    return cfg


def test_plan_refusals(L, capfd):
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_prach_plan"
    for what in REFUSED:
        assert M.plan(_spoiled(what)) is None, what
        info = capi.HipPrachInfo()
        C.memset(C.byref(info), 0x77, C.sizeof(info))
        capfd.readouterr()
        assert L.srsran_hip_prach_plan(C.byref(cfg_struct(capi, _spoiled(what))), C.byref(info)) == INV and bytes(info) == bytes(C.sizeof(info)), what
        _one_line(capfd, who, what)
    info = capi.HipPrachInfo()
    C.memset(C.byref(info), 0x77, C.sizeof(info))
    assert L.srsran_hip_prach_plan(None, C.byref(info)) == INV and bytes(info) == bytes(C.sizeof(info))
    _one_line(capfd, who, "cfg")
    assert L.srsran_hip_prach_plan(C.byref(cfg_struct(capi, _spoiled(("config_idx", 3)))), None) == INV
    _one_line(capfd, who, "info")


def test_root_order_is_the_callers(L, capfd):
    from srslte_amd import capi

    INV, cfg = capi.SRSRAN_ERROR_INVALID_INPUTS, _spoiled(("config_idx", 3))
    try:
        assert L.srsran_hip_prach_set_root_order(None) == 0 and capfd.readouterr().err == ""
        for who, call in (("srsran_hip_prach_plan", lambda: plan_of(L, capi, cfg)[0]),
                          ("srsran_hip_prach_create", lambda: L.srsran_hip_prach_create(C.byref(C.c_void_p()), C.byref(cfg_struct(capi, cfg))))):
            assert call() == INV  # no table: refused before the device is looked for
            _one_line(capfd, who, "no table")
        bad = M.root_order().copy()
        bad[5] = bad[6]
        assert set_order(L, bad) == INV
        _one_line(capfd, "srsran_hip_prach_set_root_order", "not a permutation")
        bad[5] = 839
        assert set_order(L, bad) == INV and plan_of(L, capi, cfg)[0] == INV
        capfd.readouterr()
        other = M.root_order()[::-1].copy()  # another permutation is taken as it is: the table is the caller's
        assert set_order(L, other) == 0
        rc, info = plan_of(L, capi, dict(cfg, root_seq_idx=0))
        assert rc == 0 and info.root_u[0] == other[0]
    finally:
        assert set_order(L) == 0
    rc, info = plan_of(L, capi, dict(cfg, root_seq_idx=0))
    assert rc == 0 and info.root_u[0] == M.root_order()[0] and capfd.readouterr().err == ""


# ---- refusals that need no handle, and the loud failure without a device
def test_create_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV, who = capi.SRSRAN_ERROR_INVALID_INPUTS, "srsran_hip_prach_create"
    for what in REFUSED:
        h = C.c_void_p(0x7777)
        capfd.readouterr()
        assert L.srsran_hip_prach_create(C.byref(h), C.byref(cfg_struct(capi, _spoiled(what)))) == INV and not h.value, what
        _one_line(capfd, who, what)
    h = C.c_void_p(0x7777)
    assert L.srsran_hip_prach_create(C.byref(h), None) == INV and not h.value
    _one_line(capfd, who, "cfg")
    assert L.srsran_hip_prach_create(None, C.byref(cfg_struct(capi, _spoiled(("config_idx", 3))))) == INV
    _one_line(capfd, who, "h")
    if L.srsran_hip_device_count() == 0:  # a valid create gets as far as looking for the device and fails loudly (there is no CPU fallback)
        h = C.c_void_p(0x7777)
        capfd.readouterr()
        assert L.srsran_hip_prach_create(C.byref(h), C.byref(cfg_struct(capi, _spoiled(("config_idx", 3))))) == capi.SRSRAN_ERROR and not h.value
        assert "no cpu fallback" in capfd.readouterr().err.lower()


def test_calls_without_a_handle_are_refused(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    sig = np.ones(1536, np.complex64)
    ind, toff, p2a = np.full(8, 0x77777777, np.uint32), np.full(8, 5.0, np.float32), np.full(8, 5.0, np.float32)
    for dbg in (False, True):
        who = "srsran_hip_prach_detect_offset_dbg" if dbg else "srsran_hip_prach_detect_offset"
        n = C.c_uint32(0x77777777)
        a = [None, 0, sig.ctypes.data, sig.size, ind.ctypes.data, toff.ctypes.data, p2a.ctypes.data, 8, C.byref(n)]
        capfd.readouterr()
        rc = L.srsran_hip_prach_detect_offset_dbg(*(a + [C.byref(capi.HipPrachDbg())])) if dbg else L.srsran_hip_prach_detect_offset(*a)
        assert rc == INV and n.value == 0 and np.all(ind == 0x77777777) and np.all(toff == 5.0) and np.all(p2a == 5.0), dbg
        _one_line(capfd, who, dbg)
    who = "srsran_hip_prach_detect_multi"
    occ = (capi.HipPrachOcc * 9)(*[capi.HipPrachOcc(0, sig.size, sig.ctypes.data) for _ in range(9)])
    res = (capi.HipPrachRes * 9)()
    C.memset(res, 0x77, C.sizeof(res))
    capfd.readouterr()
    assert L.srsran_hip_prach_detect_multi(None, 2, occ, res) == INV and bytes(res)[:2 * 1540] == bytes(2 * 1540) and bytes(res)[2 * 1540:] == b"\x77" * (7 * 1540)
    _one_line(capfd, who, "h")
    C.memset(res, 0x77, C.sizeof(res))
    assert L.srsran_hip_prach_detect_multi(None, 9, occ, res) == INV and bytes(res) == b"\x77" * (9 * 1540)  # n > 8: nothing is touched
    _one_line(capfd, who, "n")
    assert L.srsran_hip_prach_detect_multi(None, 0, None, None) == 0 and capfd.readouterr().err == ""  # an empty call is a no-op
    spec = np.full(839, 5.0, np.complex64)
    assert L.srsran_hip_prach_root_spectrum(None, 0, spec.ctypes.data) == INV and np.all(spec == 5.0)
    _one_line(capfd, "srsran_hip_prach_root_spectrum", "h")
    assert L.srsran_hip_prach_info(None, C.byref(capi.HipPrachInfo())) == INV
    _one_line(capfd, "srsran_hip_prach_info", "h")
    L.srsran_hip_prach_destroy(None)
    assert capfd.readouterr().err == ""
