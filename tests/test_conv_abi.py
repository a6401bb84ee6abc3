"""CPU-only checks of the convolutional-code entry points (include/srsran_amd/phy_conv_abi.h), in the manner of test_nr_chest_abi.py: the library exports them
and the ctypes mirror binds them, the header compiles for plain C, srsran_viterbi_t has the reference's layout (96 bytes; against the reference's own header
where the tree is present), the mirror's structs have the header's layout, every refusal comes before the device is looked for with one line on stderr and the
results zeroed, and a valid call without a device fails loudly.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_api as O

ROOT = O.ROOT
REF_INCLUDE = "/root/reference/lib/include"
SYMBOLS = ["srsran_viterbi_init", "srsran_viterbi_free", "srsran_viterbi_set_gain_quant", "srsran_viterbi_set_gain_quant_s", "srsran_viterbi_decode_f",
           "srsran_viterbi_decode_s", "srsran_viterbi_decode_us", "srsran_viterbi_decode_uc", "srsran_hip_viterbi_decode_us_multi",
           "srsran_hip_pdcch_dci_decode_multi", "srsran_hip_pdcch_dci_decode_multi_dbg"]
VFIELDS = ["ptr", "R", "K", "framebits", "tail_biting", "gain_quant", "gain_quant_s", "decode", "decode_s", "decode_f", "free", "tmp", "tmp_s", "symbols_uc",
           "symbols_us"]
VOFFSETS = [0, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def _compile_run(name, src, include, link=False):
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, name + ".c"), os.path.join(d, name)
    open(cfile, "w").write(src)
    libdir = os.path.join(ROOT, "srslte_amd", "lib")
    extra = ["-L", libdir, "-lsrsran_phy_hip", "-Wl,-rpath," + libdir] if link else []
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", include, cfile, "-o", exe] + extra)
    return subprocess.check_output([exe], text=True)


def _layout_program(header):
    items = ["sizeof(srsran_viterbi_t)"] + ["offsetof(srsran_viterbi_t, %s)" % f for f in VFIELDS]
    return ('#include <stdint.h>\n#include "%s"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' % header + "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) +
            "  return 0; }\n")


def test_library_exports_the_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def test_viterbi_handle_has_the_reference_layout():
    from srslte_amd import capi

    got = [int(v) for v in _compile_run("conv_layout", _layout_program("srsran_amd/phy_conv_abi.h"), os.path.join(ROOT, "include")).split()]
    assert got == [96] + VOFFSETS
    assert [C.sizeof(capi.Viterbi)] + [getattr(capi.Viterbi, f).offset for f in VFIELDS] == got
    if os.path.isdir(REF_INCLUDE):  # the reference's own header says the same
        ref = [int(v) for v in _compile_run("conv_layout_ref", _layout_program("srsran/phy/fec/convolutional/viterbi.h"), REF_INCLUDE).split()]
        assert ref == got


def test_mirror_has_the_header_layout():
    from srslte_amd import capi

    cf, rf = ["ncce", "L", "nof_bits"], ["payload", "crc_rem", "decoded", "mean"]
    items = (["sizeof(srsran_hip_pdcch_cand_t)"] + ["offsetof(srsran_hip_pdcch_cand_t, %s)" % f for f in cf] + ["sizeof(srsran_hip_pdcch_res_t)"] +
             ["offsetof(srsran_hip_pdcch_res_t, %s)" % f for f in rf] + ["SRSRAN_VITERBI_37", "SRSRAN_HIP_DCI_MAX_BITS + 16", "SRSRAN_HIP_PDCCH_MAX_CANDIDATES",
                                                                         "SRSRAN_HIP_VITERBI_MAX_FRAMEBITS"])
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' +
           "".join('  printf("%%zu ", (size_t)%s);\n' % it for it in items) + "  return 0; }\n")
    got = [int(v) for v in _compile_run("conv_mirror", src, os.path.join(ROOT, "include")).split()]
    want = ([C.sizeof(capi.HipPdcchCand)] + [getattr(capi.HipPdcchCand, f).offset for f in cf] + [C.sizeof(capi.HipPdcchRes)] +
            [getattr(capi.HipPdcchRes, f).offset for f in rf] + [capi.SRSRAN_VITERBI_37, capi.HIP_DCI_ROW, 256, 2048])
    assert got == want
    assert (C.sizeof(capi.HipPdcchCand), C.sizeof(capi.HipPdcchRes), capi.HIP_DCI_SYMS) == (12, 152, 432)


def test_header_declares_them_for_plain_c():
    """a C caller of every entry point compiles under -Wall -Werror and links (not run)"""
    src = ('#include "srsran_amd/phy_conv_abi.h"\n#include <stddef.h>\n'
           "int take(srsran_viterbi_t* q, float* f, int16_t* s, uint16_t* us, uint8_t* uc, uint8_t* data, const srsran_hip_pdcch_cand_t* cand,\n"
           "         srsran_hip_pdcch_res_t* res) {\n"
           "  int poly[3] = {0x6D, 0x4F, 0x57}; const uint16_t* syms[1] = {us}; uint8_t* datas[1] = {data}; uint32_t len[1] = {40};\n"
           "  int rc = srsran_viterbi_init(q, SRSRAN_VITERBI_37, poly, 40, true);\n"
           "  srsran_viterbi_set_gain_quant(q, 32.0f); srsran_viterbi_set_gain_quant_s(q, 4);\n"
           "  rc += srsran_viterbi_decode_f(q, f, data, 40) + srsran_viterbi_decode_s(q, s, data, 40) + srsran_viterbi_decode_us(q, us, data, 40) +\n"
           "        srsran_viterbi_decode_uc(q, uc, data, 40) + srsran_hip_viterbi_decode_us_multi(q, 1, syms, datas, len) +\n"
           "        srsran_hip_pdcch_dci_decode_multi(f, 72, 1, cand, res) + srsran_hip_pdcch_dci_decode_multi_dbg(f, 72, 1, cand, res, f, us);\n"
           "  srsran_viterbi_free(q);\n  return rc; }\n"
           "int main(int argc, char** argv) { return argc > 7 ? take(0, 0, 0, 0, 0, 0, 0, 0) : 0; }\n")
    assert _compile_run("conv_abi", src, os.path.join(ROOT, "include"), link=True) == ""


# ---- the handle
def _handle(L, capi, framebits=40, tb=True, type_=None, poly=(0x6D, 0x4F, 0x57)):
    q = capi.Viterbi()
    rc = L.srsran_viterbi_init(C.byref(q), capi.SRSRAN_VITERBI_37 if type_ is None else type_, (C.c_int * 3)(*poly), framebits, tb)
    return q, rc


def _one_line(capfd, who, tag):
    err = capfd.readouterr().err
    assert len(err.strip().splitlines()) == 1 and who in err, (tag, err)
    assert not any(w in err.lower() for w in ("hip error", "device", "illegal", "fault")), (tag, err)


def test_init_fills_the_handle_as_the_reference_does(L, capfd):
    from srslte_amd import capi

    q, rc = _handle(L, capi, 144, True)
    assert rc == 0 and (q.K, q.R, q.framebits, q.tail_biting, q.gain_quant, q.gain_quant_s) == (7, 3, 144, True, 1000.0, 4) and q.ptr
    L.srsran_viterbi_set_gain_quant(C.byref(q), 32.5)
    L.srsran_viterbi_set_gain_quant_s(C.byref(q), 7)
    assert (q.gain_quant, q.gain_quant_s) == (32.5, 7)
    L.srsran_viterbi_free(C.byref(q))
    assert bytes(q) == bytes(96)
    assert _handle(L, capi, 2048, False)[1] == 0
    assert capfd.readouterr().err == ""
    for kw, tag in [(dict(framebits=2049), "max_frame_length"), (dict(framebits=0), "max_frame_length"), (dict(type_=0), "not implemented"),
                    (dict(type_=3), "not implemented"), (dict(poly=(0x6D, 0x4F, 0x5F)), "polynomials")]:
        q, rc = _handle(L, capi, **kw)
        assert rc == -1 and bytes(q) == bytes(96), kw
        _one_line(capfd, tag, kw)


def test_handle_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    q, _ = _handle(L, capi, 40, True)
    f, s, us = np.ones(3 * 64, np.float32), np.ones(3 * 64, np.int16), np.ones(3 * 64, np.uint16)
    data = np.full(80, 0xEE, np.uint8)
    calls = [("srsran_viterbi_decode_f", f), ("srsran_viterbi_decode_s", s), ("srsran_viterbi_decode_us", us)]
    for name, x in calls:
        fn = getattr(L, name)
        capfd.readouterr()
        assert fn(C.byref(q), x.ctypes.data, data.ctypes.data, 41) == -1 and np.all(data == 0xEE)  # longer than the handle was made for: the reference's -1
        _one_line(capfd, "max frame length 40", name)
        assert fn(C.byref(q), x.ctypes.data, data.ctypes.data, 0) == -1
        _one_line(capfd, name, "zero length")
        assert fn(C.byref(q), None, data.ctypes.data, 40) == capi.SRSRAN_ERROR and fn(C.byref(q), x.ctypes.data, None, 40) == capi.SRSRAN_ERROR
        capfd.readouterr()
        blank = capi.Viterbi()
        assert fn(C.byref(blank), x.ctypes.data, data.ctypes.data, 40) == capi.SRSRAN_ERROR and np.all(data == 0xEE)
        _one_line(capfd, name, "blank handle")
    assert L.srsran_viterbi_decode_uc(C.byref(q), data.ctypes.data, data.ctypes.data, 40) == capi.SRSRAN_ERROR  # the 16-bit object has no 8-bit function
    # the multi call
    syms, datas = (C.c_void_p * 2)(us.ctypes.data, us.ctypes.data), (C.c_void_p * 2)(data.ctypes.data, data.ctypes.data + 40)
    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    capfd.readouterr()
    assert L.srsran_hip_viterbi_decode_us_multi(C.byref(q), 0, None, None, None) == 40 and capfd.readouterr().err == ""  # an empty call is a no-op
    bad = [(2, syms, datas, (C.c_uint32 * 2)(40, 41)), (2, syms, datas, (C.c_uint32 * 2)(0, 40)), (2, None, datas, (C.c_uint32 * 2)(40, 40)),
           (2, syms, None, (C.c_uint32 * 2)(40, 40)), (2, syms, datas, None), (2, (C.c_void_p * 2)(us.ctypes.data, None), datas, (C.c_uint32 * 2)(40, 40)),
           (257, syms, datas, (C.c_uint32 * 2)(40, 40))]
    for n, a, b, c in bad:
        assert L.srsran_hip_viterbi_decode_us_multi(C.byref(q), n, a, b, c) == INV and np.all(data == 0xEE)
        _one_line(capfd, "viterbi_decode_us_multi", n)
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly (there is no CPU fallback)
        for name, x in calls:
            capfd.readouterr()
            assert getattr(L, name)(C.byref(q), x.ctypes.data, data.ctypes.data, 40) == capi.SRSRAN_ERROR and np.all(data == 0xEE)
            assert "no cpu fallback" in capfd.readouterr().err.lower()
        assert L.srsran_hip_viterbi_decode_us_multi(C.byref(q), 2, syms, datas, (C.c_uint32 * 2)(40, 40)) == capi.SRSRAN_ERROR and np.all(data == 0xEE)
        assert "no cpu fallback" in capfd.readouterr().err.lower()


# ---- the PDCCH call
class _Pdcch:
    """three valid candidates on a 6-CCE region, with sentinels everywhere a call could write"""

    def __init__(self, capi, n=3):
        self.llr = np.full(6 * 72, 1.5, np.float32)
        self.nof_llr = self.llr.size
        self.cand = (capi.HipPdcchCand * max(n, 1))(*[capi.HipPdcchCand(i, i % 3, 27 + i) for i in range(max(n, 1))][:max(n, 1)])
        self.res = (capi.HipPdcchRes * max(n, 1))()
        for r in self.res:
            C.memset(C.byref(r), 0x77, C.sizeof(r))
        self.rm = np.full(max(n, 1) * 432 + 8, 5.0, np.float32)
        self.sym = np.full(max(n, 1) * 432 + 8, 5, np.uint16)
        self.n = n

    def zeroed(self, n=None):
        return bytes(self.res)[:(self.n if n is None else n) * 152] == bytes((self.n if n is None else n) * 152)

    def dbg_untouched(self):
        return np.all(self.rm == 5.0) and np.all(self.sym == 5)


def test_pdcch_refusals_need_no_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS

    def call(k, dbg, llr=True, cand=True, res=True, n=None):
        args = [k.llr.ctypes.data if llr else None, k.nof_llr, k.n if n is None else n, k.cand if cand else None, k.res if res else None]
        if dbg:
            return L.srsran_hip_pdcch_dci_decode_multi_dbg(*(args + [k.rm.ctypes.data, k.sym.ctypes.data]))
        return L.srsran_hip_pdcch_dci_decode_multi(*args)

    def spoil(k, what):
        if what == "L":
            k.cand[1].L = 4
        elif what == "past the end":
            k.cand[2].ncce = 3  # 3 * 72 + (72 << 2) > 6 * 72
        elif what == "past the end, by one":
            k.nof_llr -= 1
            k.cand[2].ncce = 2
        elif what == "nof_bits 0":
            k.cand[0].nof_bits = 0
        elif what == "nof_bits 129":
            k.cand[2].nof_bits = 129
        elif what == "ncce wraps":
            k.cand[1].ncce = 0xFFFFFFFF // 72 + 1

    for dbg in (False, True):
        for what in ("L", "past the end", "past the end, by one", "nof_bits 0", "nof_bits 129", "ncce wraps"):
            k = _Pdcch(capi)
            spoil(k, what)
            capfd.readouterr()
            assert call(k, dbg) == INV and k.zeroed() and k.dbg_untouched(), (dbg, what)
            _one_line(capfd, "pdcch_dci_decode_multi", (dbg, what))
        for null in ("llr", "cand"):
            k = _Pdcch(capi)
            capfd.readouterr()
            assert call(k, dbg, **{null: False}) == INV and k.dbg_untouched(), (dbg, null)
            _one_line(capfd, "pdcch_dci_decode_multi", (dbg, null))
        k = _Pdcch(capi)
        capfd.readouterr()
        assert call(k, dbg, res=False) == INV
        _one_line(capfd, "pdcch_dci_decode_multi", (dbg, "res"))
        assert call(k, dbg, n=257) == INV and k.dbg_untouched()
        _one_line(capfd, "pdcch_dci_decode_multi", (dbg, "n"))
        assert call(k, dbg, llr=False, cand=False, res=False, n=0) == 0 and capfd.readouterr().err == ""  # an empty search is a no-op
    # below the mean rule nothing is decoded and the device is not looked for: decoded 0, payload and crc_rem 0, the mean reported
    k = _Pdcch(capi)
    k.llr[:] = 0.25
    capfd.readouterr()
    assert call(k, True) == 0 and capfd.readouterr().err == ""
    assert all((r.decoded, r.crc_rem, r.mean, bytes(r.payload)) == (0, 0, 0.25, bytes(144)) for r in k.res)
    assert np.all(k.rm[:3 * 432] == 0) and np.all(k.sym[:3 * 432] == 0) and np.all(k.rm[3 * 432:] == 5.0) and np.all(k.sym[3 * 432:] == 5)
    if L.srsran_hip_device_count() == 0:  # a valid call gets as far as looking for the device and fails loudly
        for dbg in (False, True):
            k = _Pdcch(capi)
            capfd.readouterr()
            assert call(k, dbg) == capi.SRSRAN_ERROR and k.zeroed()
            assert "no cpu fallback" in capfd.readouterr().err.lower()
