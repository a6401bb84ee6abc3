"""CPU-only checks of the NR codeword interface (include/srsran_amd/phy_nr_chan_abi.h): the library exports its entry points, a plain C compiler
sees the two structs as the ctypes mirror does, and the seed helper is host arithmetic.  No kernel is launched."""
import ctypes as C
import os
import subprocess

import pytest

import oracle_api as O

ROOT = O.ROOT

SYMBOLS = ["srsran_hip_sequence_nr_seed", "srsran_hip_nr_cw_decode", "srsran_hip_nr_cw_decode_dbg", "srsran_hip_nr_cw_decode_multi",
           "srsran_hip_nr_cw_encode", "srsran_hip_nr_cw_encode_multi"]


@pytest.fixture(scope="module")
def L():
    from srslte_amd import build, capi

    build.build(verbose=False)
    return capi.lib()


def test_library_exports_the_codeword_entry_points(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L._name], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in SYMBOLS if s not in exported]
    for s in SYMBOLS:  # and the mirror has bound them with argument types
        assert getattr(L, s).argtypes is not None, s


def test_struct_layout_matches_ctypes_mirror():
    """sizeof / offsetof of srsran_hip_nr_cw_rx_t and srsran_hip_nr_cw_tx_t as plain gcc sees the header = the ctypes mirror in capi.py"""
    from srslte_amd import capi

    fields = {"rx": ("srsran_hip_nr_cw_rx_t", capi.HipNrCwRx), "tx": ("srsran_hip_nr_cw_tx_t", capi.HipNrCwTx)}
    src = '#include "srsran_amd/phy_nr_chan_abi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
    for tag, (ctype, mirror) in fields.items():
        src += '  printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (tag, ctype)
        for name, _ in mirror._fields_:
            src += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (tag, name, ctype, name)
    src += '  printf("tb.sizeof %zu\\n", sizeof(srsran_hip_nr_tb_t));\n  printf("res.sizeof %zu\\n", sizeof(srsran_hip_nr_tb_result_t));\n  return 0; }\n'
    d = os.path.join(ROOT, "build", "scratch")
    os.makedirs(d, exist_ok=True)
    cfile, exe = os.path.join(d, "nr_cw_layout.c"), os.path.join(d, "nr_cw_layout")
    open(cfile, "w").write(src)
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())}
    for tag, (_, mirror) in fields.items():
        assert got[tag + ".sizeof"] == C.sizeof(mirror), tag
        for name, _ in mirror._fields_:
            assert got["%s.%s" % (tag, name)] == getattr(mirror, name).offset, (tag, name)
    assert got["tb.sizeof"] == C.sizeof(capi.HipNrTb) and got["res.sizeof"] == C.sizeof(capi.HipNrTbResult)


def test_seed_is_the_closed_form_without_a_device(L):
    """pdsch_nr_cinit (pdsch_nr.c:290-302) = pusch_nr_cinit (pusch_nr.c:339-351) = (rnti << 15) + (cw_idx << 14) + n_id"""
    for rnti, cw, n_id in [(0, 0, 0), (1, 0, 0), (0x1234, 0, 500), (0x1234, 1, 500), (0xFFFF, 1, 1023), (17, 1, 1007), (0x4601, 0, 65535)]:
        assert L.srsran_hip_sequence_nr_seed(rnti, cw, n_id) == ((rnti << 15) + (cw << 14) + n_id) & 0xFFFFFFFF, (rnti, cw, n_id)


def test_refusals_need_no_device(L):
    """argument checks come before the device is looked for: an invalid codeword is SRSRAN_ERROR_INVALID_INPUTS with or without a GPU, and a valid one
    without a GPU fails loudly (there is no CPU fallback)"""
    import numpy as np

    from srslte_amd import capi

    rows = [np.zeros(50 * 7 + 8, np.int8)]
    keep = [np.zeros(64, np.uint8)]
    flags = np.zeros(1, np.bool_)
    sb = capi.SoftbufferRx(1, 50 * 7, (C.c_void_p * 1)(rows[0].ctypes.data), (C.c_void_p * 1)(keep[0].ctypes.data), flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
    x = np.zeros(24, np.complex64)
    out = np.full(8, 0xEE, np.uint8)
    res = capi.HipNrTbResult(7, 7, 7.0, 7)
    g = capi.HipNrCwRx(capi.HipNrTb(0.5, 24, 1, 0x100, 1, 48, 0, 0, 0, 0, 0), 24, 1, 0.8, 6, 0.0, 0)
    bad = capi.HipNrCwRx(capi.HipNrTb(0.5, 24, 1, 0x100, 1, 50, 0, 0, 0, 0, 0), 24, 1, 0.8, 6, 0.0, 0)  # nof_bits != nof_re * Qm
    assert L.srsran_hip_nr_cw_decode(C.byref(bad), O.P(x), None, C.byref(sb), O.P(out), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS
    assert (res.crc_ok, res.all_decoded, res.avg_iter, res.nof_cb) == (0, 0, 0.0, 0) and np.all(out == 0xEE)
    assert L.srsran_hip_nr_cw_decode(C.byref(g), None, None, C.byref(sb), O.P(out), C.byref(res)) == capi.SRSRAN_ERROR_INVALID_INPUTS
    t = capi.HipNrCwTx(capi.HipNrTb(0.5, 24, 5, 0, 1, 48, 0, 0, 0, 0, 0), 24, 1, 1.0, 0)  # modulation outside QPSK .. 256-QAM
    assert L.srsran_hip_nr_cw_encode(C.byref(t), O.P(out), O.P(x)) == capi.SRSRAN_ERROR_INVALID_INPUTS
    if L.srsran_hip_device_count() == 0:
        assert L.srsran_hip_nr_cw_decode(C.byref(g), O.P(x), None, C.byref(sb), O.P(out), C.byref(res)) == capi.SRSRAN_ERROR
        assert np.all(out == 0xEE) and not flags[0]
