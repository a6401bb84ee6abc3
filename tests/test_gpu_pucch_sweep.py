"""PUCCH receive on the device held to the second record of the reference, tests/golden/pucch_sweep_ref.npz (tests/pucch_sweep.py, tools/gen_golden_pucch_sweep.py):
per GROUP -- one cell, one subframe, two or three users summed on one PRB beside empty resources, 6 to 100 PRB, both prefixes, every subframe -- all jobs in
ONE srsran_hip_pucch_decode_multi call on the group's grid.  Decisions, bits and DRS bits EXACT against the reference, floats within the tolerances the
generator measured on these jobs; every job again through the _dbg call: the same result bytes, the 20 soft bits exact, ce against the record, z and the
pilot estimates against the float64 model on the same grid (the record does not hold them; the generator held the model to the reference there).  The
group call twice and with the job list reversed: the same bytes per job.  A handful of device calls per group."""
import ctypes as C

import numpy as np
import pytest

import pucch_model as M
import pucch_sweep as S
from test_gpu_pucch import SENTINEL, as_dict, multi
from test_pucch_abi import set_tables, structs
from test_pucch_golden import check_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0 and set_tables(lib) == 0
    return lib


def tol(name):
    return S.tolerances()[name]


@pytest.mark.parametrize("g", range(S.n_groups()))
def test_every_group_in_one_call(L, g, capfd):
    from srslte_amd import capi

    cell, sf, jobs, grid, rows = S.group(g)
    before, n = grid.copy(), len(jobs)
    got = multi(L, cell, sf, jobs, grid)
    assert len(got) == 64 * n and multi(L, cell, sf, jobs, grid) == got  # a second run gives the same bytes
    back = multi(L, cell, sf, jobs[::-1], grid)
    assert [back[64 * (n - 1 - k):64 * (n - k)] for k in range(n)] == [got[64 * k:64 * k + 64] for k in range(n)]  # a job's result does not depend on its place
    for k, (j, i) in enumerate(zip(jobs, rows)):
        name, e, p = "group %d job %d" % (g, k), S.entry(i), M.plan(cell, sf, j)
        check_record(e, j, p, as_dict(capi.HipPucchRes.from_buffer_copy(got[64 * k:64 * k + 64])), name, tol, arrays=False)
        # the _dbg call: the same bytes, and the arrays
        cs, ss, js = structs(capi, cell, sf, j)
        z, llr, ce, pe = np.full(120, SENTINEL, np.complex64), np.full(20, 77, np.int16), np.full((2, 12), SENTINEL, np.complex64), np.full((6, 12), SENTINEL, np.complex64)
        res, dbg = capi.HipPucchRes(), capi.HipPucchDbg(z.ctypes.data, llr.ctypes.data, ce.ctypes.data, pe.ctypes.data)
        assert L.srsran_hip_pucch_decode_dbg(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, C.byref(res), C.byref(dbg)) == 0
        assert bytes(res) == got[64 * k:64 * k + 64], name
        d = as_dict(res)
        d.update(llr=llr, ce=ce)
        check_record(e, j, p, d, name, tol)  # llr exact, ce within its tolerance
        m = M.decode(grid, cell, sf, j, p)
        n_rs, nof_re = int(p["n_rs"]), 12 * int(p["N_sf"].sum())
        assert np.max(np.abs(pe[:2 * n_rs].astype(np.complex128) - m["pe"])) <= tol("pe") * np.max(np.abs(m["pe"])), name
        assert np.all(pe[2 * n_rs:] == SENTINEL) and np.all(z[nof_re:] == 0), name
        zm = m["z"].reshape(-1).astype(np.complex128)
        assert np.max(np.abs(z[:nof_re].astype(np.complex128) - zm)) <= tol("z" if j["format"] >= M.F2 else "z_f1") * np.max(np.abs(zm)), name
    assert np.array_equal(grid, before)  # only read
    assert capfd.readouterr().err == ""
