"""PUCCH receive on the device (include/srsran_amd/phy_pucch_abi.h) through the C ABI, on the recorded cases of tests/golden/pucch_ref.npz (the reference's own
estimator and decoder on signals of its own encoder).  Every case through the _dbg call: decisions, bits, DRS bits and the 20 soft bits EXACT (the generator
asserts the margins that make them so), floats within the tolerances the generator measured.  The estimator stage alone on a sentinel-filled grid; group
calls against the single calls bit for bit, twice, with 1, 5 and 65 jobs; four host threads; the refusals that need a device."""
import ctypes as C
import threading

import numpy as np
import pytest

import pucch_model as M
from test_conv_abi import _one_line
from test_pucch_abi import a_job, set_tables, structs
from test_pucch_golden import check_against_record, ref, tol

pytestmark = pytest.mark.gpu
SENTINEL = np.complex64(-7.5 + 3.25j)
RES_FLOATS = ("correlation", "dmrs_correlation", "noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "rsrp", "rsrp_dBfs", "epre", "epre_dBfs", "ta_us")


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0 and set_tables(lib) == 0
    return lib


def as_dict(res):
    d = {k: np.float32(getattr(res, k)) for k in RES_FLOATS}
    d.update(detected=bool(res.detected), ack_valid=bool(res.ack_valid), pucch_bits=np.array(list(res.pucch_bits), np.uint8), drs=res.drs_bits[0] + 2 * res.drs_bits[1])
    return d


def decode_dbg(L, c):
    from srslte_amd import capi

    cell, sf, j, grid = M.case(c)
    cs, ss, js = structs(capi, cell, sf, j)
    z, llr, ce, pe = np.full(120, SENTINEL, np.complex64), np.full(20, 77, np.int16), np.full((2, 12), SENTINEL, np.complex64), np.full((6, 12), SENTINEL, np.complex64)
    res, before = capi.HipPucchRes(), grid.copy()
    dbg = capi.HipPucchDbg(z.ctypes.data, llr.ctypes.data, ce.ctypes.data, pe.ctypes.data)
    assert L.srsran_hip_pucch_decode_dbg(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, C.byref(res), C.byref(dbg)) == 0
    assert np.array_equal(grid, before)  # only read
    g = as_dict(res)
    g.update(z=z, llr=llr, ce=ce, pe=pe)
    return g, res


@pytest.mark.parametrize("c", range(M.n_cases()))
def test_every_recorded_case(L, c, capfd):
    from srslte_amd import capi

    g, res = decode_dbg(L, c)
    cell, sf, j, grid = M.case(c)
    p = M.plan(cell, sf, j)
    n_rs, nof_re = int(p["n_rs"]), 12 * int(p["N_sf"].sum())
    assert np.all(g["pe"][2 * n_rs:] == SENTINEL) and np.all(g["z"][nof_re:] == 0)  # rows behind 2 n_rs are the caller's; z behind nof_re is zeroed
    check_against_record(c, g, "case %d" % c)
    plain = capi.HipPucchRes()
    cs, ss, js = structs(capi, cell, sf, j)
    assert L.srsran_hip_pucch_decode(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, C.byref(plain)) == 0 and bytes(plain) == bytes(res)
    assert capfd.readouterr().err == ""


@pytest.mark.parametrize("c", [0, 13, 21, 34, 41, 47, 53])  # formats 1 / 1A / 1B / 2 / 2B, both prefixes, 6 and 25 PRB, smoothing off, a noise-only case
def test_estimator_stage_alone(L, c, capfd):
    from srslte_amd import capi

    cell, sf, j, grid = M.case(c)
    p, e = M.plan(cell, sf, j), ref(c)
    nsymb = 6 if cell["cp"] else 7
    cs, ss, js = structs(capi, cell, sf, j)
    ce, res = np.full((2 * nsymb, 12 * cell["nof_prb"]), SENTINEL, np.complex64), capi.HipPucchRes()
    assert L.srsran_hip_chest_ul_estimate_pucch(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, ce.ctypes.data, C.byref(res)) == 0
    mask = np.zeros(ce.shape, bool)
    for s in range(2):
        cols = slice(12 * p["n_prb"][s], 12 * p["n_prb"][s] + 12)
        mask[s * nsymb:(s + 1) * nsymb, cols] = True
        rows = ce[s * nsymb:(s + 1) * nsymb, cols]
        assert np.all(rows == rows[0]) and np.max(np.abs(rows[0].astype(np.complex128) - e["ce"][s])) <= tol("ce") * np.max(np.abs(e["ce"])), (c, s)
    assert np.all(ce[~mask] == SENTINEL)  # nothing else is written
    full, _ = decode_dbg(L, c)
    for k in ("noise_estimate", "noise_estimate_dbm", "snr", "snr_db", "rsrp", "rsrp_dBfs", "epre", "epre_dBfs", "ta_us"):  # the same bits as the full call's
        assert np.float32(getattr(res, k)).tobytes() == np.float32(full[k]).tobytes(), (c, k)
    assert list(res.drs_bits) == [full["drs"] % 2, full["drs"] // 2] and not res.detected and res.correlation == 0 and not any(res.pucch_bits) and not res.ack_valid
    assert capfd.readouterr().err == ""


def group(cell_key, tti, shortened):
    r = M.record()
    return [c for c in range(M.n_cases()) if tuple(int(v) for v in r["cell"][c]) == cell_key and int(r["sf"][c][0]) == tti and int(r["sf"][c][1]) == shortened]


def multi(L, cell, sf, jobs, grid):
    from srslte_amd import capi

    cs, ss, _ = structs(capi, cell, sf, jobs[0])
    arr = (capi.HipPucchJob * len(jobs))(*[structs(capi, cell, sf, j)[2] for j in jobs])
    res = (capi.HipPucchRes * len(jobs))()
    C.memset(res, 0x55, C.sizeof(res))
    assert L.srsran_hip_pucch_decode_multi(C.byref(cs), C.byref(ss), len(jobs), arr, grid.ctypes.data, res) == 0
    return bytes(res)


def single(L, cell, sf, j, grid):
    from srslte_amd import capi

    cs, ss, js = structs(capi, cell, sf, j)
    res = capi.HipPucchRes()
    assert L.srsran_hip_pucch_decode(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, C.byref(res)) == 0
    return bytes(res)


@pytest.mark.parametrize("key", [((6, 0, 1), 0, 0), ((6, 1, 77), 0, 0), ((25, 0, 150), 7, 0), ((25, 0, 150), 7, 1)])
def test_group_calls_equal_the_single_calls(L, key, capfd):
    """all recorded jobs of one (cell, subframe) on ONE of its grids -- most find no signal of theirs there: hypotheses that fail -- in one call, against
    the single calls, bit for bit, twice; then 1, 5 and 65 jobs (the recorded ones repeated), which do not fill a workgroup of four"""
    cases = group(*key)
    assert len(cases) >= 2
    cell, sf, _, grid = M.case(cases[0])
    jobs = [M.case(c)[2] for c in cases]
    want = [single(L, cell, sf, j, grid) for j in jobs]
    got = multi(L, cell, sf, jobs, grid)
    assert got == b"".join(want) and multi(L, cell, sf, jobs, grid) == got
    for n in (1, 5, 65):
        rep = [jobs[i % len(jobs)] for i in range(n)]
        assert multi(L, cell, sf, rep, grid) == b"".join(want[i % len(jobs)] for i in range(n)), n
    # the first job's own grid: the record's decisions come out of the group call too
    first = M.record()["outf"][cases[0]]
    res0 = np.frombuffer(got[:64], np.uint32)[0]
    assert bool(res0) == bool(first[0])
    assert capfd.readouterr().err == ""


def test_four_host_threads(L):
    cases, out, want = [3, 20, 36, 44], {}, {}
    for c in cases:
        cell, sf, j, grid = M.case(c)
        want[c] = single(L, cell, sf, j, grid)

    def work(c):
        cell, sf, j, grid = M.case(c)
        got = [single(L, cell, sf, j, grid) for _ in range(5)] + [multi(L, cell, sf, [j] * 3, grid)]
        out[c] = all(g == want[c] for g in got[:5]) and got[5] == want[c] * 3

    threads = [threading.Thread(target=work, args=(c,)) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out == {c: True for c in cases}


def test_refusals_with_a_device(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    cell, sf, j, grid = M.case(0)
    cs, ss, js = structs(capi, cell, sf, j)
    n = 257
    res = (capi.HipPucchRes * n)()
    C.memset(res, 0x77, C.sizeof(res))
    jobs = (capi.HipPucchJob * n)(*[js] * n)
    capfd.readouterr()
    assert L.srsran_hip_pucch_decode_multi(C.byref(cs), C.byref(ss), n, jobs, grid.ctypes.data, res) == INV and bytes(res) == b"\x77" * C.sizeof(res)
    _one_line(capfd, "srsran_hip_pucch_decode_multi", "n")
    assert L.srsran_hip_pucch_decode_multi(C.byref(cs), C.byref(ss), 256, jobs, grid.ctypes.data, res) == 0  # the maximum runs
    assert bytes(res)[:256 * 64] == single(L, cell, sf, j, grid) * 256 and bytes(res)[256 * 64:] == b"\x77" * 64
    bad = structs(capi, cell, sf, dict(j, N_cs=3, delta_pucch_shift=2))[2]
    jobs[200] = bad
    C.memset(res, 0x77, C.sizeof(res))
    capfd.readouterr()
    assert L.srsran_hip_pucch_decode_multi(C.byref(cs), C.byref(ss), 256, jobs, grid.ctypes.data, res) == INV and bytes(res)[:256 * 64] == bytes(256 * 64)
    _one_line(capfd, "srsran_hip_pucch_decode_multi", "job 200")
    try:
        assert L.srsran_hip_pucch_set_tables(None, None) == 0
        one = capi.HipPucchRes()
        capfd.readouterr()
        assert L.srsran_hip_pucch_decode(C.byref(cs), C.byref(ss), C.byref(js), grid.ctypes.data, C.byref(one)) == INV and bytes(one) == bytes(64)
        _one_line(capfd, "srsran_hip_pucch_decode", "no tables")
    finally:
        assert set_tables(L) == 0
    assert single(L, cell, sf, a_job(format=M.F2, nof_uci_bits=0, n_pucch=3, n_rb_2=1), grid)  # the degenerate one-word search runs
    assert capfd.readouterr().err == ""
