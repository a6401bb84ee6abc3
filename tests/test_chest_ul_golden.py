"""tests/chest_ul_model.py against what the reference's srsran_chest_ul_estimate_pusch gave (tests/golden/chest_ul_ref.npz, recorded by
tools/gen_golden_chest_ul.py), case by case: the rows within 1e-6 max |ce|, noise_estimate and snr within 1e-5 relative, cfo_hz within 4e-3 Hz; ta_us, the
NAN / -inf cases and the untouched surroundings exact.  The model is what tests/test_gpu_chest_ul.py holds the device's measurements to.  No device."""
import os

import numpy as np

import chest_ul_model as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def record():
    return np.load(os.path.join(G, "chest_ul_ref.npz"))


def case_grid(d, i, rng=None):
    """(grid, r, geometry, filter or None, meas_ta_en) of case i: the two recorded rows in a grid that is random (rng) or zero everywhere else"""
    L_prb, nof_prb, n_prb, cp_nsymb, filter_on, meas_ta_en = [int(v) for v in d["cases"][i]]
    n, a = 12 * L_prb, 12 * n_prb
    shape = (2 * cp_nsymb, 12 * nof_prb)
    grid = np.zeros(shape, np.complex64) if rng is None else (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    for s in range(2):
        grid[M.ref_symbol(s, cp_nsymb), a:a + n] = d["rx_%d" % i][s]
    return np.ascontiguousarray(grid.reshape(-1)), d["r_%d" % i], (nof_prb, cp_nsymb, n_prb, L_prb), d["filter"] if filter_on else None, meas_ta_en


def test_record_covers_the_cases():
    d = record()
    c = d["cases"]
    assert sorted(set(c[:, 0])) == [1, 2, 6, 25, 100] and set(c[:, 3]) == {6, 7} and set(d["snr_db"]) == {0.0, 10.0, 30.0}
    assert set(c[:, 4]) == {0, 1} and np.sum(c[:, 5] == 0) == 1 and np.sum(c[:, 0] == 100) <= 2
    for i in range(len(c)):
        assert d["flags_%d" % i].all(), i  # the reference wrote the grant's columns of every symbol, and nothing else
        # and sat within these distances of the float64 model when the record was made
        dist = d["dist_%d" % i]
        assert dist[0] < 1.5e-7 and dist[1] < 1.1e-6 and dist[2] < 1.1e-6 and dist[3] < 5e-5 and dist[4] == 0, (i, dist)


def test_model_against_the_reference_record():
    d = record()
    sentinel = d["sentinel"][0]
    for i in range(len(d["cases"])):
        grid, r, (nof_prb, cp_nsymb, n_prb, L_prb), filt, meas_ta_en = case_grid(d, i)
        ce0 = np.full(grid.size, sentinel, np.complex64)
        sm, m, ce = M.estimate(grid, r, nof_prb, cp_nsymb, (n_prb, n_prb), L_prb, filt, meas_ta_en, ce=ce0)
        want, out = d["ce_%d" % i], d["out_%d" % i]
        assert np.max(np.abs(sm - want.astype(np.complex128))) <= 1e-6 * np.max(np.abs(want)), i
        noise, noise_dbm, snr, snr_db, cfo_hz, ta_us = [np.float32(v) for v in out]
        if filt is None:  # no smoothing: noise 0, its logarithm -inf, snr NAN
            assert noise == 0 and m["noise_estimate"] == 0 and np.isnan(snr) and np.isnan(m["snr"]) and np.isnan(snr_db) and np.isnan(m["snr_db"]), i
            assert np.isneginf(noise_dbm) and np.isneginf(m["noise_estimate_dbm"]), i
        else:
            assert abs(float(m["noise_estimate"]) - float(noise)) <= 1e-5 * float(noise) and abs(float(m["snr"]) - float(snr)) <= 1e-5 * float(snr), i
            assert abs(float(m["snr_db"]) - float(snr_db)) <= 1e-4 and abs(float(m["noise_estimate_dbm"]) - float(noise_dbm)) <= 1e-4, i
        assert abs(float(m["cfo_hz"]) - float(cfo_hz)) <= 4e-3, i
        assert m["ta_us"] == ta_us and (meas_ta_en or ta_us == 0), i
        # the grid: the slot's row in the grant's columns of every symbol, the sentinel everywhere else
        g2 = ce.reshape(2 * cp_nsymb, 12 * nof_prb)
        inside = np.zeros(g2.shape, bool)
        inside[:, 12 * n_prb:12 * (n_prb + L_prb)] = True
        assert np.all(g2[~inside] == sentinel), i
        for l in range(2 * cp_nsymb):
            assert np.array_equal(g2[l, 12 * n_prb:12 * (n_prb + L_prb)], sm[l // cp_nsymb].astype(np.complex64)), i


def test_model_places_a_hopping_grant_by_slot():
    """n_prb_tilde differs between the slots: each slot is read and written where the UE sent it (the reference's record has no such case)"""
    rng = np.random.default_rng(3)
    nof_prb, cp_nsymb, L_prb, n_prb = 15, 7, 2, (1, 9)
    n = 12 * L_prb
    grid = (rng.standard_normal(14 * 180) + 1j * rng.standard_normal(14 * 180)).astype(np.complex64)
    r = np.exp(2j * np.pi * rng.random(2 * n)).astype(np.complex64)
    sm, _, ce = M.estimate(grid, r, nof_prb, cp_nsymb, n_prb, L_prb, None, 1)
    g, c = grid.reshape(14, 180), ce.reshape(14, 180)
    for s in range(2):
        want = g[M.ref_symbol(s, cp_nsymb), 12 * n_prb[s]:12 * n_prb[s] + n].astype(np.complex128) * np.conj(r[s * n:(s + 1) * n].astype(np.complex128))
        assert np.array_equal(sm[s], want)
        assert np.array_equal(c[7 * s:7 * s + 7, 12 * n_prb[s]:12 * n_prb[s] + n], np.tile(want.astype(np.complex64), (7, 1)))
        other = np.ones(180, bool)
        other[12 * n_prb[s]:12 * n_prb[s] + n] = False
        assert not c[7 * s:7 * s + 7, other].any()
