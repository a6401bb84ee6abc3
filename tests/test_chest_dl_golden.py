"""tests/chest_dl_model.py against what the reference's srsran_chest_dl_estimate_cfg gave (tests/golden/chest_dl_ref.npz, recorded by
tools/gen_golden_chest_dl.py), case by case, at the project's bounds for the uplink estimator's model: the ce grids within 1e-6 of max |ce|, the power-like
values (per-pair rsrp, rssi, rsrp_corr and noise estimates, what fill_res sets; dB values as the power ratio they stand for) within 1e-5 relative, cfo
within 4e-3 Hz.  The recorded distances of the reference to the model sit under these bounds (worst: 2.7e-7, 1.4e-6, 3.8e-9 Hz), so no wider one is used.
NAN, +-inf and exact zeros (a noise estimate of 0, its logarithm, the ce of zeros behind a filter of length 0, what fill_res leaves alone) compare exactly,
and the reference left no sentinel in a grid it was given.  The model is what tests/test_gpu_chest_dl.py holds the device to.  No device."""
import os

import numpy as np

import chest_dl_model as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID_BOUND, POWER_BOUND, CFO_BOUND = 1e-6, 1e-5, 4e-3


def record():
    return np.load(os.path.join(G, "chest_dl_ref.npz"))


def test_record_covers_the_cases():
    d = record()
    c = d["cases"]
    assert sorted(set(c[:, 0])) == [6, 15, 25, 100] and sorted(set(c[:, 1])) == [1, 2, 4] and sorted(set(c[:, 2])) == [1, 2] and set(c[:, 3]) == {6, 7}
    assert set(c[:, 4]) == {M.ALG_AVERAGE, M.ALG_INTERPOLATE} and set(c[:, 5]) == {M.FILTER_GAUSS, M.FILTER_TRIANGLE, M.FILTER_NONE}
    assert set(c[:, 6]) == {M.NOISE_REFS, M.NOISE_PSS, M.NOISE_EMPTY} and {0, 5} < set(c[:, 7]) and set(c[:, 8] % 6) == {0, 2, 5}
    assert set(d["snr_db"]) == {0.0, 10.0, 30.0} and set(c[:, 9]) == {0, 1} and set(c[:, 10]) == {0, 1}
    hundred = c[c[:, 0] == 100]
    assert len(hundred) == 1 and tuple(hundred[0, 1:3]) == (1, 1)
    auto = (c[:, 5] == M.FILTER_GAUSS) & (d["filter_coef"][:, 0] <= 0)
    assert auto.sum() >= 3 and (d["filter_coef"][:, 0] == 8).any()  # automatic taps; nine taps
    assert os.path.getsize(os.path.join(G, "chest_dl_ref.npz")) <= max(os.path.getsize(os.path.join(G, f)) for f in os.listdir(G))
    for i in range(len(c)):
        assert d["flags_%d" % i][0], i  # the reference wrote every point of every grid it was given
        assert d["flags_%d" % i][1] == (c[i, 4] == M.ALG_AVERAGE), i
        dist = d["dist_%d" % i]  # its distance to the float64 model when the record was made
        assert dist[0] < GRID_BOUND and dist[1] < POWER_BOUND and dist[2] < CFO_BOUND and dist[3] == 1, (i, dist)


def test_model_against_the_reference_record():
    d = record()
    for i in range(len(d["cases"])):
        cfg, state, grids, pilots, pss = M.case_of(d, i)
        m = M.estimate(cfg, state, grids, pilots, pss)
        want = M.recorded_ce(d, i)
        assert want.shape == m["ce"].shape, i
        assert M.grid_distance(want, m["ce"]) <= GRID_BOUND, i
        assert np.array_equal(want == 0, m["ce"] == 0), i
        power, cfo, same = M.scalar_distance(M.named(m), M.unpack(d["out_%d" % i], d["state_out_%d" % i]))
        assert power <= POWER_BOUND and cfo <= CFO_BOUND and same, (i, power, cfo, same)


def test_a_filter_of_length_zero_gives_a_ce_of_zeros():
    """automatic Gauss taps from a noise estimate of 0 (PSS / EMPTY before the first subframe 0 or 5): chest_common.c:87 returns length 0, the convolution
    sums nothing -- the record has the case, and the measurements show it (noise 0, snr +inf)"""
    d = record()
    hit = [i for i in range(len(d["cases"])) if not M.recorded_ce(d, i).any()]
    assert len(hit) == 1
    o = M.unpack(d["out_%d" % hit[0]], d["state_out_%d" % hit[0]])
    assert o["noise_estimate"] == 0 and np.isneginf(o["noise_estimate_dbm"]) and np.isposinf(o["snr_db"])
    assert M.taps(M.FILTER_GAUSS, (0.0, 0.0), 0.0).size == 0


def test_model_time_interpolation_is_a_chain_from_the_first_symbol_for_ports_2_and_3():
    """interpolate_pilots, chest_dl.c:537-539: symbols 9 .. 13 of ports 2 and 3 start at symbol 1, not at symbol 8"""
    sched = M.time_schedule(7, 2)
    assert sched[2] == (1, 8, 1, 9, 7, 5) and M.time_schedule(6, 3)[2] == (1, 7, 1, 8, 6, 4)
    covered = {1, 8} | {b + k for _, _, _, b, _, m in sched for k in range(m)}
    assert covered == set(range(14))
    for cp, port in ((7, 0), (6, 1), (6, 2)):
        crs = {M.nsymbol(l, cp, port) for l in range(M.nof_symbols(port))}
        assert crs | {b + k for _, _, _, b, _, m in M.time_schedule(cp, port) for k in range(m)} == set(range(2 * cp))
