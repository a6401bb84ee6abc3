"""tests/nr_chest_model.py against the reference's record, tests/golden/nr_chest_ref.npz (tools/gen_golden_nr_chest.py wrote it from the reference's
srsran_dmrs_sch_estimate and srsran_dmrs_sch_get_symbols_idx): the DMRS symbols and nof_re exact; the extracted ce and the measurements within the
distances the record itself states for the reference (and the ce within 2.5e-5 of max |ce|, as the generator asserted).  The extraction positions are held
through the ce: the estimates of neighbouring REs differ by far more than the distance allowed, so an RE taken from a wrong place, or in a wrong order, shows.
Needs no device."""
import functools
import os

import numpy as np
import pytest

import nr_chest_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nr_chest_ref.npz")
CFG_KEYS = ["nof_prb", "scs", "slot_idx", "S", "L", "dmrs_type", "typeA_pos", "additional_pos", "length", "n_id", "n_scid", "cdm"]


@functools.lru_cache(maxsize=None)
def record():
    return dict(np.load(GOLDEN))


def nof_cases():
    return len(record()["names"])


def case_cfg(d, i):
    cfg = {k: int(v) for k, v in zip(CFG_KEYS, d["cfg_%d" % i])}
    cfg["beta"] = float(d["beta_%d" % i])
    cfg["rvd"] = [tuple(int(x) for x in row) for row in d["rvd_%d" % i]]
    cfg["prb"] = d["prb_%d" % i]
    return cfg


def fill_grid(seed, nof_prb):
    """the grid outside the DMRS rows, as tools/gen_golden_nr_chest.py drew it"""
    rng = np.random.default_rng(int(seed))
    return (0.7 * (rng.standard_normal((14, 12 * nof_prb)) + 1j * rng.standard_normal((14, 12 * nof_prb)))).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def case_grid(i):
    """(cfg, grid [14, 12 nof_prb] complex64): the recorded DMRS rows in the regenerated grid.  Shared: do not write to it."""
    d = record()
    cfg = case_cfg(d, i)
    grid = fill_grid(d["gseed_%d" % i], cfg["nof_prb"])
    grid[M.dmrs_symbols(cfg)] = d["rows_%d" % i]
    grid.setflags(write=False)
    return cfg, grid


@functools.lru_cache(maxsize=None)
def case_model(i):
    cfg, grid = case_grid(i)
    return M.estimate(grid, cfg)


def distances(m, ce, out8):
    """tools/gen_golden_nr_chest.py: ce relative to max |ce|, noise_estimate, rsrp and sync_error relative, cfo in Hz"""
    rel = lambda a, b: 0.0 if a == b else (np.inf if b == 0 else abs(float(a) - float(b)) / abs(float(b)))  # noqa: E731
    return np.array([np.max(np.abs(ce.astype(np.complex128) - m["ce"])) / np.max(np.abs(m["ce"])), rel(out8[0], m["noise_estimate"]), rel(out8[2], m["rsrp"]),
                     abs(float(out8[5]) - float(m["cfo"])), rel(out8[6], m["sync_error"])], np.float64)


def test_record_covers_the_cases():
    d = record()
    cfgs = [case_cfg(d, i) for i in range(nof_cases())]
    n_sym = {len(M.dmrs_symbols(c)) for c in cfgs}
    assert n_sym == {1, 2, 3, 4}
    assert {c["dmrs_type"] for c in cfgs} == {0, 1} and {c["typeA_pos"] for c in cfgs} == {2, 3} and {c["length"] for c in cfgs} == {1, 2}
    assert {1, 2} <= {c["cdm"] for c in cfgs} and any(c["n_scid"] for c in cfgs) and any(c["beta"] != 1.0 for c in cfgs)
    assert any(c["S"] > 0 and c["S"] + c["L"] < 14 for c in cfgs)
    assert any(len(c["rvd"]) == 1 and c["rvd"][0][2] > 1 for c in cfgs) and any(len(c["rvd"]) == 2 for c in cfgs)
    assert any(c["nof_prb"] == 275 for c in cfgs) and {0.0, 10.0, 30.0} <= {float(x) for x in d["snr_db"] if not np.isnan(x)}
    assert sum(np.isnan(d["snr_db"])) == 1  # the noiseless flat-channel case
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("i", range(nof_cases()))
def test_model_against_the_record(i):
    d = record()
    cfg, grid = case_grid(i)
    sym5, out8, ce = d["sym_%d" % i], d["out_%d" % i], d["ce_%d" % i]
    sym = M.dmrs_symbols(cfg)
    assert sym5[0] == len(sym) and list(sym5[1:1 + len(sym)]) == sym
    m = case_model(i)
    assert m["nof_re"] == int(out8[7]) == ce.size == M.nof_re(cfg) == M.positions(cfg)[0].size
    dist = distances(m, ce, out8)
    print(d["names"][i], dist)
    assert dist[0] <= 2.5e-5
    assert np.allclose(dist, d["dist_%d" % i], rtol=1e-6, atol=1e-12), (dist, d["dist_%d" % i])
    # the dB values are the reference's log10f of its own linear values
    db = M.db_values(out8[2], out8[0])
    assert abs(float(db["rsrp_dbm"]) - float(out8[3])) <= 1e-5 * abs(float(out8[3])) + 1e-6 and abs(float(db["noise_estimate_dbm"]) - float(out8[1])) <= 2e-5
    if np.isnan(d["snr_db"][i]):  # flat and noiseless: both isnormal branches are skipped
        assert out8[5] == 0 and out8[6] == 0 and m["cfo"] == 0 and m["sync_error"] == 0


def test_put_and_get_are_inverse():
    cfg, grid = case_grid(3)
    g = np.array(grid)
    x = (np.arange(M.nof_re(cfg)) + 1j).astype(np.complex64)
    M.put(g, cfg, x)
    assert np.array_equal(M.get(g, cfg), x)
    idx = M.positions(cfg)[0]
    assert np.all(np.diff(idx) > 0) and idx.min() >= cfg["S"] * 12 * cfg["nof_prb"] and idx.max() < (cfg["S"] + cfg["L"]) * 12 * cfg["nof_prb"]
