"""The PDSCH's RE de-mapping against the reference's own srsran_pdsch_get (tests/golden/pdsch_map_ref.npz, recorded by tools/gen_golden_pdsch_map.py): the numpy
model the GPU tests use (tests/pdsch_map_model.py) gives the recorded indices element by element, and the library's host-side count (srsran_hip_pdsch_nof_re:
csrc/pdsch_map.h, the restatement the segment table is built from) gives the recorded counts.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_api as O
import pdsch_map_model as PM

REC = os.path.join(O.ROOT, "tests", "golden", "pdsch_map_ref.npz")


@pytest.fixture(scope="module")
def record():
    z = np.load(REC)
    out = []
    for i, row in enumerate(z["cases"]):
        nof_prb, ports, cell_id, cp, ft, sfi, lstart, n0, n1, nof_re = (int(v) for v in row)
        sf = PM.make(nof_prb, ports, cell_id, z["prb_%d" % i], cp, ft, sfi, lstart, (n0, n1))
        out.append((z["kinds"][i].decode(), sf, np.cumsum(z["step_%d" % i]).astype(np.int32), nof_re))
    return out


def test_record_covers_what_it_should(record):
    sfs = [sf for _, sf, _, _ in record]
    kinds = {k for k, _, _, _ in record}
    assert {sf["nof_prb"] for sf in sfs} == {6, 15, 25, 50} and {sf["ports"] for sf in sfs} == {1, 2, 4} and {sf["cp_nsymb"] for sf in sfs} == {6, 7}
    assert {sf["cell_id"] % 6 for sf in sfs if sf["ports"] == 1} == set(range(6)) and {sf["cell_id"] % 3 for sf in sfs if sf["ports"] > 1} == set(range(3))
    assert {(sf["frame_type"], sf["sf_idx"]) for sf in sfs} >= {(0, 0), (0, 5), (0, 1), (1, 0), (1, 1), (1, 5), (1, 6)}
    assert {sf["nsymb"] for sf in sfs} >= {(7, 7), (6, 6), (7, 5), (7, 2), (3, 0)}
    assert {sf["lstart"] for sf in sfs if sf["nof_prb"] > 6} >= {1, 2, 3} and {sf["lstart"] for sf in sfs if sf["nof_prb"] == 6} >= {2, 3, 4}
    assert kinds >= {"crs_all", "sync_all", "sync_one_centre", "sync_one_edge", "sync_random", "sync_centre", "sync_halves", "short_all", "short_random", "wide_random"}
    assert all(idx.size == n for _, _, idx, n in record)
    assert any(n == 0 for _, _, _, n in record)  # an allocation wholly under the synchronisation signals gives nothing
    assert os.path.getsize(REC) < 512 * 1024


def test_model_gives_the_reference_indices(record):
    for i, (kind, sf, idx, nof_re) in enumerate(record):
        got = PM.indices(sf)
        assert got.size == nof_re, (i, kind, got.size, nof_re)
        bad = np.flatnonzero(got != idx)
        assert bad.size == 0, (i, kind, {k: v for k, v in sf.items() if k != "prb"}, int(bad[0]), int(got[bad[0]]), int(idx[bad[0]]))
        assert idx.size == 0 or idx.max() < PM.grid_points(sf)


def test_library_count_is_the_reference_count(record):
    from srslte_amd import build, capi

    build.build(verbose=False)
    L = capi.lib()
    for i, (kind, sf, _, nof_re) in enumerate(record):
        c = PM.to_struct(capi, sf)
        assert L.srsran_hip_pdsch_nof_re(C.byref(c)) == nof_re, (i, kind)
        c.csi_enable = 1
        assert L.srsran_hip_pdsch_nof_re(C.byref(c)) == nof_re, (i, kind)
