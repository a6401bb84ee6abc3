"""numpy restatement of the PDSCH's RE de-mapping (srsran_pdsch_get, lib/src/phy/phch/pdsch.c:246; srsran_pdsch_cp :136-220): indices(sf) gives the grid index of
every extracted RE, in order.  tests/test_pdsch_map_golden.py holds it to the reference's own function (tests/golden/pdsch_map_ref.npz); the GPU tests hold the
library to it.

`sf` is a dict with the fields of srsran_hip_pdsch_sf_t (include/srsran_amd/phy_chan_abi.h): nof_prb, ports, cell_id, cp_nsymb, frame_type, sf_idx, lstart,
nsymb = (slot 0, slot 1), prb = uint8 [2][nof_prb].  The grid has (nsymb[0] + nsymb[1]) rows of 12 nof_prb points; symbol l of slot s is row l + s nsymb[0]."""
import numpy as np

K = np.arange(12)


def crs_free(sf, l):
    """bool [12]: the REs of a PRB that carry no cell-specific reference signal on symbol l of a slot"""
    if not (l == 0 or l == sf["cp_nsymb"] - 3 or (l == 1 and sf["ports"] == 4)):
        return np.ones(12, bool)
    if sf["ports"] == 1:
        return K % 6 != (sf["cell_id"] % 6 if l == 0 else (sf["cell_id"] + 3) % 6)
    return K % 3 != sf["cell_id"] % 3


def under_sync(sf, s, l, n):
    """PRB n on symbol l of slot s lies under PSS / SSS / PBCH"""
    nof_prb, sfi, ns = sf["nof_prb"], sf["sf_idx"], sf["nsymb"][s]
    if not (nof_prb // 2 - 3 <= n < nof_prb // 2 + 3 + nof_prb % 2):
        return False
    if sf["frame_type"] == 0:
        if s == 0 and sfi in (0, 5) and ns >= 2 and l >= ns - 2:  # (the reference's unsigned ns - 2: a one-symbol slot has no such symbols)
            return True
    else:
        if s == 1 and sfi in (0, 5) and l >= ns - 1:
            return True
        if s == 0 and sfi in (1, 6) and l == 2:
            return True
    return s == 1 and sfi == 0 and l < 4


def indices(sf):
    nof_prb = sf["nof_prb"]
    out = []
    for s in range(2):
        for l in range(sf["lstart"] if s == 0 else 0, sf["nsymb"][s]):
            keep = crs_free(sf, l)
            row = l + s * sf["nsymb"][0]
            for n in np.flatnonzero(np.asarray(sf["prb"][s][:nof_prb])):
                take = keep
                if under_sync(sf, s, l, n):
                    if nof_prb % 2 == 0:
                        continue
                    if n == nof_prb // 2 - 3:
                        take = keep & (K < 6)
                    elif n == nof_prb // 2 + 3:
                        take = keep & (K >= 6)
                    else:
                        continue
                out.append((row * nof_prb + n) * 12 + K[take])
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


def grid_points(sf):
    return (sf["nsymb"][0] + sf["nsymb"][1]) * 12 * sf["nof_prb"]


def to_struct(capi, sf, csi_enable=0):
    """the ctypes srsran_hip_pdsch_sf_t of the description"""
    c = capi.HipPdschSf(sf["nof_prb"], sf["ports"], sf["cell_id"], sf["cp_nsymb"], sf["frame_type"], sf["sf_idx"], sf["lstart"])
    c.nof_symb_slot[0], c.nof_symb_slot[1] = sf["nsymb"]
    c.csi_enable = csi_enable
    for s in range(2):
        for n in np.flatnonzero(np.asarray(sf["prb"][s][:sf["nof_prb"]])):
            c.prb_idx[s][n] = 1
    return c


def make(nof_prb, ports, cell_id, prb, cp_nsymb=7, frame_type=0, sf_idx=1, lstart=1, nsymb=None):
    prb = np.asarray(prb, np.uint8)
    assert prb.shape == (2, nof_prb)
    return dict(nof_prb=nof_prb, ports=ports, cell_id=cell_id, cp_nsymb=cp_nsymb, frame_type=frame_type, sf_idx=sf_idx, lstart=lstart,
                nsymb=tuple(nsymb) if nsymb is not None else (cp_nsymb, cp_nsymb), prb=prb)
