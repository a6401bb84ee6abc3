#!/usr/bin/env python3
"""Record which REs the reference's srsran_pdsch_get (lib/src/phy/phch/pdsch.c:246; srsran_pdsch_cp :136-220, prb_dl.c) takes from a subframe grid:
tests/golden/pdsch_map_ref.npz.

    python tools/gen_golden_pdsch_map.py          (needs the reference tree and oracle/_ref/libsrsran_ref.so, built by `make -C oracle ref`)

tools/pdsch_map_ref_wrap.c includes the reference's pdsch.c and prb_dl.c where they lie and exports one wrapper.  It is compiled with the REF_FLAGS of
oracle/Makefile into a temporary directory (nothing compiled is kept) and loaded lazily behind libsrsran_ref.so, which is loaded globally for the data symbols
pdsch.c refers to; the call itself binds nothing outside the wrapper.  The function runs on a grid whose point i is (i, 0); the real parts of what it extracts are
the indices.

The record: `cases` int32 [n][10] = nof_prb, ports, cell_id, cp_nsymb, frame_type, sf_idx, lstart, nsymb0, nsymb1, nof_re (what the function returned);
`prb_<i>` uint8 [2][nof_prb]; `step_<i>` int32 [nof_re]: the indices as their first differences (step[0] is the first index, np.cumsum gives the indices back:
runs of 1 compress, the plain indices do not and would take 690 KB).  The file is written with fixed zip time stamps, so the tool reproduces it byte for byte.

Cases (6-, 15- and 25-PRB cells, one 50-PRB case; lstart rotates over 1 .. 3, 2 .. 4 on 6 PRB):
  crs    every PRB, FDD subframe 1, normal and extended CP: one port with cell ids covering id % 6 = 0 .. 5 ((id + 3) % 6 == 5 is where prb_cp_ref copies no
         tail), 2 and 4 ports with id % 3 = 0 .. 2
  sync   ports rotating, both CPs, FDD subframes 0 / 5 / 1 and TDD subframes 0 / 1 / 5 / 6, each with the masks: all PRBs; one PRB (a centre one, an edge one);
         random and different in the two slots; wholly inside the centre six; on odd cells only the two half PRBs
  short  TDD special and shortened subframes: nof_symb_slot {7,5}, {7,2}, {3,0} (normal CP) on subframes 0 / 1 / 5 / 6, all PRBs and a random mask
tests/test_pdsch_map_golden.py holds tests/pdsch_map_model.py and srsran_hip_pdsch_nof_re to this record."""
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_api as O  # noqa: E402
from gen_golden_csi import ref_flags  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pdsch_map_ref.npz")
FIELDS = ("nof_prb", "ports", "cell_id", "cp_nsymb", "frame_type", "sf_idx", "lstart", "nsymb0", "nsymb1", "nof_re")


def load_wrap(tmp):
    """the wrapper, built into `tmp`: fn(nof_prb, ports, cell_id, cp_nsymb, frame_type, sf_idx, lstart, nsymb0, nsymb1, prb, n_planes, grids, planes) -> nof_re"""
    rlib, flags = ref_flags()
    C.CDLL(O.REF_LIB, mode=os.RTLD_GLOBAL | os.RTLD_NOW)
    so = os.path.join(tmp, "libpdsch_map_ref_wrap.so")
    phch = os.path.join(rlib, "src", "phy", "phch")
    subprocess.check_call(["gcc"] + flags + ['-DREF_PDSCH_C="%s"' % os.path.join(phch, "pdsch.c"), '-DREF_PRB_DL_C="%s"' % os.path.join(phch, "prb_dl.c"), "-shared",
                           os.path.join(ROOT, "tools", "pdsch_map_ref_wrap.c"), "-o", so])
    fn = C.CDLL(so, mode=os.RTLD_LAZY).pdsch_map_ref_get
    fn.argtypes = [C.c_uint] * 9 + [C.c_void_p, C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    fn.restype = C.c_int
    return fn


def ref_args(case, prb, grids, planes):
    """the wrapper's arguments.  case: the first nine FIELDS; grids, planes: lists of complex64 arrays (kept alive by the caller, as is the returned tuple)"""
    prb = np.ascontiguousarray(prb, np.uint8)
    gp = (C.c_void_p * len(grids))(*[g.ctypes.data for g in grids])
    pp = (C.c_void_p * len(planes))(*[p.ctypes.data for p in planes])
    return tuple(int(v) for v in case[:9]) + (prb.ctypes.data, len(grids), gp, pp), prb


def ref_get(fn, case, prb, grids, planes):
    args, _keep = ref_args(case, prb, grids, planes)
    return fn(*args)


def masks(rng, nof_prb, sync):
    """(name, uint8 [2][nof_prb])"""
    half = nof_prb // 2
    m = [("all", np.ones((2, nof_prb), np.uint8))]
    if not sync:
        return m
    for name, n in (("one_centre", half), ("one_edge", nof_prb - 1)):
        one = np.zeros((2, nof_prb), np.uint8)
        one[:, n] = 1
        m.append((name, one))
    r = (rng.random((2, nof_prb)) < 0.5).astype(np.uint8)
    r[0, rng.integers(nof_prb)] = r[1, rng.integers(nof_prb)] = 1
    if np.array_equal(r[0], r[1]):
        r[1] ^= 1
    m.append(("random", r))
    c6 = np.zeros((2, nof_prb), np.uint8)
    c6[:, half - 3 + nof_prb % 2:half + 3] = 1  # (the seven centre PRBs of an odd cell less its two half ones)
    m.append(("centre", c6))
    if nof_prb % 2:
        h = np.zeros((2, nof_prb), np.uint8)
        h[:, [half - 3, half + 3]] = 1
        m.append(("halves", h))
    return m


def case_list():
    rng = np.random.default_rng(36211)
    cases, rot = [], 0

    def add(kind, nof_prb, ports, cell_id, cp, ft, sfi, nsymb, sync):
        nonlocal rot
        for name, prb in masks(rng, nof_prb, sync):
            lstart = 1 + rot % 3 + (1 if nof_prb < 10 else 0)
            rot += 1
            if lstart >= nsymb[0]:
                lstart = nsymb[0] - 1
            cases.append(("%s_%s" % (kind, name), (nof_prb, ports, cell_id, cp, ft, sfi, lstart, nsymb[0], nsymb[1]), prb))

    for nof_prb in (6, 15, 25):
        for cp in (7, 6):
            for k in range(6):
                add("crs", nof_prb, 1, (0, 301, 122, 63, 460, 503)[k], cp, 0, 1, (cp, cp), False)  # id % 6 = 0, 1, 2, 3, 4, 5
            for ports in (2, 4):
                for k in range(3):
                    add("crs", nof_prb, ports, (150, 1, 422)[k], cp, 0, 1, (cp, cp), False)  # id % 3 = 0, 1, 2
    ports_rot = 0
    for nof_prb in (6, 15, 25):
        for cp in (7, 6):
            for ft, sfi in ((0, 0), (0, 5), (0, 1), (1, 0), (1, 1), (1, 5), (1, 6)):
                ports = (1, 2, 4)[ports_rot % 3]
                ports_rot += 1
                add("sync", nof_prb, ports, 17 + 5 * ports_rot, cp, ft, sfi, (cp, cp), True)
    for nof_prb in (6, 15, 25):
        for sfi in (0, 1, 5, 6):
            for nsymb in ((7, 5), (7, 2), (3, 0)):
                ports = (1, 2, 4)[ports_rot % 3]
                ports_rot += 1
                add("short", nof_prb, ports, (90 + 7 * ports_rot) % 504, 7, 1, sfi, nsymb, False)
                r = (rng.random((2, nof_prb)) < 0.5).astype(np.uint8)
                r[:, rng.integers(nof_prb)] = 1
                cases.append(("short_random", (nof_prb, ports, (90 + 7 * ports_rot) % 504, 7, 1, sfi, min(2, nsymb[0] - 1), nsymb[0], nsymb[1]), r))
    r50 = (rng.random((2, 50)) < 0.6).astype(np.uint8)
    r50[:, 22:28] = 1
    cases.append(("wide_random", (50, 2, 77, 7, 0, 0, 2, 7, 7), r50))
    return cases


def write_npz(path, arrays):
    """np.load-readable, and the same bytes on every run: fixed time stamps, fixed order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    cases = case_list()
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_wrap(tmp)
        rows, arrays = [], []
        for i, (kind, case, prb) in enumerate(cases):
            pts = (case[7] + case[8]) * 12 * case[0]
            grid = np.arange(pts).astype(np.complex64)
            plane = np.full(pts + 8, -1, np.complex64)
            n = ref_get(fn, case, prb, [grid], [plane])
            assert 0 <= n <= pts and np.all(plane[n:] == -1) and np.all(plane[:n].imag == 0)
            rows.append(case + (n,))
            arrays += [("prb_%d" % i, prb), ("step_%d" % i, np.diff(plane[:n].real.astype(np.int32), prepend=0).astype(np.int32))]
    head = [("cases", np.array(rows, np.int32)), ("kinds", np.array([k for k, _, _ in cases], "S16"))]
    write_npz(OUT, head + arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases,", sum(r[-1] for r in rows), "REs")


if __name__ == "__main__":
    main()
