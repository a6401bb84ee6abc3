"""The reference's control-channel test programs on the device control path (tests/ref_link/Makefile target `ctrl`, tests/ref_link/ctrl_bind.c).

In oracle/_ref/ref_link/bin_ctrl the reference's own srsran_viterbi_* definitions are renamed away (the decoder handle of the PDCCH, PBCH, long-CQI, NB-IoT and
sidelink receivers is the library's) and srsran_pcfich_decode, srsran_phich_decode, srsran_pdcch_extract_llr and srsran_pdcch_decode_msg are the binding's, which
call srsran_hip_pcfich_decode, srsran_hip_phich_decode_multi, srsran_hip_pdcch_extract_llr and srsran_hip_pdcch_dci_decode_multi.  With CTRL_BIND_CHECK=1 every
such call also runs the renamed original on the same inputs and compares: decisions, DCI bits and the REG tables exactly (the tables once per distinct
description: pcfich_test and phich_test walk all 504 cell ids), the PCFICH's correlation, the PHICH's distance and the PDCCH's soft bits within the tolerances
the records tests/golden/ctrl_ref.npz and pdcch_sf_ref.npz store, handed over in the environment.  With CTRL_BIND_SEARCH=1 every candidate is decoded a second
time by srsran_hip_pdcch_search_sf from the grids of its subframe, and the result bytes must be those of srsran_hip_pdcch_dci_decode_multi.

The binding's [ctrl_bind] line at exit carries, per function, the calls on the device, the calls the library refused (they go to the original) and the
mismatches, then the descriptions whose tables were compared and the worst float deviations.  REF_CTEST_FULL=1 adds the phy_dl_test lines above 6 PRB.
"""
import json
import os
import re
import subprocess

import pytest
from ref_link_common import HERE, add_ctest_data, make_data_dir, program, run_program
from test_ctrl_golden import tol
from test_pdcch_sf_golden import llr_tol

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(HERE, "ref_link", "ctest_manifest.json")))["entries"]
FULL = os.environ.get("REF_CTEST_FULL", "0") == "1"

# the functions each program reaches: pcfich_decode, phich_decode, extract_llr, decode_msg (pbch_test and pbch_file_test reach the decoder handle only)
REACHES = {
    "pdcch_test": ("extract_llr", "decode_msg"),
    "pcfich_test": ("pcfich_decode",),
    "phich_test": ("phich_decode",),
    "pbch_test": (),
    "pbch_file_test": (),
    "pcfich_file_test": ("pcfich_decode",),
    "phich_file_test": ("phich_decode",),
    "pdcch_file_test": ("extract_llr", "decode_msg"),
    "pdsch_pdcch_file_test": ("pcfich_decode", "extract_llr", "decode_msg"),
    "phy_dl_test": ("pcfich_decode", "extract_llr", "decode_msg"),
}
FUNCTIONS = ("pcfich_decode", "phich_decode", "extract_llr", "decode_msg", "search")


def _arg(e, flag):
    a = e["args"]
    return int(a[a.index(flag) + 1])


def _phy_dl_6prb(e):
    return _arg(e, "-p") == 6


def _checked():
    for e in MANIFEST:
        if e["program"] == "phy_dl_test":
            if FULL or _phy_dl_6prb(e):
                yield e
        elif e["program"] in REACHES:
            yield e


def _searched():
    for e in MANIFEST:
        if e["program"] in ("pdcch_test", "pdsch_pdcch_file_test"):
            yield e
        elif e["program"] == "phy_dl_test" and _phy_dl_6prb(e) and _arg(e, "-t") == 1:
            yield e


def _viterbi_users():
    """programs judged by their exit code: the long CQI on PUSCH (srsran_viterbi_decode_s), one NB-IoT and one sidelink receiver"""
    seen = set()
    for e in MANIFEST:
        if e["program"] == "pusch_test" and "cqi" in e["args"]:
            yield e
        elif e["program"] in ("npbch_test", "psbch_test") and (FULL or e["program"] not in seen):
            seen.add(e["program"])
            yield e


REPORT = re.compile(r"\[ctrl_bind\] " + "".join(r"%s dev (\d+) ref (\d+) bad (\d+) \| " % f for f in FUNCTIONS) +
                    r"tables (\d+) bad (\d+) \| corr (\S+) distance (\S+) llr (\S+)")


def parse_report(out):
    m = REPORT.search(out)
    if not m:
        return None
    g = m.groups()
    r = {f: dict(dev=int(g[3 * i]), ref=int(g[3 * i + 1]), bad=int(g[3 * i + 2])) for i, f in enumerate(FUNCTIONS)}
    r.update(tables=int(g[15]), tables_bad=int(g[16]), corr=float(g[17]), distance=float(g[18]), llr=float(g[19]))
    return r


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory, hiplib):
    return add_ctest_data(make_data_dir(tmp_path_factory.mktemp("ref_ctrl_data")))


def run_bound(entry, data_dir, search=False):
    args = [str(data_dir / a[1:]) if a.startswith("@") else a for a in entry["args"]]
    env = {"CTRL_BIND_CHECK": "1", "CTRL_BIND_REPORT": "1", "CTRL_BIND_TOL_CORR": repr(tol("corr")), "CTRL_BIND_TOL_DISTANCE": repr(tol("distance")),
           "CTRL_BIND_TOL_LLR": repr(llr_tol())}
    if search:
        env["CTRL_BIND_SEARCH"] = "1"
    os.environ.update(env)
    try:
        rc, out = run_program("bin_ctrl", entry["program"], args, data_dir, timeout=900)
    finally:
        for k in env:
            del os.environ[k]
    assert rc == 0, "%s %s -> %d\n%s" % (entry["program"], " ".join(args), rc, out[-3000:])
    rep = parse_report(out)
    assert rep is not None, out[-1500:]
    print("%s: %s" % (entry["name"], REPORT.search(out).group(0)))
    return rep, out


def judge(entry, rep, out):
    reached = REACHES[entry["program"]]
    for f in FUNCTIONS[:4]:
        assert rep[f]["ref"] == 0 and rep[f]["bad"] == 0, (f, rep, out[-3000:])
        assert (rep[f]["dev"] > 0) == (f in reached), (f, rep)
    assert rep["tables_bad"] == 0 and (rep["tables"] > 0) == bool(reached), rep
    assert rep["corr"] <= tol("corr") and rep["distance"] <= tol("distance") and rep["llr"] <= llr_tol(), rep


@pytest.mark.parametrize("entry", list(_checked()), ids=lambda e: "ctrl:%s:%s" % (e["program"], e["name"]))
def test_ctest_line_on_the_device_control_path(entry, data_dir):
    rep, out = run_bound(entry, data_dir)
    judge(entry, rep, out)
    assert rep["search"] == dict(dev=0, ref=0, bad=0), rep


@pytest.mark.parametrize("entry", list(_searched()), ids=lambda e: "search:%s:%s" % (e["program"], e["name"]))
def test_ctest_line_with_every_candidate_searched_from_the_grids(entry, data_dir):
    rep, out = run_bound(entry, data_dir, search=True)
    judge(entry, rep, out)
    assert rep["search"]["dev"] == rep["decode_msg"]["dev"] > 0 and rep["search"]["ref"] == 0 and rep["search"]["bad"] == 0, (rep, out[-3000:])


@pytest.mark.parametrize("entry", list(_viterbi_users()), ids=lambda e: "viterbi:%s:%s" % (e["program"], e["name"]))
def test_ctest_line_on_the_librarys_decoder_handle(entry, data_dir):
    exe = program("bin_ctrl", entry["program"])
    syms = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True).stdout.split()
    assert "srsran_viterbi_init" in syms and ("srsran_viterbi_decode_s" in syms or "srsran_viterbi_decode_f" in syms), \
        "bin_ctrl/%s does not take its convolutional decoder from the library" % entry["program"]
    args = [str(data_dir / a[1:]) if a.startswith("@") else a for a in entry["args"]]
    rc, out = run_program("bin_ctrl", entry["program"], args, data_dir, timeout=900)
    assert rc == 0, "%s %s -> %d\n%s" % (entry["program"], " ".join(args), rc, out[-3000:])


def test_the_report_parser_reads_the_bindings_line():
    line = ("[ctrl_bind] pcfich_decode dev 3 ref 0 bad 0 | phich_decode dev 0 ref 1 bad 0 | extract_llr dev 3 ref 0 bad 0 | decode_msg dev 9 ref 0 bad 2 | "
            "search dev 9 ref 0 bad 0 | tables 2 bad 0 | corr 1.2e-07 distance 0 llr 3.4e-07")
    r = parse_report("noise\n" + line + "\n")
    assert r["decode_msg"] == dict(dev=9, ref=0, bad=2) and r["phich_decode"]["ref"] == 1 and r["tables"] == 2 and r["corr"] == 1.2e-07 and r["llr"] == 3.4e-07
    assert parse_report("nothing") is None
