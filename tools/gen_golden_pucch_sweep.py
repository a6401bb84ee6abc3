#!/usr/bin/env python3
"""A second, compact record of the reference's PUCCH receive side, over cells, subframes and users per PRB: tests/golden/pucch_sweep_ref.npz.

    python tools/gen_golden_pucch_sweep.py            (needs the reference tree; about a minute; rewrites the file byte for byte)
    python tools/gen_golden_pucch_sweep.py --dry      (no reference: the listed groups through the model's plan and the coverage rules alone)
    python tools/gen_golden_pucch_sweep.py --survey   (every group's draws and the tolerances they would give; goes on past a group that finds no draw; writes nothing)

It stands on tools/gen_golden_pucch.py (the wrapper tools/pucch_ref_wrap.c, draw, run_reference, conditions, distances, words) and on the two tables
tests/golden/pucch_ref.npz already holds; neither is touched.

A GROUP is one cell, one subframe, one (N_cs, delta_pucch_shift, n_rb_2, group_hopping_en) and a list of jobs that together occupy one or two PRB pairs.
Each job marked present contributes the reference's own UE signal through a channel of its own (draw, at a per-user SNR of 200 dB: noiseless in
float32); the column blocks are summed per (slot, PRB) and noise is added once, at 10, 20 or 30 dB.  Absent jobs contribute nothing.  Then EVERY job of the
group, present or absent, goes through the reference and through the float64 model on the full grid.  Stored per group: the parameters, the seed, the
touched column blocks.  Per job: the job words, present, the sent bits, the reference's plan, outf, outb, llr, max_corr, early and the two ce rows
(z and pilot_estimates are not stored: the device test takes them from the model, which this generator holds to the reference here).

Asserted on the reference alone, as gen_golden_pucch.py does: conditions() is None for every job of a group, or the whole group is drawn again with
the next seed (20 draws, then the generator fails: no job is left out); the model's decisions, bits, DRS bits, llr and max_corr equal the reference's;
in a group with a single present user the reference decodes what was sent.  With two or three users on a PRB the reference's receiver is NOT required
to decode what was sent -- it does not separate many users -- only to be reproduced, with its margins.
Tolerances: per float quantity four times the worst model-reference deviation over the sweep's jobs; the draws use gen_golden_pucch.PROVISIONAL and
the conditions are asserted again with the stored values.  The coverage rules (tests/pucch_sweep.py: coverage) are asserted before the file is written."""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "tests", "golden", "pucch_sweep_ref.npz")
USER_SNR_DB = 200.0
F1, F1A, F1B, F2, F2A, F2B = range(6)
P, A = 1, 0


def J(fmt, n_pucch, present, nbits=0, drs=(0, 0), **settings):
    """settings: filter_on, meas_ta, th_dmrs.  An absent job is decoded with meas_ta_en = 0 unless it says otherwise: the time alignment of an empty
    resource is the angle of a noise sum, and its rounding rule alone turns down one draw in five"""
    settings.setdefault("meas_ta", present)
    return dict(fmt=fmt, n_pucch=n_pucch, present=present, nbits=nbits, drs=drs, **settings)


def G(cell, tti, short, N_cs, delta, n_rb_2, hop, noise_db, jobs):
    return dict(cell=cell, tti=tti, short=short, N_cs=N_cs, delta=delta, n_rb_2=n_rb_2, hop=hop, noise_db=noise_db, jobs=jobs)


GROUPS = [
    # ---- formats 1x beside each other where n_pucch >= c N_cs / delta: the same n_oc and another n_cs, or (in one slot) the same n_cs and another n_oc
    G((6, 0, 0), 0, 0, 0, 1, 0, 0, 20, [J(F1A, 0, P), J(F1B, 1, P), J(F1A, 12, A, meas_ta=1), J(F1, 24, A), J(F1B, 5, A)]),
    G((6, 1, 29), 1, 1, 0, 1, 0, 1, 10, [J(F1A, 1, P), J(F1B, 2, P), J(F1, 3, A), J(F1A, 13, A), J(F1B, 20, A)]),
    G((15, 0, 31), 2, 0, 0, 2, 1, 0, 10, [J(F1B, 0, P), J(F1A, 12, P), J(F1, 1, A), J(F1A, 20, P), J(F1B, 25, A, meas_ta=0)]),
    G((25, 0, 62), 3, 1, 0, 3, 0, 1, 20, [J(F1, 0, P), J(F1A, 1, P), J(F1B, 10, A), J(F1A, 2, A), J(F1B, 5, A)]),
    G((75, 0, 341), 1, 0, 0, 1, 0, 0, 20, [J(F1A, 0, P), J(F1B, 1, P), J(F1, 11, A), J(F1A, 2, A), J(F1B, 25, A, filter_on=0)]),
    G((100, 0, 372), 2, 1, 0, 2, 2, 1, 10, [J(F1B, 0, P), J(F1A, 2, P), J(F1, 4, A), J(F1A, 9, A), J(F1B, 17, A)]),
    G((6, 1, 403), 3, 0, 0, 2, 0, 0, 20, [J(F1A, 0, P), J(F1B, 1, P), J(F1, 2, A), J(F1A, 6, A), J(F1B, 8, A)]),
    G((100, 0, 186), 7, 0, 0, 2, 0, 1, 10, [J(F1A, 162, P), J(F1B, 174, P), J(F1, 163, A), J(F1A, 170, A), J(F1B, 150, P), J(F1A, 151, A)]),
    G((50, 1, 428), 14, 1, 3, 3, 1, 1, 20, [J(F1B, 2, P), J(F1A, 7, A), J(F1, 4, A), J(F1B, 5, A)]),
    G((15, 0, 460), 6, 0, 6, 3, 0, 0, 10, [J(F1A, 6, P), J(F1B, 7, P), J(F1, 9, A), J(F1A, 14, A), J(F1B, 17, A, th_dmrs=0.4)]),
    # ---- the mixed PRB (n_rb_2 >= 1, N_cs > 0): formats 1x below the edge -- pairs with one n_cs on every data symbol of both slots and another n_oc
    # live only here -- beside formats 2x at n_pucch >= 12 n_rb_2 (the signed-x branch of the second slot)
    G((50, 0, 93), 4, 0, 2, 1, 2, 0, 20, [J(F1A, 0, P), J(F1B, 4, P), J(F2, 27, P, 5), J(F1, 1, A, meas_ta=1)]),
    G((75, 0, 124), 5, 1, 1, 1, 1, 1, 10, [J(F1B, 1, P), J(F1A, 2, P), J(F2, 14, P, 7), J(F1, 0, A), J(F2A, 22, A, 4)]),
    G((100, 0, 155), 6, 0, 1, 1, 4, 0, 10, [J(F1A, 1, P), J(F1B, 2, P), J(F2B, 53, P, 11, (1, 1)), J(F1, 0, A)]),
    G((6, 1, 217), 8, 0, 3, 1, 1, 0, 20, [J(F1A, 0, P), J(F1B, 5, P), J(F2, 16, P, 6), J(F1, 2, A), J(F2, 19, A, 7)]),
    G((15, 1, 248), 9, 1, 6, 1, 1, 1, 10, [J(F1B, 0, P), J(F1A, 11, P), J(F1A, 3, A), J(F1, 7, A), J(F2, 13, A, 5)]),
    G((25, 0, 279), 13, 0, 4, 2, 1, 0, 20, [J(F1A, 0, P), J(F1B, 4, P), J(F2, 19, P, 1), J(F1, 1, A), J(F2, 18, A, 2)]),
    G((50, 0, 310), 0, 1, 2, 1, 1, 1, 20, [J(F1B, 1, P), J(F1A, 3, P), J(F1, 0, A), J(F1A, 4, A), J(F2, 20, A, 3)]),
    G((75, 0, 44), 9, 0, 6, 2, 5, 0, 10, [J(F1A, 2, P), J(F2A, 64, P, 4, (1, 0)), J(F1B, 8, A), J(F2, 61, A, 8)]),
    # ---- formats 2x beside each other: every CQI length, every DRS value
    G((25, 0, 434), 4, 0, 0, 1, 2, 1, 20, [J(F2, 3, P, 8), J(F2, 7, P, 9), J(F2, 9, A, 10, meas_ta=1)]),
    G((50, 0, 465), 5, 0, 0, 2, 2, 0, 20, [J(F2, 13, P, 4), J(F2A, 18, P, 3, (0, 0)), J(F2, 15, A, 11)]),
    G((15, 0, 496), 6, 0, 0, 1, 1, 0, 30, [J(F2A, 2, P, 4, (1, 0)), J(F2B, 5, P, 11, (0, 1))]),
    G((75, 0, 503), 7, 0, 0, 3, 3, 1, 20, [J(F2B, 13, P, 6, (1, 0)), J(F2B, 17, P, 10, (0, 0))]),
    G((100, 0, 12), 8, 0, 0, 1, 6, 0, 10, [J(F2B, 62, P, 11, (1, 1)), J(F2, 66, P, 2), J(F2, 61, A, 4, filter_on=0)]),
    G((25, 0, 76), 19, 0, 0, 1, 1, 1, 20, [J(F2B, 4, P, 10, (0, 0)), J(F2, 9, P, 7), J(F2, 1, A, 4, meas_ta=0)]),
    G((6, 1, 108), 2, 0, 0, 1, 1, 0, 30, [J(F2, 2, P, 5), J(F2, 7, P, 6)]),
    # ---- one present user and its empty neighbours (what was sent is what is decoded)
    G((6, 0, 140), 0, 1, 0, 2, 0, 0, 20, [J(F1B, 7, P), J(F1A, 1, A, meas_ta=1), J(F1, 13, A), J(F1B, 8, A), J(F1A, 16, A)]),
    G((15, 1, 172), 1, 0, 4, 2, 1, 1, 10, [J(F1A, 9, P, filter_on=0), J(F1B, 4, A), J(F1, 10, A), J(F1A, 15, A)]),
    G((25, 0, 204), 3, 0, 3, 3, 2, 0, 10, [J(F1, 30, P, th_dmrs=0.4), J(F1A, 31, A, th_dmrs=0.4), J(F1B, 33, A), J(F1A, 27, A), J(F1B, 36, A)]),
    G((50, 0, 236), 4, 1, 0, 1, 0, 1, 20, [J(F1A, 150, P, meas_ta=0), J(F1B, 151, A), J(F1, 162, A), J(F1A, 174, A), J(F1B, 179, A)]),
    G((75, 0, 268), 5, 0, 2, 2, 3, 0, 20, [J(F2, 40, P, 7, meas_ta=0), J(F2, 44, A, 6), J(F1A, 0, A), J(F2A, 37, A, 5, th_dmrs=0.4)]),
    G((100, 0, 300), 6, 0, 0, 1, 0, 1, 30, [J(F2B, 118, P, 9, (0, 1)), J(F2, 109, A, 5), J(F2, 119, A, 1)]),
    G((6, 0, 332), 7, 1, 6, 1, 0, 0, 10, [J(F1B, 20, P), J(F1A, 2, A), J(F1, 21, A), J(F1A, 32, A), J(F1B, 44, A)]),
    G((15, 0, 364), 8, 0, 7, 1, 1, 1, 20, [J(F2, 12, P, 12), J(F1A, 3, A)]),
    G((25, 1, 396), 9, 0, 0, 3, 2, 0, 10, [J(F2, 14, P, 4, th_dmrs=0.4), J(F2, 20, A, 7), J(F2, 17, A, 12, th_dmrs=0.4)]),
    G((50, 0, 59), 11, 0, 2, 2, 0, 1, 20, [J(F1A, 10, P), J(F1B, 11, P), J(F1, 5, A), J(F1A, 17, A), J(F1B, 9, A)]),
    G((75, 1, 89), 12, 1, 0, 1, 0, 0, 20, [J(F1A, 30, P), J(F1B, 42, P), J(F1, 43, A), J(F1A, 41, A), J(F1B, 47, A)]),
    G((100, 0, 479), 15, 0, 6, 3, 3, 1, 10, [J(F1A, 0, P), J(F1B, 3, P), J(F1, 5, A), J(F1A, 2, A), J(F1B, 4, A)]),
]


def save(path, rec):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def jobs_of(M, FILTER, TH, g, spec):
    out = []
    for k, e in enumerate(spec["jobs"]):
        on = e.get("filter_on", 1)
        j = dict(zip(M.JOB_FIELDS, (e["fmt"], e["n_pucch"], spec["N_cs"], spec["delta"], spec["n_rb_2"], spec["hop"], 0x2000 + 16 * g + k, e["nbits"], e.get("meas_ta", 1), 3 if on else 0)))
        j["filter"] = [float(v) for v in FILTER] if on else [0.0, 0.0, 0.0]
        j.update(zip(M.TH_FIELDS, (float(np.float32(v)) for v in TH + (e.get("th_dmrs", 0.0),))))
        out.append(j)
    return out


IN_CONDITIONS = ("correlation", "dmrs_correlation", "pe", "z")  # the tolerances conditions() reads: drawn under gen_golden_pucch.PROVISIONAL
CAP = 9.9e-6  # the others: every stored tolerance is asserted below 1e-5


def cancelling(m):
    """None, or which float32 sum of the reference cancels.  A sum that comes to the fraction f of its terms carries a relative rounding of about
    2^-24 / f, in the reference as on a device; a relative tolerance below 1e-5 can hold such a result only down to f of a few hundredths.  An empty
    resource orthogonal to its neighbour gives such sums (its estimate, its rsrp, its correlation are what is LEFT of the neighbour); the draw keeps
    those whose results still stand a few hundredths above their terms.  Judged on the model's float64 values alone, like the ta phasor sum."""
    if np.max(np.abs(m["ce"])) < 0.05 * np.sqrt(float(m["epre"])):
        return "the slot average cancels"
    if float(m["rsrp"]) < 7e-3 * float(m["epre"]):
        return "the rsrp sum cancels"
    if not m["early"] and abs(float(m["correlation"])) < 0.015:
        return "the correlation cancels"
    return None


def sent_bits(rng, e):
    b = tuple(int(v) for v in rng.integers(0, 2, e["nbits"] if e["fmt"] >= F2 else 2))
    return {F1: (0, 0), F1A: (b[0], 0)}.get(e["fmt"], b)


def blocks_of(plans):
    """the distinct PRB pairs of a group's jobs, in order of first use"""
    prb = []
    for p in plans:
        t = (int(p["n_prb"][0]), int(p["n_prb"][1]))
        if t not in prb:
            prb.append(t)
    assert 1 <= len(prb) <= 2, prb
    return prb


def arrays(M, groups, rows):
    rec = dict(g_cell=np.array([s["cell"] for s in GROUPS], np.uint32), g_sf=np.array([(s["tti"], s["short"]) for s in GROUPS], np.uint32),
               g_cfg=np.array([(s["N_cs"], s["delta"], s["n_rb_2"], s["hop"]) for s in GROUPS], np.uint32), g_noise_db=np.array([s["noise_db"] for s in GROUPS], np.float32),
               g_seed=np.array([e["seed"] for e in groups], np.uint32), g_nblk=np.array([len(e["prb"]) for e in groups], np.uint32),
               g_prb=np.zeros((len(groups), 2, 2), np.uint32), g_cols=np.zeros((len(groups), 2, 2, 7, 12), np.complex64))
    for g, e in enumerate(groups):
        rec["g_prb"][g, :len(e["prb"])] = e["prb"]
        rec["g_cols"][g, :len(e["prb"])] = e["cols"]
    dt = dict(group=np.uint32, job=np.uint32, filter=np.float32, th=np.float32, present=np.uint8, sent=np.uint8, sent_drs=np.uint8, plan=np.uint32, outf=np.float32,
              outb=np.uint8, llr=np.int16, max_corr=np.int32, early=np.uint8, ce=np.complex64)
    rec.update({k: np.array([e[k] for e in rows], t) for k, t in dt.items()})
    return rec


def dry():
    import pucch_model as M
    import pucch_sweep as S
    from gen_golden_pucch import FILTER, TH

    groups, rows = [], []
    for g, spec in enumerate(GROUPS):
        cell, sf = dict(zip(M.CELL_FIELDS, spec["cell"])), {"tti": spec["tti"], "shortened": spec["short"]}
        jobs = jobs_of(M, FILTER, TH, g, spec)
        plans = [M.plan(cell, sf, j) for j in jobs]
        assert all(p is not None for p in plans), g
        prb = blocks_of(plans)
        groups.append(dict(seed=0, prb=prb, cols=np.zeros((len(prb), 2, 7, 12), np.complex64)))
        for j, p, e in zip(jobs, plans, spec["jobs"]):
            w = M.plan_words(p)
            rows.append(dict(group=g, job=[j[k] for k in M.JOB_FIELDS], filter=j["filter"], th=[j[k] for k in M.TH_FIELDS], present=e["present"], sent=np.zeros(13), sent_drs=e["drs"],
                             plan=w, outf=np.zeros(13), outb=np.array([0] * 13 + list(e["drs"])), llr=np.zeros(20), max_corr=0,
                             early=int(e.get("th_dmrs", 0.0) > 0 and not e["present"]), ce=np.zeros((2, 12))))
        print("group %2d: PRB pairs %s, m %s" % (g, prb, [S.m_of(t) for t in prb]))
    c = S.coverage(arrays(M, groups, rows))
    print({k: v for k, v in c.items() if k != "pairs"})
    print("pairs:", [(k, g) for k, g, _, _ in c["pairs"]])


def main():
    import pucch_model as M
    import pucch_sweep as S
    from gen_golden_pucch import FILTER, PROVISIONAL, TH, conditions, distances, draw, load_wrapper, run_reference, words

    quantities = M.FLOATS + ("ce", "z", "z_f1", "pe")
    tol = {k: PROVISIONAL.get(k, PROVISIONAL["other"]) if k in IN_CONDITIONS else CAP for k in quantities}
    worst, where = {k: 0.0 for k in quantities}, {}
    groups, rows, failed, survey = [], [], [], "--survey" in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        L = load_wrapper(tmp)
        for g, spec in enumerate(GROUPS):
            cell, sf = dict(zip(M.CELL_FIELDS, spec["cell"])), {"tti": spec["tti"], "shortened": spec["short"]}
            nsymb = 6 if cell["cp"] else 7
            jobs = jobs_of(M, FILTER, TH, g, spec)
            assert L.pucch_ref_open(*spec["cell"]) == 0
            plans, pws = [], []
            for j in jobs:  # the reference's own plan, and the model's against it
                p, pw = M.plan(cell, sf, j), np.zeros(65, np.uint32)
                assert p is not None and L.pucch_ref_plan(words(M, j, sf).ctypes.data, pw.ctypes.data) == 0, (g, j)
                mw = M.plan_words(p)
                if j["format"] >= M.F2:
                    mw[37:47] = 0  # n_prime of formats 2x is not exposed by the reference
                assert np.array_equal(mw, pw), (g, j, mw, pw)
                plans.append(p)
                pws.append(pw)
            prb = blocks_of(plans)
            n_present = sum(e["present"] for e in spec["jobs"])
            why = "never drawn"
            for attempt in range(20):
                seed = 50000 + 100 * g + attempt
                rng = np.random.default_rng(seed)
                sent = [sent_bits(rng, e) for e in spec["jobs"]]
                cols = np.zeros((len(prb), 2, 7, 12), np.complex128)
                for j, p, e, b in zip(jobs, plans, spec["jobs"], sent):
                    if e["present"]:
                        cols[prb.index((int(p["n_prb"][0]), int(p["n_prb"][1])))] += draw(L, M, rng, cell, sf, j, p, b, e["drs"], USER_SNR_DB)
                sigma = 10 ** (-spec["noise_db"] / 20) / np.sqrt(2)
                cols[:, :, :nsymb] += sigma * (rng.standard_normal((len(prb), 2, nsymb, 12)) + 1j * rng.standard_normal((len(prb), 2, nsymb, 12)))
                cols = cols.astype(np.complex64)
                grid = S.build_grid(seed, cell, np.array(prb), cols)
                refs, ms = [], []
                for j, p in zip(jobs, plans):
                    refs.append(run_reference(L, M, cell, sf, j, grid))
                    ms.append(M.decode(grid, cell, sf, j, p))
                whys = [conditions(M, j, m, tol) or cancelling(m) for j, m in zip(jobs, ms)]
                why = "; ".join("job %d: %s" % (k, w) for k, w in enumerate(whys) if w is not None) or None
                if why is None:
                    break
                print("group %2d draw %d: %s" % (g, attempt, why))
            if why is not None and survey:  # --survey: go on to the other groups, write nothing
                failed.append(g)
                continue
            assert why is None, (g, why)
            groups.append(dict(seed=seed, prb=prb, cols=cols))
            for k, (j, p, pw, e, b, ref, m) in enumerate(zip(jobs, plans, pws, spec["jobs"], sent, refs, ms)):
                o, name = ref["outf"], "group %d job %d" % (g, k)
                # the model's decisions are the reference's
                assert bool(o[0]) == m["detected"] and bool(o[3]) == m["ack_valid"] and np.array_equal(ref["outb"][:13], m["pucch_bits"]), (name, o, m["pucch_bits"], ref["outb"])
                assert list(ref["outb"][13:]) == [m["drs"] % 2, m["drs"] // 2] and np.array_equal(ref["llr"], m["llr"]) and ref["max_corr"] == m["max_corr"], name
                assert abs(float(o[12]) - float(m["ta_us"])) < 0.01, (name, o[12], m["ta_us"])
                if n_present == 1 and e["present"]:  # alone on the grid: what was sent is what is decoded
                    assert not m["early"], name
                    want = list(b[:e["nbits"]]) if e["fmt"] >= F2 else list(b[:{F1: 0, F1A: 1, F1B: 2}[e["fmt"]]])
                    assert bool(o[0]) and list(ref["outb"][:len(want)]) == want and list(ref["outb"][13:]) == list(e["drs"]), (name, ref["outb"], want)
                dist = distances(M, p, j, ref, m)
                dist["z_f1" if e["fmt"] < F2 else "z"], dist["z" if e["fmt"] < F2 else "z_f1"] = dist["z"], 0.0
                for q in worst:
                    if dist[q] > worst[q]:
                        worst[q], where[q] = dist[q], name
                rows.append(dict(group=g, job=[j[q] for q in M.JOB_FIELDS], filter=j["filter"], th=[j[q] for q in M.TH_FIELDS], present=e["present"],
                                 sent=list(b) + [0] * (13 - len(b)), sent_drs=e["drs"], plan=pw, outf=o, outb=ref["outb"], llr=ref["llr"], max_corr=ref["max_corr"],
                                 early=int(m["early"]), ce=np.stack([ref["ce"][s * nsymb, 12 * p["n_prb"][s]:12 * p["n_prb"][s] + 12] for s in range(2)])))
                print("group %2d job %d fmt %d n_pucch %3d %s: det %d corr %.4f dmrs %.4f early %d" % (g, k, e["fmt"], e["n_pucch"], "present" if e["present"] else "absent ",
                                                                                                     o[0], o[1], o[2], m["early"]))
            print("group %2d: draw %d, PRB pairs %s" % (g, attempt, prb), flush=True)
    final = {k: 4.0 * v for k, v in worst.items()}
    print("tolerances:", {k: "%.3g (%s)" % (v, where[k]) for k, v in final.items()})
    if survey:
        sys.exit("groups that found no draw: %s" % failed)
    assert all(0 < v <= tol[k] and v < 1e-5 for k, v in final.items()), "a stored tolerance is above the provisional value the draws used"
    rec = arrays(M, groups, rows)
    rec["tol_names"] = np.array(sorted(final))
    rec["tol"] = np.array([final[k] for k in sorted(final)], np.float64)
    c = S.coverage(rec)
    print({k: v for k, v in c.items() if k != "pairs"}, "pairs:", [(k, g) for k, g, _, _ in c["pairs"]])
    save(OUT, rec)
    # with the record in place: every job again through the public loader, conditions under the stored tolerances
    S._rec = None
    for g in range(S.n_groups()):
        cell, sf, jobs, grid, idx = S.group(g)
        for j in jobs:
            m = M.decode(grid, cell, sf, j)
            assert conditions(M, j, m, final) is None and cancelling(m) is None, (g, j)
    size = os.path.getsize(OUT)
    assert size < 400000, size
    print("wrote %s (%d groups, %d jobs, %d bytes)" % (OUT, len(groups), len(rows), size))


if __name__ == "__main__":
    dry() if "--dry" in sys.argv[1:] else main()
