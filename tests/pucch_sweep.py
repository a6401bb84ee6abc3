"""The second record of the reference's PUCCH receive side, tests/golden/pucch_sweep_ref.npz (tools/gen_golden_pucch_sweep.py): GROUPS of jobs that share one
received grid.  A group is one cell, one subframe, one (N_cs, delta_pucch_shift, n_rb_2, group_hopping_en) and up to two PRB pairs that carry the summed
signals of the jobs marked present, plus noise; every job of the group, present or absent, was decoded by the reference on that grid.  This module loads
the record (group(g) -> cell, subframe, jobs, grid, row numbers) and states what the record has to cover (coverage)."""
import os

import numpy as np

import pucch_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pucch_sweep_ref.npz")
PER_JOB = ("plan", "ce", "llr", "outf", "outb", "max_corr", "early", "present", "sent", "sent_drs")

_rec = None


def record():
    global _rec
    if _rec is None:
        _rec = dict(np.load(GOLDEN))
    return _rec


def tolerances(r=None):
    r = record() if r is None else r
    return {str(k): float(v) for k, v in zip(r["tol_names"], r["tol"])}


def n_groups():
    return record()["g_cell"].shape[0]


def build_grid(seed, cell, prb, cols):
    """pucch_model.full_grid with the group's blocks.  prb [n, 2]: the PRB of each slot; cols [n, 2, 7, 12]"""
    nsymb = 6 if cell["cp"] else 7
    g = M.full_grid(seed, cell["nof_prb"], nsymb, prb[0], cols[0][:, :nsymb])
    for b in range(1, len(prb)):
        for s in range(2):
            g[s * nsymb:(s + 1) * nsymb, 12 * prb[b][s]:12 * prb[b][s] + 12] = cols[b][s][:nsymb]
    return np.ascontiguousarray(g)


def job_of(r, i):
    j = dict(zip(M.JOB_FIELDS, (int(v) for v in r["job"][i])))
    j["filter"] = [float(v) for v in r["filter"][i]]
    j.update(zip(M.TH_FIELDS, (float(v) for v in r["th"][i])))
    return j


def group(g, r=None):
    """(cell, sf, jobs, grid, rows): rows are the jobs' row numbers in the per-job arrays of the record"""
    r = record() if r is None else r
    cell = dict(zip(M.CELL_FIELDS, (int(v) for v in r["g_cell"][g])))
    sf = {"tti": int(r["g_sf"][g][0]), "shortened": int(r["g_sf"][g][1])}
    rows = [int(i) for i in np.nonzero(r["group"] == g)[0]]
    n = int(r["g_nblk"][g])
    grid = build_grid(int(r["g_seed"][g]), cell, r["g_prb"][g][:n].astype(int), r["g_cols"][g][:n])
    return cell, sf, [job_of(r, i) for i in rows], grid, rows


def entry(i, r=None):
    r = record() if r is None else r
    return {k: r[k][i] for k in PER_JOB}


def m_of(n_prb):
    """m of srsran_pucch_n_prb from the two PRB indices it gave"""
    return 2 * int(min(n_prb)) + int(n_prb[0] > n_prb[1])


def pairs(r):
    """the pairs of PRESENT format-1x jobs of one group on one PRB pair, read off the reference's plan words: (kind, group, row a, row b) with kind
    "n_oc" -- the same n_cs on every data symbol of both slots, another n_oc on every one -- or "n_cs" -- the same n_oc on every one, another n_cs"""
    out = []
    plan = r["plan"].astype(int)
    for g in range(r["g_cell"].shape[0]):
        rows = [int(i) for i in np.nonzero((r["group"] == g) & (r["present"] == 1) & (r["job"][:, 0] <= M.F1B))[0]]
        for x, a in enumerate(rows):
            for b in rows[x + 1:]:
                if tuple(plan[a, 1:3]) != tuple(plan[b, 1:3]):
                    continue
                used = np.concatenate([np.arange(5) < plan[a, 5], np.arange(5) < plan[a, 6]])
                cs_a, cs_b, oc_a, oc_b = plan[a, 17:27][used], plan[b, 17:27][used], plan[a, 27:37][used], plan[b, 27:37][used]
                if np.all(cs_a == cs_b) and np.all(oc_a != oc_b):
                    out.append(("n_oc", g, a, b))
                if np.all(oc_a == oc_b) and np.all(cs_a != cs_b):
                    out.append(("n_cs", g, a, b))
    return out


def coverage(r):
    """what the sweep has to cover, asserted on the record (or on the generator's arrays before it writes them)"""
    G, J = r["g_cell"].shape[0], r["job"].shape[0]
    assert G >= 30 and J >= 150, (G, J)
    cell, sf, cfg, job, grp, plan = r["g_cell"].astype(int), r["g_sf"].astype(int), r["g_cfg"].astype(int), r["job"].astype(int), r["group"].astype(int), r["plan"].astype(int)
    present, fmt = r["present"] == 1, job[:, 0]
    # cells
    assert set(cell[:, 0]) == {6, 15, 25, 50, 75, 100} and set(cell[:, 1]) == {0, 1}
    assert len(set(cell[:, 2] % 30)) >= 20 and {0, 29} <= set(cell[:, 2] % 30) and len(set(cell[:, 2] // 30)) >= 8
    assert 3 * int(np.sum(cfg[:, 3] == 1)) >= G and np.all(job[:, 5] == cfg[grp, 3])
    # subframes
    assert set(range(10)) <= set(sf[:, 0]) and np.any(sf[:, 0] >= 10)
    f1 = fmt <= M.F1B
    assert set(sf[grp[f1], 1]) == {0, 1}
    # formats, DRS values (as the reference decided them for the present jobs)
    assert set(fmt) == set(range(6))
    drs = {f: {tuple(int(v) for v in r["outb"][i][13:]) for i in np.nonzero((fmt == f) & present & (r["early"] == 0))[0]} for f in (M.F2A, M.F2B)}
    assert drs[M.F2A] == {(0, 0), (1, 0)} and drs[M.F2B] == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for d in (1, 2, 3):
        assert np.any((cfg[:, 1] == d) & (cfg[:, 0] == 0)) and np.any((cfg[:, 1] == d) & (cfg[:, 0] > 0)), d
    assert np.all(job[:, 2] == cfg[grp, 0]) and np.all(job[:, 3] == cfg[grp, 1]) and np.all(job[:, 4] == cfg[grp, 2])
    # PRB position
    m = np.array([m_of(plan[i, 1:3]) for i in range(J)])
    assert len(set(grp[m >= 4])) >= 3
    assert np.any((cell[grp, 0] == 100) & (plan[:, 1:3].max(axis=1) >= 95) & (m >= 4))
    # users sharing a PRB
    shared, absent_beside = 0, 0
    for g in range(G):
        rows = np.nonzero(grp == g)[0]
        blocks = {}
        for i in rows:
            blocks.setdefault(tuple(plan[i, 1:3]), []).append(bool(present[i]))
        assert 1 <= len(blocks) <= 2 and len(blocks) == int(r["g_nblk"][g]), g
        shared += any(sum(v) >= 2 for v in blocks.values())
        absent_beside += sum(len(v) - sum(v) for v in blocks.values() if any(v))
    assert 2 * shared >= G and absent_beside >= 20, (shared, absent_beside)
    pr = pairs(r)
    for kind in ("n_oc", "n_cs"):
        mine = [p for p in pr if p[0] == kind]
        assert len(mine) >= 4, (kind, mine)
        assert any(sf[p[1], 1] == 1 for p in mine) and any(cell[p[1], 1] == 1 for p in mine), kind  # the N_sf = 3 cover, the extended prefix
    # one PRB pair with formats 1x below the c N_cs / delta edge and formats 2x at n_pucch >= 12 n_rb_2, both present
    mixed = 0
    for g in range(G):
        if cfg[g, 2] >= 1 and cfg[g, 0] > 0:
            rows = np.nonzero((grp == g) & present)[0]
            edge = (2 if cell[g, 1] else 3) * cfg[g, 0] // cfg[g, 1]
            lo = {tuple(plan[i, 1:3]) for i in rows if fmt[i] <= M.F1B and job[i, 1] < edge}
            hi = {tuple(plan[i, 1:3]) for i in rows if fmt[i] >= M.F2 and job[i, 1] >= 12 * cfg[g, 2]}
            mixed += bool(lo & hi)
    assert mixed >= 2, mixed
    # CQI lengths
    nbits = job[fmt == M.F2, 7]
    assert set(range(1, 13)) <= set(nbits) and all(int(np.sum(nbits == n)) >= 2 for n in (5, 6, 7))
    # settings
    th = np.round(r["th"][:, 3].astype(np.float64), 3)
    assert np.sum(job[:, 9] == 0) >= 2 and np.sum(job[:, 8] == 0) >= 2 and np.any((th == 0.4) & (r["early"] == 1)) and np.any((th == 0.4) & (r["early"] == 0))
    return dict(groups=G, jobs=J, shared=shared, absent_beside=absent_beside, pairs=pr, mixed=mixed)
