"""The second record of the reference's PUCCH receive side, tests/golden/pucch_sweep_ref.npz (tools/gen_golden_pucch_sweep.py; loaded by tests/pucch_sweep.py):
what it covers -- every cell size, both prefixes, 20 and more base-sequence groups, hopping, every subframe, two and three users on one PRB told apart by
n_oc or by n_cs alone, empty resources beside occupied ones, the mixed PRB, every CQI length -- and the float64 model against it, job by job: the plan
words exact, decisions, bits, DRS bits and soft bits exact, floats within the tolerances the generator measured on these jobs.  No device, no library."""
import os

import numpy as np
import pytest

import pucch_model as M
import pucch_sweep as S
from test_pucch_golden import check_record


def tol(name):
    return S.tolerances()[name]


def test_the_sweep_covers_what_it_should():
    r = S.record()
    c = S.coverage(r)
    assert c["groups"] <= 40 and c["jobs"] <= 250 and os.path.getsize(S.GOLDEN) < 400000
    # a pair that shares n_cs with n_oc 1 against n_oc 2 on an unshortened slot: what a swapped row of the cover table would hit
    plan = r["plan"].astype(int)
    assert any(k == "n_oc" and {plan[a, 27], plan[b, 27]} == {1, 2} and plan[a, 5] == 4 for k, _, a, b in c["pairs"])


def test_stored_tolerances_are_well_formed():
    t = S.tolerances()
    assert set(t) == set(M.FLOATS) | {"ce", "pe", "z", "z_f1"} and all(0 < v < 1e-5 for v in t.values())
    r = S.record()
    assert set(np.unique(r["g_noise_db"])) == {10.0, 20.0, 30.0} and set(np.unique(r["present"])) == {0, 1}
    for g in range(S.n_groups()):  # a group's jobs share its (N_cs, delta_pucch_shift, n_rb_2, group_hopping_en) and lie on its blocks
        cell, sf, jobs, _, rows = S.group(g)
        blocks = {tuple(int(v) for v in b) for b in r["g_prb"][g][:int(r["g_nblk"][g])]}
        assert {tuple(int(v) for v in r["plan"][i][1:3]) for i in rows} == blocks, g


@pytest.mark.parametrize("g", range(S.n_groups()))
def test_model_equals_the_sweep(g):
    cell, sf, jobs, grid, rows = S.group(g)
    for k, (j, i) in enumerate(zip(jobs, rows)):
        e, p = S.entry(i), M.plan(cell, sf, j)
        w = M.plan_words(p)
        if j["format"] >= M.F2:
            w[37:47] = 0  # n' of formats 2x is not exposed by the reference
        assert np.array_equal(w, e["plan"]), (g, k)
        m = M.decode(grid, cell, sf, j, p)
        assert m["max_corr"] == int(e["max_corr"]) and bool(m["early"]) == bool(e["early"]), (g, k)
        check_record(e, j, p, m, "group %d job %d" % (g, k), tol)


def test_a_single_present_user_is_decoded_as_sent():
    r = S.record()
    seen = 0
    for g in range(S.n_groups()):
        rows = np.nonzero(r["group"] == g)[0]
        mine = [i for i in rows if r["present"][i]]
        if len(mine) != 1:
            continue
        i, fmt = mine[0], int(r["job"][mine[0]][0])
        n = int(r["job"][i][7]) if fmt >= M.F2 else {M.F1: 0, M.F1A: 1, M.F1B: 2}[fmt]
        assert r["outf"][i][0] == 1 and np.array_equal(r["outb"][i][:n], r["sent"][i][:n]) and np.array_equal(r["outb"][i][13:], r["sent_drs"][i]), g
        seen += 1
    assert seen >= 5
