"""The numpy model of PBCH decoding (tests/pbch_model.py) against what the reference gave (tests/golden/pbch_ref.npz, tools/gen_golden_pbch.py): the RE map
exact; the decode stage bit-exact (the bits of rm_f, the 40 decoded bits, the verdicts) for every combination of frame_idx 1 .. 4; the call sequences with
their decisions and state exact and their floats within the stored tolerances.  CPU only."""
import os

import numpy as np
import pytest

import oracle_api as O
import pbch_model as PB


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(O.ROOT, "tests", "golden", "pbch_ref.npz"))


def rel(a, b):
    return float(np.abs(np.asarray(a).astype(np.complex128) - b).max()) / float(np.sqrt(np.mean(np.abs(np.asarray(b, np.complex128)) ** 2)))


def test_map_is_exact(golden):
    cells = [PB.from_row(r) for r in golden["m_cells"]]
    assert {(c["nof_prb"], c["id"] % 3, c["cp_nsymb"]) for c in cells} == {(p, o, cp) for p in (6, 15, 25) for o in (0, 1, 2) for cp in (7, 6)}
    for i, c in enumerate(cells):
        t = golden["m_table_%d" % i]
        assert t.size == PB.nof_re(c) and np.array_equal(PB.table(c), t), c
        rows = t // (12 * c["nof_prb"])
        assert [int((rows == r).sum()) for r in range(4)] == ([48, 48, 72, 72] if c["cp_nsymb"] == 7 else [48, 48, 72, 48]), c


def test_hypothesis_lists():
    assert [len(PB.combos(f)) for f in (1, 2, 3, 4)] == [4, 11, 20, 30]
    assert PB.combos(2)[:5] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0)] and PB.combos(4)[-1] == (3, 0, 0)
    assert PB.nant_list(PB.cell(6, 0, 1)) == [1, 2, 4] and PB.nant_list(PB.cell(6, 4, 1)) == [4]


def test_fast_dematcher_is_the_written_one():
    import conv_model as CM

    rng = np.random.default_rng(5)
    x = rng.standard_normal(1920).astype(np.float32)
    x[rng.permutation(1920)[:700]] = CM.RX_NULL
    x[:480] = CM.RX_NULL
    assert np.array_equal(PB.rm_rx_fast(x).view(np.uint32), CM.rm_rx(x, 120).view(np.uint32))


def test_stage_cases_are_bit_exact(golden):
    seen = set()
    for i, name in enumerate(golden["t_names"]):
        c, f, llr = PB.from_row(golden["t_cell_%d" % i]), int(golden["t_f_%d" % i]), golden["t_llr_%d" % i]
        rows = PB.try_frames(c, llr, f)
        assert len(rows) == len(PB.combos(f)) == len(golden["t_hit_%d" % i])
        for j, r in enumerate(rows):
            assert np.array_equal(r["rm_f"].view(np.uint32), golden["t_rm_f_%d" % i][j].view(np.uint32)), (name, j)
            assert np.array_equal(r["bits"], golden["t_data_%d" % i][j]) and PB.verdict(r, 1) == bool(golden["t_hit_%d" % i][j]), (name, j)
        seen.add((f, c["cp_nsymb"]))
    assert {(1, 7), (2, 7), (3, 7), (4, 7), (4, 6)} <= seen


def test_call_sequences(golden):
    seqs = PB.record_sequences(golden)
    d_tol, llr_tol = float(golden["d_tol"]), float(golden["llr_tol"])
    assert 0 < d_tol < 1e-4 and 0 < llr_tol < 1e-4
    hits = 0
    for s in seqs:
        c = s["cell"]
        for i, call in enumerate(s["calls"]):
            res, st, dbg = PB.decode(c, PB.state_before(c, s, i), call["rx_rows"], call["ce_rows"], float(call["noise"]))
            tag = (s["name"], i)
            assert (res["ret"], res["nof_tx_ports"], res["sfn_offset"]) == (int(call["ret"]), int(call["ports"]), int(call["off"])), tag
            assert (res["nb"], res["dst"], res["src"]) == tuple(int(v) for v in call["comb"]) and np.array_equal(res["payload"], call["payload"]), tag
            assert st["frame_idx"] == int(call["f_out"]), tag
            f_out = int(call["f_out"])
            for r in range(f_out):  # the rows a later call reads
                assert rel(st["llr"][r], call["llr"][r]) <= llr_tol, (tag, r)
            assert rel(dbg["d"][int(call["d_nant"])], call["d"]) <= d_tol, tag
            hits += res["ret"]
    assert hits >= 12
