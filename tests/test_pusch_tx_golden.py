"""tests/pusch_tx_model.py against the reference's own record (tests/golden/pusch_tx_ref.npz, tools/gen_golden_pusch_tx.py: srsran_ulsch_encode and
srsran_sequence_pusch_apply_pack on seeded grants), bit for bit, and against the literal de-multiplexer the receive tests use.  CPU only: the record and the
restatements agree here before anything runs on a device."""
import os

import numpy as np
import pytest

import oracle_api as O
import pusch_tx_model as M
from test_gpu_pusch_uci import _literal_demux

REC = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pusch_tx_ref.npz"))
NAMES = [str(n) for n in REC["names"]]


@pytest.fixture(scope="module")
def restated():
    """the model's srsran_ulsch_encode stage for every recorded case, computed once: name -> dict"""
    out = {}
    for i, (mod, tbs, rv, L_prb, cols, Qa, Qr, Qc) in enumerate(REC["cases"].tolist()):
        Qm = O.QM[mod]
        H = cols * 12 * L_prb
        types = REC["type_%d" % i]
        ri, ack = types[:Qr * Qm], types[Qr * Qm:]
        cqi = np.unpackbits(REC["cqi_%d" % i])[:Qc * Qm]
        e, _ = O.tb_coded_bits(tbs, Qm, (H - Qr - Qc) * Qm, rv, None, payload=np.unpackbits(REC["pay_%d" % i]), tx_order=True)
        q, lst = M.ulsch_encode(e, cqi, ri, ack, H, cols, Qm)
        out[NAMES[i]] = dict(i=i, Qm=Qm, H=H, cols=cols, counts=(Qa, Qr, Qc), e=e, ri=ri, ack=ack, cqi=cqi, q=q, lst=lst, seed=int(REC["seeds"][i]))
    return out


def test_record_covers_what_it_should():
    c = REC["cases"]
    kinds = [np.bincount(REC["type_%d" % i], minlength=4) for i in range(len(NAMES))]
    assert any(k[2] for k in kinds) and any(k[3] for k in kinds)  # repetition and placeholder types
    assert set(c[:, 0]) == {1, 2, 3} and {9, 10, 11, 12} <= set(c[:, 4]) and 2 in set(c[:, 2])
    assert (c[:, 5] > 0).any() and (c[:, 6] > 0).any() and (c[:, 7] > 0).any() and ((c[:, 5] > 0) & (c[:, 6] > 0) & (c[:, 7] > 0)).any()
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pusch_tx_ref.npz")) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_model_gives_the_recorded_bits(restated, name):
    r = restated[name]
    i = r["i"]
    assert np.array_equal(np.array([p for p, _ in r["lst"]], np.uint32), REC["pos_%d" % i])  # the positions, in list order
    assert np.array_equal(np.array([t for _, t in r["lst"]], np.uint8), REC["type_%d" % i])
    assert np.array_equal(np.packbits(r["q"]), REC["q_%d" % i])  # srsran_ulsch_encode's q_bits
    scr, fixed = M.scramble_and_fix(r["q"], r["lst"], r["seed"])
    assert np.array_equal(np.packbits(scr), REC["scr_%d" % i])  # srsran_sequence_pusch_apply_pack of them
    # the fix-up touches nothing but the listed positions
    listed = np.zeros(scr.size, bool)
    listed[[p for p, _ in r["lst"]]] = True
    assert np.array_equal(scr[~listed], fixed[~listed])


@pytest.mark.parametrize("name", NAMES)
def test_model_round_trip_through_the_literal_demultiplexer(restated, name):
    """what the model multiplexed comes back from the receive side's literal de-multiplexer (tests/test_gpu_pusch_uci.py): e bits, CQI bits, RI and ACK bits"""
    r = restated[name]
    Qm, H, cols = r["Qm"], r["H"], r["cols"]
    Qa, Qr, Qc = r["counts"]
    soft = (2 * r["q"].astype(np.int16) - 1) * 100
    ack, ackp, ri, rip, cqi, e, g = _literal_demux(soft, H, cols, Qm, Qa, Qr, Qc)
    assert np.array_equal(ack > 0, r["ack"] == 1) and np.array_equal(ri > 0, r["ri"] == 1)  # a bit of type 1 is sent as 1, every other type as 0
    assert np.array_equal(ackp, [p for p, _ in r["lst"][Qr * Qm:]]) and np.array_equal(rip, [p for p, _ in r["lst"][:Qr * Qm]])
    sent = np.concatenate([r["cqi"], r["e"]])
    got = np.concatenate([cqi, e])
    first = 1 if Qr > 0 else 0  # with RI symbols g[0] holds the soft bit of the highest RI position (vector.c:141-146 on the table of sch.c:660-681)
    there = got != 0             # an ACK symbol punctures the stream and leaves zeros
    there[:first] = False
    assert np.array_equal(got[there] > 0, sent[there] == 1)
    assert (got[first:] == 0).sum() == Qa * Qm
