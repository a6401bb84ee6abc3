"""The inputs of the PRACH size sweep (tests/prach_sizes.py: D = 4, 6, 8, 8, 12 and 12 streams, three occasions each, one of them with the wanted bins
wrapping past the end of the transform) on the double-precision model alone: prach_model.preamble() held once to the record of the reference (the recorded
occasions rebuilt from what was sent give the recorded detections), and for every size the rules tools/gen_golden_prach.py asserts on the reference
(prach_model.margins, with the stored tolerances): the model detects exactly what was sent, every window peak lies more than 100 tolerances from the
threshold, every reported peak leads its window's runner-up by more than 100 tolerances, the phase form's sample count is more than 0.05 from a
half-integer.  So the device test that stands on these inputs (tests/test_gpu_prach_sizes.py) can ask for exact detections.  Runs on the CPU."""
import numpy as np
import pytest

import prach_model as M
import prach_sizes as Z
from test_prach_golden import case, names, tol

QUANT = ("spec", "bins", "corr", "ave", "cross", "pv", "p2a")
# what tools/gen_golden_prach.py sent in its recorded cases: (preamble or ("root", i), delay in samples, gain in dB)
RECORDED_TX = {"6prb_zcz0_roots_12db": [(5, 3, 0.0), (40, 11, -12.0)], "6prb_zcz1_neighbours_first_last": [(10, 0, 0.0), (11, 22, 0.0)],
               "6prb_zcz11": [(63, 20, 0.0), (12, 5, -3.0)], "6prb_zcz15_phase": [(0, 17, 0.0), (3, 40, 0.0)], "6prb_noise_only": [], "6prb_nra4": [(2, 7, 0.0)],
               "6prb_factor": [(9, 30, 0.0)], "15prb_fo3_format1_phase": [(20, 9, 0.0)], "25prb_hs_fo2_format3": [(("root", 1), 6, 0.0), (("root", 7), 30, -6.0)],
               "100prb_standard_fo40": [(30, 200, 0.0), (7, 50, -6.0)]}
RECORDED_NOISE = {"6prb_factor": 0.5}


@pytest.mark.parametrize("c", range(len(names())), ids=names())
def test_preamble_rebuilds_the_recorded_occasions(c):
    """the signal from `sent` and the case's delays, through M.detect: the recorded detections"""
    g = case(c)
    cfg, p = g["cfg_dict"], M.plan(g["cfg_dict"], g["info_dict"]["N_ifft_ul"])
    n, tx = p["N_ifft_prach"], RECORDED_TX[names()[c]]
    assert len(tx) == g["sent"].size
    rng = np.random.default_rng(100 + c)
    sig, rms = np.zeros(n, np.complex128), None
    for (_, delay, gain), sent in zip(tx, g["sent"]):
        root, win = int(sent) // p["n_wins"], int(sent) % p["n_wins"]  # restricted sets: the first preamble of a root, whose shift is 0
        x = M.preamble(p, cfg["nof_prb"], int(g["fo"]), p["root_u"][root], win * p["N_cs"], delay)
        rms = rms or float(np.sqrt(np.mean(np.abs(x) ** 2)))
        sig += x * 10.0 ** (gain / 20.0)
    rms = rms or 1.0 / np.sqrt(n)
    sig += RECORDED_NOISE.get(names()[c], 0.05) * rms / np.sqrt(2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    _, _, roots, (ind, toff, _) = M.detect(cfg, int(g["fo"]), sig.astype(np.complex64), g["factor_used"], n_ifft_ul=g["info_dict"]["N_ifft_ul"])
    assert np.array_equal(ind, g["ind"])
    if not cfg["freq_domain_offset_calc"]:  # whole-sample delays: the peak offsets, and so t_offsets, are the recorded ones whatever the noise
        assert np.array_equal(np.array([r[4] for r in roots])[g["ind"] // p["n_wins"], g["ind"] % p["n_wins"]], g["po"][g["ind"] // p["n_wins"], g["ind"] % p["n_wins"]])
        assert toff.tobytes() == g["toff"].tobytes()


def test_the_sizes_are_the_untested_stream_counts():
    seen = []
    for size in Z.SIZES:
        p = M.plan(Z.cfg_of(size), M.symbol_sz(*size))
        seen.append(p["N_ifft_prach"] // 1536)
        assert p["N_ifft_ul"] // 128 == Z.D_OF[size] == seen[-1] and (p["N_cs"], p["n_wins"], p["num_ra_preambles"]) == (119, 7, 4) and p["N_roots"] >= 4
        fos = Z.freq_offsets(size)
        assert [Z.wraps(p, size[0], fo) for fo in fos] == [False, True, False]
        assert not Z.wraps(p, size[0], fos[1] - 1)  # the FIRST wrapping one
        assert all(len({s // 7 for s in sent}) == 2 for _, _, sent in Z.occasions(size))  # two preambles of different roots
    assert sorted(seen) == [4, 6, 8, 8, 12, 12] and sum(Z.cfg_of(s)["freq_domain_offset_calc"] for s in Z.SIZES) == 1


@pytest.mark.parametrize("size", Z.SIZES, ids=[Z.name(s) for s in Z.SIZES])
def test_margins_on_the_model(size):
    cfg, n_ul = Z.cfg_of(size), M.symbol_sz(*size)
    t = {q: tol(q) for q in QUANT}
    for o, (fo, sig, sent) in enumerate(Z.occasions(size)):
        p, _, roots, (ind, toff, p2a) = M.detect(cfg, fo, sig, 18.0, n_ifft_ul=n_ul)
        rec = dict(ind=ind, sent=np.array(sent), ave=np.array([r[1] for r in roots]), cross=np.array([r[2] for r in roots]), pv=np.stack([r[3] for r in roots]),
                   po=np.stack([r[4] for r in roots]))
        aux = dict(f=np.float32(18.0), p=p, corr_all=np.stack([r[0] for r in roots]), n_wins=p["n_wins"], N_cs=p["N_cs"])
        M.margins(dict(name="%s occasion %d" % (Z.name(size), o), cfg=tuple(cfg[k] for k in M.CFG_FIELDS)), rec, aux, t)
        assert [int(v) for v in ind] == sent and toff.size == 2 and np.all(p2a > 18.0)
