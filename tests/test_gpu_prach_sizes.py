"""PRACH detection on the device at the stream counts D = N_ifft_ul / 128 that tests/golden/prach_ref.npz does not hold -- D = 4 (25 PRB standard), 6 (50),
8 (50 standard, 75), 12 (75 standard, 100): the default symbol sizes of the 50, 75 and 100 PRB cells among them -- and, at each, an occasion whose 839
wanted bins wrap past the end of the transform.  The inputs are those of tests/prach_sizes.py; the reference is the double-precision model, which
tools/gen_golden_prach.py --check-sizes held to the reference itself on exactly these signals (profiles/prach_sizes_model_vs_ref.txt: every deviation
within the stored tolerances) and whose margins tests/test_prach_sizes.py asserts.  bins, corr, corr_ave, the cross sum, the window peaks and peak_to_avg
within the stored tolerances; peak offsets, the detections, their order and t_offsets EXACT; the plain call and _detect_multi of the three occasions give
the _dbg call's bits; the first and the last searched root's spectrum."""
import numpy as np
import pytest

import prach_model as M
import prach_sizes as Z
from test_gpu_prach import Handle, same
from test_prach_abi import set_order
from test_prach_golden import INFO, rel, tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0 and set_order(lib) == 0
    return lib


@pytest.mark.parametrize("size", Z.SIZES, ids=[Z.name(s) for s in Z.SIZES])
def test_every_stream_count_and_the_wrap(L, size, capfd):
    cfg, n_ul = Z.cfg_of(size), M.symbol_sz(*size)
    h = Handle(L, dict(standard=size[1], cfg_dict=cfg, factor=0.0))
    try:
        p = M.plan(cfg, n_ul)
        assert {k: getattr(h.info, k) for k in INFO} == {k: p[k] for k in INFO}
        for i in (0, h.R - 1):
            want = M.root_spectrum(p["root_u"][i])
            assert rel(h.spectrum(i), want, np.abs(want).max()) <= tol("spec"), i
        singles = []
        for o, (fo, sig, sent) in enumerate(Z.occasions(size)):
            sig = np.array(sig)
            _, mb, mroots, (mind, mtoff, mp2a) = M.detect(cfg, fo, sig, 18.0, n_ifft_ul=n_ul)
            (ind, toff, p2a), d = h.detect(fo, sig, dbg=True)
            plain, _ = h.detect(fo, sig)
            assert same(plain, (ind, toff, p2a)), o  # the _dbg call is the call
            singles.append((ind, toff, p2a))
            devs = dict(bins=rel(d["bins"], mb, np.abs(mb).max()), corr=max(rel(d["corr"][i], mroots[i][0], mroots[i][0].max()) for i in range(h.R)),
                        ave=max(abs(d["ave"][i] - mroots[i][1]) / mroots[i][1] for i in range(h.R)),
                        cross=max(abs(d["cross"][i] - mroots[i][2]) / mroots[i][1] for i in range(h.R)),
                        pv=max(rel(d["pv"][i], mroots[i][3], mroots[i][0].max()) for i in range(h.R)), p2a=float(np.max(np.abs(p2a - mp2a[:p2a.size]) / mp2a[:p2a.size])) if p2a.size else 0.0)
            with capfd.disabled():
                print(Z.name(size), "fo", fo, {q: "%.3g of %.3g" % (v, tol(q)) for q, v in devs.items()}, "detections", ind, mind)
            assert devs["bins"] <= tol("bins"), (o, fo, devs["bins"], tol("bins"))  # first: a wrong wrap or stride shows here
            assert np.array_equal(d["po"], np.stack([r[4] for r in mroots])), o
            assert np.array_equal(ind, mind) and [int(v) for v in ind] == sent and toff.tobytes() == mtoff.tobytes(), (o, ind, mind, toff, mtoff)
            for q, v in devs.items():
                assert v <= tol(q), (o, q, v, tol(q))
        multi = h.multi([(fo, np.array(sig)) for fo, sig, _ in Z.occasions(size)])
        for o, (s, m) in enumerate(zip(singles, multi)):
            assert same(s, m[:3]) and m[3] == bytes(len(m[3])), o
    finally:
        h.close()
    assert capfd.readouterr().err == ""
