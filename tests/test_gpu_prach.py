"""PRACH detection on the device (include/srsran_amd/phy_prach_abi.h) through the C ABI, on the recorded occasions of tests/golden/prach_ref.npz (the
reference's own detector on preambles of its own generator).  Root spectra, prach_bins, corr, corr_ave, the cross sum and the window peaks of the _dbg call are
held to the record within the tolerances its generator measured; peak_offsets, the detection lists, their order and both forms of t_offsets are EXACT (the
generator asserts the margins that make them so).  max_det smaller than the list, _multi of mixed occasions against the single calls bit for bit and on a
second run, four host threads with their own handles, reuse of a handle across occasions, and the refusals that need a handle.

The record holds corr (and so the scale peak_values are judged against) only for the first, the last and every detected root of a case: the other roots of a
64-root case are held to the record through corr_ave, the cross sum and the exact peak_offsets alone."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_conv_abi import _one_line
from test_prach_abi import cfg_struct, set_order
from test_prach_golden import INFO, case, names, rel, tol

pytestmark = pytest.mark.gpu
NAMES = names()


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0 and set_order(lib) == 0
    return lib


class Handle:
    def __init__(self, L, g):
        from srslte_amd import capi

        self.L, self.capi, self.h = L, capi, C.c_void_p()
        L.srsran_use_standard_symbol_size(bool(g["standard"]))
        try:
            rc = L.srsran_hip_prach_create(C.byref(self.h), C.byref(cfg_struct(capi, g["cfg_dict"], float(g["factor"]))))
        finally:
            L.srsran_use_standard_symbol_size(False)
        assert rc == 0 and self.h.value
        self.info = capi.HipPrachInfo()
        assert L.srsran_hip_prach_info(self.h, C.byref(self.info)) == 0
        self.R, self.n_wins = self.info.num_ra_preambles, self.info.n_wins

    def close(self):
        self.L.srsran_hip_prach_destroy(self.h)

    def spectrum(self, i):
        out = np.full(839 + 4, 77.0, np.complex64)
        assert self.L.srsran_hip_prach_root_spectrum(self.h, i, out.ctypes.data) == 0 and np.all(out[839:] == 77.0)
        return out[:839]

    def detect(self, fo, sig, max_det=128, dbg=False, sig_len=None):
        ind, toff, p2a = np.full(max_det + 4, 0x77777777, np.uint32), np.full(max_det + 4, 77.0, np.float32), np.full(max_det + 4, 77.0, np.float32)
        n = C.c_uint32(0x77777777)
        a = [self.h, fo, sig.ctypes.data, sig.size if sig_len is None else sig_len, ind.ctypes.data, toff.ctypes.data, p2a.ctypes.data, max_det, C.byref(n)]
        o = None
        if dbg:
            R, W = self.R, self.n_wins
            o = dict(bins=np.full(839 + 2, 77.0, np.complex64), corr=np.full(R * 839 + 2, 77.0, np.float32), ave=np.full(R + 2, 77.0, np.float32),
                     cross=np.full(R + 2, 77.0, np.complex64), pv=np.full(R * W + 2, 77.0, np.float32), po=np.full(R * W + 2, 77, np.uint32))
            d = self.capi.HipPrachDbg(*[o[k].ctypes.data for k in ("bins", "corr", "ave", "cross", "pv", "po")])
            rc = self.L.srsran_hip_prach_detect_offset_dbg(*(a + [C.byref(d)]))
            assert all(np.all(v[-2:] == 77.0) for v in o.values())
            o = dict(bins=o["bins"][:839], corr=o["corr"][:-2].reshape(R, 839), ave=o["ave"][:R], cross=o["cross"][:R], pv=o["pv"][:-2].reshape(R, W),
                     po=o["po"][:-2].reshape(R, W))
        else:
            rc = self.L.srsran_hip_prach_detect_offset(*a)
        assert rc == 0 and n.value <= max_det
        k = n.value
        assert np.all(ind[k:] == 0x77777777) and np.all(toff[k:] == 77.0) and np.all(p2a[k:] == 77.0)  # nothing behind the count is touched
        return (ind[:k].copy(), toff[:k].copy(), p2a[:k].copy()), o

    def multi(self, occs):
        capi = self.capi
        occ = (capi.HipPrachOcc * len(occs))(*[capi.HipPrachOcc(fo, sig.size, sig.ctypes.data) for fo, sig in occs])
        res = (capi.HipPrachRes * len(occs))()
        C.memset(res, 0x77, C.sizeof(res))
        assert self.L.srsran_hip_prach_detect_multi(self.h, len(occs), occ, res) == 0
        return [(np.array(r.indices[:r.n_indices], np.uint32), np.array(r.t_offsets[:r.n_indices], np.float32), np.array(r.peak_to_avg[:r.n_indices], np.float32),
                 bytes(r)[4 + 4 * r.n_indices:516]) for r in res]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("c", range(len(NAMES)), ids=NAMES)
def test_detection_against_the_record(L, c):
    g = case(c)
    h = Handle(L, g)
    try:
        assert {k: getattr(h.info, k) for k in INFO} == g["info_dict"]
        for a, i in enumerate(g["keep"]):
            d = rel(h.spectrum(int(i)), g["spec"][a], np.abs(g["spec"][a]).max())
            print("spectrum of root %d: %.3g of %.3g" % (i, d, tol("spec")))
            assert d <= tol("spec")
        sig = np.concatenate([g["sig"], np.full(16, 7.0 + 7.0j, np.complex64)])  # sig_len may exceed N_ifft_prach: the tail is not read
        (ind, toff, p2a), o = h.detect(int(g["fo"]), sig, dbg=True)
        plain, _ = h.detect(int(g["fo"]), sig)
        assert same(plain, (ind, toff, p2a))  # the _dbg call is the call
        top = {int(i): float(g["corr"][a].max()) for a, i in enumerate(g["keep"])}
        devs = dict(bins=rel(o["bins"], g["bins"], np.abs(g["bins"]).max()),
                    corr=max(rel(o["corr"][i], g["corr"][a], top[int(i)]) for a, i in enumerate(g["keep"])),
                    ave=float(np.max(np.abs(o["ave"] - g["ave"]) / g["ave"])), cross=float(np.max(np.abs(o["cross"] - g["cross"]) / g["ave"])),
                    pv=max(rel(o["pv"][i], g["pv"][i], top[i]) for i in top), p2a=float(np.max(np.abs(p2a - g["p2a"]) / g["p2a"])) if ind.size else 0.0)
        print(NAMES[c], {q: "%.3g of %.3g" % (v, tol(q)) for q, v in devs.items()}, "detections", ind, g["ind"])
        # exact
        assert np.array_equal(o["po"], g["po"])
        assert np.array_equal(ind, g["ind"]) and toff.tobytes() == g["toff"].tobytes()
        for q, v in devs.items():
            assert v <= tol(q), (q, v, tol(q))
    finally:
        h.close()


def test_max_det_smaller_than_the_list(L):
    g = case(NAMES.index("6prb_zcz1_neighbours_first_last"))
    h = Handle(L, g)
    try:
        full, _ = h.detect(0, g["sig"])
        assert full[0].size == 2
        one, _ = h.detect(0, g["sig"], max_det=1)
        assert one[0].size == 1 and same(one, [v[:1] for v in full])
        ind, n = np.full(4, 0x77777777, np.uint32), C.c_uint32(7)  # t_offsets and peak_to_avg may be NULL, as in the reference
        assert L.srsran_hip_prach_detect_offset(h.h, 0, g["sig"].ctypes.data, g["sig"].size, ind.ctypes.data, None, None, 4, C.byref(n)) == 0
        assert n.value == 2 and np.array_equal(ind[:2], full[0]) and np.all(ind[2:] == 0x77777777)
    finally:
        h.close()


def test_multi_equals_the_single_calls_bit_for_bit_and_repeats(L):
    """occasions of one 15-PRB cell at different freq_offset, one of them empty; then a handle reused across occasions of different content"""
    g = case(NAMES.index("15prb_fo3_format1_phase"))
    rng = np.random.default_rng(5)
    noise = (0.01 * (rng.standard_normal(g["sig"].size) + 1j * rng.standard_normal(g["sig"].size))).astype(np.complex64)
    occs = [(3, g["sig"]), (0, g["sig"]), (9, noise), (3, (g["sig"] + noise).astype(np.complex64)), (3, np.zeros_like(noise)), (3, g["sig"]), (1, noise), (9, g["sig"])]
    h = Handle(L, g)
    try:
        single = [h.detect(fo, sig)[0] for fo, sig in occs]
        # the preamble lies on PRB 3 .. 8: an occasion at PRB 9 does not see it (one at PRB 0 or 1 sees a part of its bins, whatever that gives)
        assert np.array_equal(single[0][0], g["ind"]) and single[2][0].size == 0 and single[4][0].size == 0 and single[7][0].size == 0
        assert same(single[0], single[5])  # no stale state: the same occasion after others gives the same bits
        for run in range(2):
            multi = h.multi(occs)
            for o, (s, m) in enumerate(zip(single, multi)):
                assert same(s, m[:3]) and m[3] == bytes(len(m[3])), (run, o)  # behind the count the result is zeroed
        assert same(h.multi(occs[2:5])[1][:3], single[3])  # another number of occasions in the launch: the same bits
    finally:
        h.close()


def test_four_threads_with_their_own_handles(L):
    picks = [NAMES.index(n) for n in ("6prb_zcz0_roots_12db", "6prb_zcz11", "25prb_hs_fo2_format3", "6prb_zcz15_phase")]
    out, err = {}, []

    def work(c):
        try:
            g = case(c)
            h = Handle(L, g)
            try:
                out[c] = [h.detect(int(g["fo"]), g["sig"])[0] for _ in range(3)]
            finally:
                h.close()
        except Exception as e:  # noqa: BLE001
            err.append((c, repr(e)))

    threads = [threading.Thread(target=work, args=(c,)) for c in picks]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not err, err
    for c in picks:
        g = case(c)
        assert all(same(r, out[c][0]) for r in out[c])
        assert np.array_equal(out[c][0][0], g["ind"]) and out[c][0][1].tobytes() == g["toff"].tobytes()


def test_refusals_with_a_handle(L, capfd):
    from srslte_amd import capi

    INV = capi.SRSRAN_ERROR_INVALID_INPUTS
    g = case(NAMES.index("6prb_zcz11"))
    h = Handle(L, g)
    try:
        sig = g["sig"]
        for dbg in (False, True):
            who = "srsran_hip_prach_detect_offset_dbg" if dbg else "srsran_hip_prach_detect_offset"
            for what in ("signal", "indices", "n_indices", "sig_len", "freq_offset", "max_det", "dbg"):
                if what == "dbg" and not dbg:
                    continue
                ind, toff, p2a, n = np.full(8, 0x77777777, np.uint32), np.full(8, 5.0, np.float32), np.full(8, 5.0, np.float32), C.c_uint32(0x77777777)
                a = [h.h, 1 if what == "freq_offset" else 0, None if what == "signal" else sig.ctypes.data, sig.size - 1 if what == "sig_len" else sig.size,
                     None if what == "indices" else ind.ctypes.data, toff.ctypes.data, p2a.ctypes.data, 0 if what == "max_det" else 8,
                     None if what == "n_indices" else C.byref(n)]
                capfd.readouterr()
                rc = L.srsran_hip_prach_detect_offset_dbg(*(a + [None if what == "dbg" else C.byref(capi.HipPrachDbg())])) if dbg else L.srsran_hip_prach_detect_offset(*a)
                assert rc == INV and (what == "n_indices" or n.value == 0), (dbg, what)
                assert np.all(ind == 0x77777777) and np.all(toff == 5.0) and np.all(p2a == 5.0), (dbg, what)
                _one_line(capfd, who, (dbg, what))
        who = "srsran_hip_prach_detect_multi"
        for what in ("signal", "sig_len", "freq_offset", "occ", "res"):
            occ = (capi.HipPrachOcc * 2)(capi.HipPrachOcc(0, sig.size, sig.ctypes.data),
                                          capi.HipPrachOcc(1 if what == "freq_offset" else 0, sig.size - 1 if what == "sig_len" else sig.size,
                                                           None if what == "signal" else sig.ctypes.data))
            res = (capi.HipPrachRes * 3)()
            C.memset(res, 0x77, C.sizeof(res))
            capfd.readouterr()
            assert L.srsran_hip_prach_detect_multi(h.h, 2, None if what == "occ" else occ, None if what == "res" else res) == INV, what
            assert what == "res" or (bytes(res)[:2 * 1540] == bytes(2 * 1540) and bytes(res)[2 * 1540:] == b"\x77" * 1540), what
            _one_line(capfd, who, what)
        spec = np.full(839, 5.0, np.complex64)
        assert L.srsran_hip_prach_root_spectrum(h.h, h.R, spec.ctypes.data) == INV and np.all(spec == 5.0)
        _one_line(capfd, "srsran_hip_prach_root_spectrum", "i")
        full, _ = h.detect(0, sig)  # the handle is as good as before
        assert np.array_equal(full[0], g["ind"])
    finally:
        h.close()
