"""PCFICH and PHICH on the device (include/srsran_amd/phy_conv_abi.h: srsran_hip_pcfich_decode{,_dbg}, srsran_hip_phich_decode_multi) through the C ABI, on the
recorded regions and subframes (tests/golden/ctrl_ref.npz).  cfi and ack_value are compared exactly; data_f, corr, data_rx and distance are held to the
reference's within the tolerances the record's generator measured (four times the model's deviation from the reference: data_f against the case's rms, corr
against |corr|, data_rx and distance against the rms over the case's resources); everything the device computes twice is compared bit for bit.  The recorded
subframes go through the library's own chain -- srsran_hip_chest_dl_estimate, srsran_hip_pcfich_decode with its noise estimate, srsran_hip_pdcch_search_sf with
that CFI, srsran_hip_phich_decode_multi -- and must give the CFI, payloads and ACKs of the reference's chain."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_ctrl_golden import est_cases, float_devs, signal_cases, tol
from test_pdcch_sf_golden import sf_struct
from test_pdcch_sf_golden import signal_cases as pdcch_cases

pytestmark = pytest.mark.gpu
CASES = signal_cases()


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0
    return lib


def plane_args(rx, ce):
    """(sf_symbols[], ce[][4], the arrays they point to) for rx[a], ce[p][a]"""
    keep = [np.ascontiguousarray(g) for g in rx], [[np.ascontiguousarray(g) for g in row] for row in ce]
    y = (C.c_void_p * 4)(*([g.ctypes.data for g in keep[0]] + [None] * (4 - len(keep[0]))))
    rows = [[g.ctypes.data for g in row] + [None] * (4 - len(row)) for row in keep[1]] + [[None] * 4] * (4 - len(keep[1]))
    return y, ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in rows]), keep


class Region:
    """the arguments of the calls for one subframe: a description, grids rx[a] and ce[p][a], a noise estimate, PHICH resources"""

    def __init__(self, sf, rx, ce, noise, res):
        from srslte_amd import capi

        self.capi, self.sf, self.noise, self.n = capi, sf_struct(capi, sf), C.c_float(noise), len(res)
        self.y, self.h, self.keep = plane_args(rx, ce)
        self.r = (capi.HipPhichResource * self.n)(*[capi.HipPhichResource(int(g), int(s)) for g, s in res])

    def pcfich(self, L):
        cfi, corr = C.c_uint32(77), C.c_float(77.0)
        assert L.srsran_hip_pcfich_decode(C.byref(self.sf), self.y, self.h, self.noise, C.byref(cfi), C.byref(corr)) == 1
        return cfi.value, np.float32(corr.value)

    def pcfich_dbg(self, L):
        cfi, corr = C.c_uint32(77), C.c_float(77.0)
        o = dict(data_f=np.full(32 + 4, 77.0, np.float32), d=np.full(16 + 4, 77.0, np.complex64), corr3=np.full(3 + 4, 77.0, np.float32))
        assert L.srsran_hip_pcfich_decode_dbg(C.byref(self.sf), self.y, self.h, self.noise, C.byref(cfi), C.byref(corr), o["data_f"].ctypes.data, o["d"].ctypes.data,
                                              o["corr3"].ctypes.data) == 1
        assert np.all(o["data_f"][32:] == 77.0) and np.all(o["d"][16:] == 77.0) and np.all(o["corr3"][3:] == 77.0)
        return cfi.value, np.float32(corr.value), dict(data_f=o["data_f"][:32], d=o["d"][:16], corr3=o["corr3"][:3])

    def phich(self, L, n=None):
        n = self.n if n is None else n
        res = (self.capi.HipPhichRes * (n + 1))()
        C.memset(res, 0x77, C.sizeof(res))
        assert L.srsran_hip_phich_decode_multi(C.byref(self.sf), self.y, self.h, self.noise, n, self.r, res) == 0
        assert bytes(res[n]) == b"\x77" * 44
        return res


def region_of(c):
    nof_rx, ports = c["sf"]["nof_rx"], c["sf"]["cell_nof_ports"]
    return Region(c["sf"], list(c["rx"]), [[c["ce"][p][a] for a in range(nof_rx)] for p in range(ports)], c["noise"], c["res"])


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_pcfich_against_the_record(L, c):
    """cfi exact, corr and data_f within the stored tolerances; the plain form, the _dbg form and a repeat call give the same bits; the decision is the
    reference's on the call's own correlations (no positive one: cfi 1, corr 0)"""
    r = region_of(c)
    cfi, corr, o = r.pcfich_dbg(L)
    assert cfi == c["cfi"]
    dev = float_devs(c, o["data_f"], corr, c["bits"], c["distance"])
    print("%s: data_f %.3g (tol %.3g)  corr %.3g (tol %.3g)" % (c["name"], dev["data_f"], tol("data_f"), dev["corr"], tol("corr")))
    assert dev["data_f"] <= tol("data_f") and dev["corr"] <= tol("corr")
    best = int(np.argmax(o["corr3"]))
    if o["corr3"][best] > 0:
        assert cfi == best + 1 and same_bits(corr, o["corr3"][best])
    else:
        assert cfi == 1 and corr == 0 and not c["cfi_sent"]
    assert r.pcfich(L) == (cfi, corr)
    cfi2, corr2, o2 = r.pcfich_dbg(L)
    assert (cfi2, corr2) == (cfi, corr) and all(same_bits(o[k], o2[k]) for k in o)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_phich_against_the_record(L, c):
    """ack_value exact, data_rx and distance within the stored tolerances; a repeat call, and every resource in a call of its own, give the same bits"""
    r = region_of(c)
    res = r.phich(L)
    assert [int(x.ack_value) for x in res[:r.n]] == list(c["ack"])
    bits, dist = np.array([list(x.bits) for x in res[:r.n]], np.float32), np.array([x.distance for x in res[:r.n]], np.float32)
    dev = float_devs(c, c["data_f"], c["corr"], bits, dist)
    print("%s: data_rx %.3g (tol %.3g)  distance %.3g (tol %.3g)" % (c["name"], dev["bits"], tol("bits"), dev["distance"], tol("distance")))
    assert dev["bits"] <= tol("bits") and dev["distance"] <= tol("distance")
    assert bytes(r.phich(L)) == bytes(res)
    for i in (0, r.n - 1):
        one = Region(c["sf"], list(c["rx"]), r.keep[1], c["noise"], c["res"][i:i + 1])
        assert bytes(one.phich(L)[0]) == bytes(res[i]), i
    assert bytes(r.phich(L, 0)[0]) == b"\x77" * 44  # an empty call touches nothing


def chain(L, c, sf=None):
    """the library's own chain on a recorded subframe -> (cfi after the rule, corr, search results, PHICH results, the estimator's record)"""
    from srslte_amd import capi

    sf = dict(c["sf"]) if sf is None else sf
    nof_rx, ports, npts = sf["nof_rx"], sf["cell_nof_ports"], c["rx"].shape[1]
    est = capi.HipChestDl()
    est.nof_prb, est.nof_ports, est.id, est.cp_nsymb, est.nof_rx, est.sf_idx = sf["cell_nof_prb"], ports, sf["cell_id"], sf["cp_nsymb"], nof_rx, sf["sf_idx"]
    est.estimator_alg, est.noise_alg, est.filter_type = 1, 0, 2  # INTERPOLATE, REFS, no filter: what the record's reference side ran
    pilots = [np.ascontiguousarray(c["pilots0"]), np.ascontiguousarray(c["pilots1"])]
    est.pilots[0], est.pilots[1] = pilots[0].ctypes.data, pilots[1].ctypes.data
    state, out = capi.HipChestDlState(), capi.HipChestDlRes()
    ce = [[np.zeros(npts, np.complex64) for _ in range(nof_rx)] for _ in range(ports)]
    y, h, keep = plane_args(list(c["rx"]), ce)
    assert L.srsran_hip_chest_dl_estimate(C.byref(est), C.byref(state), y, h, C.byref(out)) == 0, capi.last_error()
    r = Region(sf, keep[0], keep[1], out.noise_estimate, c["res"])
    cfi, corr = r.pcfich(L)
    if c["cfi3_to_2"] and cfi == 3:
        cfi = 2
    n = len(c["cand"])
    cand, res = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*[int(v) for v in k]) for k in c["cand"]]), (capi.HipPdcchRes * n)()
    sf_c = sf_struct(capi, dict(sf, cfi=cfi))
    assert L.srsran_hip_pdcch_search_sf(C.byref(sf_c), r.y, r.h, r.noise, n, cand, res) == 0
    return cfi, corr, res, r.phich(L), out


@pytest.mark.parametrize("c", est_cases(), ids=lambda c: c["name"])
def test_recorded_subframes_through_the_three_call_chain(L, c):
    """the estimator, the PCFICH, the search with its CFI and the PHICH give the reference chain's CFI, payloads (crc_rem == rnti) and ACKs"""
    cfi, corr, res, ph, out = chain(L, c)
    assert cfi == c["cfi"] and corr > 0 and out.noise_estimate > 0
    for i in range(len(c["cand"])):
        assert res[i].decoded == 1 and res[i].crc_rem == c["crc"][i] and bytes(res[i].payload) == c["bits"][i].tobytes(), (c["name"], i)
    sent = c["sent"] >= 0
    acks = np.array([int(x.ack_value) for x in ph[:len(c["res"])]])
    assert np.array_equal(acks[sent], c["ack"][sent]) and np.array_equal(acks[sent], c["sent"][sent])


def test_four_threads_with_different_regions_give_what_each_gives_alone(L):
    picks = [CASES[0], CASES[3], CASES[4], CASES[6]]
    alone = [(region_of(c).pcfich(L), bytes(region_of(c).phich(L))) for c in picks]
    got, errors = [None] * 4, []

    def work(i):
        try:
            r = region_of(picks[i])
            for _ in range(5):
                got[i] = (r.pcfich(L), bytes(r.phich(L)))
                assert got[i] == alone[i]
        except BaseException as e:  # noqa: B036 -- reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == alone


# ---- the search from the received grids alone
def est_lists(c):
    """three candidate lists of different lengths: the case's DCIs where the CFI's region holds them, and c + 1 more candidates on the first CCE"""
    lists = []
    for k in range(3):
        fit = [tuple(int(v) for v in x) for x in c["cand"] if 72 * int(x[0]) + (72 << int(x[1])) <= 72 * int(c["nof_cce"][k])]
        lists.append(fit + [(0, 0, 27 + i) for i in range(k + 1)])
    assert len({len(x) for x in lists}) > 1
    return lists


class EstCall:
    """the arguments of srsran_hip_pdcch_search_est{,_dbg} for one recorded subframe"""

    def __init__(self, c, rule=None, lists=None):
        from srslte_amd import capi

        self.c, self.capi, sf = c, capi, c["sf"]
        self.nof_rx, self.ports, self.npts = sf["nof_rx"], sf["cell_nof_ports"], c["rx"].shape[1]
        self.sf = sf_struct(capi, sf)
        est = capi.HipChestDl()
        est.nof_prb, est.nof_ports, est.id, est.cp_nsymb, est.nof_rx, est.sf_idx = sf["cell_nof_prb"], self.ports, sf["cell_id"], sf["cp_nsymb"], self.nof_rx, sf["sf_idx"]
        est.estimator_alg, est.noise_alg, est.filter_type = 1, 0, 2
        self.pilots = [np.ascontiguousarray(c["pilots0"]), np.ascontiguousarray(c["pilots1"])]
        est.pilots[0], est.pilots[1] = self.pilots[0].ctypes.data, self.pilots[1].ctypes.data
        self.est, self.state = est, capi.HipChestDlState()
        self.rx = [np.ascontiguousarray(g) for g in c["rx"]]
        self.y = (C.c_void_p * 4)(*([g.ctypes.data for g in self.rx] + [None] * (4 - self.nof_rx)))
        self.lists = est_lists(c) if lists is None else lists
        flat = [k for x in self.lists for k in x]
        self.cand = (capi.HipPdcchCand * max(len(flat), 1))(*[capi.HipPdcchCand(*k) for k in flat])
        self.max_n, self.n_ph = max(len(x) for x in self.lists), len(c["res"])
        self.opt = capi.HipPdcchEst((C.c_uint32 * 3)(*[len(x) for x in self.lists]), int(c["cfi3_to_2"]) if rule is None else rule, self.n_ph)
        self.r = (capi.HipPhichResource * self.n_ph)(*[capi.HipPhichResource(int(g), int(s)) for g, s in c["res"]])

    def call(self, L, dbg):
        capi = self.capi
        res, ph = (capi.HipPdcchRes * (self.max_n + 1))(), (capi.HipPhichRes * (self.n_ph + 1))()
        C.memset(res, 0x77, C.sizeof(res))
        C.memset(ph, 0x77, C.sizeof(ph))
        cfi, corr, out = C.c_uint32(77), C.c_float(77.0), capi.HipChestDlRes()
        a = [C.byref(self.sf), C.byref(self.est), C.byref(self.state), self.y, C.byref(self.opt), self.cand, res, self.r, ph, C.byref(cfi), C.byref(corr), C.byref(out)]
        o = None
        if dbg:
            nmax = 72 * int(self.c["nof_cce"][2])
            o = dict(llr=np.full(nmax + 8, 77.0, np.float32), data_f=np.full(32 + 4, 77.0, np.float32), rm=np.full(self.max_n * 432 + 8, 77.0, np.float32),
                     sym=np.full(self.max_n * 432 + 8, 77, np.uint16), ce=[[np.full(self.npts + 4, 77.0, np.complex64) for _ in range(self.nof_rx)] for _ in range(self.ports)])
            rows = [[g.ctypes.data for g in row] + [None] * (4 - self.nof_rx) for row in o["ce"]] + [[None] * 4] * (4 - self.ports)
            co = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in rows])
            assert L.srsran_hip_pdcch_search_est_dbg(*(a + [o["llr"].ctypes.data, o["data_f"].ctypes.data, co, o["rm"].ctypes.data, o["sym"].ctypes.data])) == 0, capi.last_error()
            assert np.all(o["data_f"][32:] == 77.0) and np.all(o["rm"][self.max_n * 432:] == 77.0) and np.all(o["sym"][self.max_n * 432:] == 77)
            assert all(np.all(g[self.npts:] == 77.0) for g in sum(o["ce"], []))
        else:
            assert L.srsran_hip_pdcch_search_est(*a) == 0, capi.last_error()
        assert bytes(res[self.max_n]) == b"\x77" * 152 and bytes(ph[self.n_ph]) == b"\x77" * 44
        return cfi.value, np.float32(corr.value), res, ph, out, o


EST_RUNS = [(c, None) for c in est_cases()] + [(c, 0) for c in est_cases() if c["cfi3_to_2"]]  # CFI 2, 3 -> 2, 1 and 3


@pytest.mark.parametrize("c,rule", EST_RUNS, ids=lambda v: v["name"] if isinstance(v, dict) else "rule%s" % v)
def test_search_est_equals_the_three_call_chain_bit_for_bit(L, c, rule):
    """srsran_hip_pdcch_search_est_dbg against srsran_hip_chest_dl_estimate -> srsran_hip_pcfich_decode with res.noise_estimate -> srsran_hip_pdcch_search_sf_dbg with
    that CFI and ce (-> srsran_hip_phich_decode_multi) on the same grids: CFI, correlation, soft bits, every result row, both _dbg rows, the PHICH results, the
    estimator's record and its ce grids; the rows past the chosen list's length are zero; the plain form gives the same"""
    from srslte_amd import capi

    k = EstCall(c, rule)
    cfi, corr, res, ph, out, o = k.call(L, True)
    # the chain
    state, ref_out = capi.HipChestDlState(), capi.HipChestDlRes()
    ce = [[np.zeros(k.npts, np.complex64) for _ in range(k.nof_rx)] for _ in range(k.ports)]
    y, h, keep = plane_args(k.rx, ce)
    assert L.srsran_hip_chest_dl_estimate(C.byref(k.est), C.byref(state), y, h, C.byref(ref_out)) == 0
    r = Region(c["sf"], keep[0], keep[1], ref_out.noise_estimate, c["res"])
    ref_cfi, ref_corr, po = r.pcfich_dbg(L)
    if k.opt.cfi3_to_2 and ref_cfi == 3:
        ref_cfi = 2
    assert cfi == ref_cfi and same_bits(corr, ref_corr) and same_bits(o["data_f"][:32], po["data_f"])
    assert bytes(out) == bytes(ref_out)
    for p in range(k.ports):
        for a in range(k.nof_rx):
            assert same_bits(o["ce"][p][a][:k.npts], ce[p][a]), (p, a)
    mine = k.lists[cfi - 1]
    n, nbits = len(mine), 72 * int(c["nof_cce"][cfi - 1])
    cand, ref = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*x) for x in mine]), (capi.HipPdcchRes * n)()
    llr, rm, sym = np.zeros(nbits, np.float32), np.zeros(n * 432, np.float32), np.zeros(n * 432, np.uint16)
    sf_c = sf_struct(capi, dict(c["sf"], cfi=cfi))
    assert L.srsran_hip_pdcch_search_sf_dbg(C.byref(sf_c), r.y, r.h, r.noise, n, cand, ref, llr.ctypes.data, None, None, None, rm.ctypes.data, sym.ctypes.data) == 0
    assert same_bits(o["llr"][:nbits], llr) and np.all(o["llr"][nbits:] == 77.0)
    for i in range(n):
        assert bytes(res[i]) == bytes(ref[i]), (c["name"], i)
    assert same_bits(o["rm"][:n * 432], rm) and same_bits(o["sym"][:n * 432], sym)
    assert bytes(res)[n * 152:k.max_n * 152] == bytes((k.max_n - n) * 152)  # the rows past the chosen list's length
    assert np.all(o["rm"][n * 432:k.max_n * 432] == 0) and np.all(o["sym"][n * 432:k.max_n * 432] == 0)
    assert bytes(ph)[:k.n_ph * 44] == bytes(r.phich(L))[:k.n_ph * 44]
    cfi2, corr2, res2, ph2, out2, _ = k.call(L, False)
    assert (cfi2, bytes(res2), bytes(ph2), bytes(out2)) == (cfi, bytes(res), bytes(ph), bytes(out)) and same_bits(corr2, corr)


@pytest.mark.parametrize("c", est_cases(), ids=lambda c: c["name"])
def test_search_est_gives_the_reference_chain_on_the_recorded_subframes(L, c):
    """CFI, payloads (crc_rem == rnti) and ACKs of the reference's chain, with the recorded DCIs as the list of every CFI whose region holds them"""
    k = EstCall(c)
    cfi, corr, res, ph, out, _ = k.call(L, False)
    assert cfi == c["cfi"] and corr > 0
    mine = k.lists[cfi - 1]
    for i, x in enumerate(c["cand"]):
        j = mine.index(tuple(int(v) for v in x))
        assert res[j].decoded == 1 and res[j].crc_rem == c["crc"][i] and bytes(res[j].payload) == c["bits"][i].tobytes(), (c["name"], i)
    sent = c["sent"] >= 0
    acks = np.array([int(x.ack_value) for x in ph[:k.n_ph]])
    assert np.array_equal(acks[sent], c["ack"][sent])


def test_search_est_on_four_threads(L):
    cases = est_cases()
    picks = [cases[i % len(cases)] for i in range(4)]
    alone = []
    for c in picks:
        cfi, corr, res, ph, out, _ = EstCall(c).call(L, False)
        alone.append((cfi, bytes(res), bytes(ph), bytes(out)))
    got, errors = [None] * 4, []

    def work(i):
        try:
            k = EstCall(picks[i])
            for _ in range(5):
                cfi, corr, res, ph, out, _ = k.call(L, False)
                got[i] = (cfi, bytes(res), bytes(ph), bytes(out))
                assert got[i] == alone[i]
        except BaseException as e:  # noqa: B036 -- reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == alone


def test_search_est_on_more_descriptions_than_the_table_caches_hold(L):
    """the tables of CFI 1, 2 and 3 of a dozen and more descriptions through one thread's caches of 32 entries, which start over when they are full: every call's
    soft bits and result rows are what srsran_hip_pdcch_search_sf_dbg gives with that call's own estimates, i.e. each kernel read the tables of ITS description"""
    from srslte_amd import capi

    c0 = next(c for c in est_cases() if c["cfi3_to_2"])
    lists, done = [[(0, 0, 27)], [(0, 0, 27), (1, 0, 31)], [(0, 0, 27), (1, 0, 31), (0, 1, 27)]], 0
    for length, mbsfn in ((0, 0), (1, 0), (1, 1)):
        for ng in (0, 1, 2):
            for mi in (1, 2):
                sf = dict(c0["sf"], phich_length=length, mbsfn_or_sf1_6_tdd=mbsfn, phich_resources=ng, phich_mi=mi)
                nregs = [L.srsran_hip_regs_pdcch_nregs(C.byref(sf_struct(capi, dict(sf, cfi=k)))) for k in (1, 2, 3)]
                if min(nregs) < 18:
                    continue
                c = dict(c0, sf=sf, res=c0["res"][:1], nof_cce=np.array(nregs) // 9)
                k = EstCall(c, lists=lists)
                cfi, corr, res, ph, out, o = k.call(L, True)
                assert cfi == 2
                r = Region(dict(sf, cfi=cfi), k.rx, [[g[:k.npts] for g in row] for row in o["ce"]], out.noise_estimate, c["res"])
                n, nbits = len(lists[cfi - 1]), 8 * nregs[cfi - 1]
                cand, ref = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*x) for x in lists[cfi - 1]]), (capi.HipPdcchRes * n)()
                llr = np.zeros(nbits, np.float32)
                assert L.srsran_hip_pdcch_search_sf_dbg(C.byref(r.sf), r.y, r.h, r.noise, n, cand, ref, llr.ctypes.data, None, None, None, None, None) == 0
                assert same_bits(o["llr"][:nbits], llr) and bytes(res)[:n * 152] == bytes(ref), sf
                assert bytes(ph)[:44] == bytes(r.phich(L))[:44], sf
                done += 1
    assert 3 * done > 32 + 3  # the caches started over at least once, with entries of the call in hand


def test_a_recorded_pdcch_search_still_gives_its_recorded_bits(L):
    """after the new calls, one recorded srsran_hip_pdcch_search_sf region (2 ports, 2 antennas): the shared front kernel serves its earlier caller unchanged --
    the soft bits against the reference's within the record's llr_tol, every DCI's payload, the zero region not decoded"""
    from srslte_amd import capi
    from test_pdcch_sf_golden import llr_tol, rel_dev

    region_of(CASES[3]).pcfich(L)
    EstCall(est_cases()[1]).call(L, False)
    c = next(c for c in pdcch_cases() if c["name"] == "15prb_2p_2rx")
    y, h, keep = plane_args(list(c["rx"]), [[c["ce"][p][a] for a in range(2)] for p in range(2)])
    n = len(c["cand"])
    cand, res = (capi.HipPdcchCand * n)(*[capi.HipPdcchCand(*[int(v) for v in k]) for k in c["cand"]]), (capi.HipPdcchRes * n)()
    sf, llr = sf_struct(capi, c["sf"]), np.zeros(c["llr"].size, np.float32)
    assert L.srsran_hip_pdcch_search_sf_dbg(C.byref(sf), y, h, C.c_float(c["noise"]), n, cand, res, llr.ctypes.data, None, None, None, None, None) == 0
    assert rel_dev(llr, c["llr"]) <= llr_tol()
    for i in range(n):
        if c["carry"][i]:
            assert res[i].decoded == 1 and res[i].crc_rem == c["crc"][i] and bytes(res[i].payload) == c["bits"][i].tobytes(), i
        if c["mean"][i] == 0:
            assert res[i].decoded == 0 and res[i].mean == 0 and bytes(res[i].payload) == bytes(144), i
