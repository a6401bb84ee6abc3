"""The PDCCH search from the subframe grids (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pdcch_get, srsran_hip_pdcch_extract_llr,
srsran_hip_pdcch_search_sf{,_dbg}) through the C ABI, on the recorded control regions (tests/golden/pdcch_sf_ref.npz).  Copies, decoded bits, CRC remainders
and everything the device computes twice are compared exactly (integers or float32 bit patterns); the soft bits are held to the reference's within llr_tol,
which the record's generator measured (four times the model's deviation from the reference, relative to the region's rms)."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_pdcch_sf_golden import llr_tol, rel_dev, sf_struct, signal_cases

pytestmark = pytest.mark.gpu
CASES = signal_cases()


@pytest.fixture(scope="module")
def L():
    from srslte_amd import capi

    lib = capi.lib()
    assert lib.srsran_hip_device_count() > 0
    return lib


class Region:
    """the arguments of the calls for one recorded case (the grids hold the region's rows, which is all the calls read)"""

    def __init__(self, c):
        from srslte_amd import capi

        self.c, self.capi = c, capi
        sf = c["sf"]
        self.ports, self.nof_rx, self.nsym, self.n = sf["cell_nof_ports"], sf["nof_rx"], c["table"].size, len(c["cand"])
        self.sf = sf_struct(capi, sf)
        self.rx = [np.ascontiguousarray(g) for g in c["rx"]]
        self.ce = [[np.ascontiguousarray(c["ce"][p][a]) for a in range(self.nof_rx)] for p in range(self.ports)]
        self.y = (C.c_void_p * 4)(*([g.ctypes.data for g in self.rx] + [None] * (4 - self.nof_rx)))
        rows = [[g.ctypes.data for g in row] + [None] * (4 - self.nof_rx) for row in self.ce] + [[None] * 4] * (4 - self.ports)
        self.h = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in rows])
        self.cand = (capi.HipPdcchCand * self.n)(*[capi.HipPdcchCand(*[int(v) for v in k]) for k in c["cand"]])
        self.noise = C.c_float(c["noise"])

    def extract(self, L):
        llr = np.full(2 * self.nsym + 8, 77.0, np.float32)
        assert L.srsran_hip_pdcch_extract_llr(C.byref(self.sf), self.y, self.h, self.noise, llr.ctypes.data) == 2 * self.nsym
        assert np.all(llr[2 * self.nsym:] == 77.0)
        return llr[:2 * self.nsym]

    def search(self, L):
        res = (self.capi.HipPdcchRes * self.n)()
        C.memset(res, 0x77, C.sizeof(res))
        assert L.srsran_hip_pdcch_search_sf(C.byref(self.sf), self.y, self.h, self.noise, self.n, self.cand, res) == 0
        return res

    def search_dbg(self, L):
        res = (self.capi.HipPdcchRes * self.n)()
        C.memset(res, 0x77, C.sizeof(res))
        o = dict(llr=np.full(2 * self.nsym + 8, 77.0, np.float32), d=np.full(self.nsym + 4, 77.0, np.complex64), rm=np.full(self.n * 432 + 8, 77.0, np.float32),
                 sym=np.full(self.n * 432 + 8, 77, np.uint16), x_rx=[np.full(self.nsym + 4, 77.0, np.complex64) for _ in range(self.nof_rx)],
                 x_ce=[[np.full(self.nsym + 4, 77.0, np.complex64) for _ in range(self.nof_rx)] for _ in range(self.ports)])
        so = (C.c_void_p * 4)(*([g.ctypes.data for g in o["x_rx"]] + [None] * (4 - self.nof_rx)))
        rows = [[g.ctypes.data for g in row] + [None] * (4 - self.nof_rx) for row in o["x_ce"]] + [[None] * 4] * (4 - self.ports)
        co = ((C.c_void_p * 4) * 4)(*[(C.c_void_p * 4)(*row) for row in rows])
        assert L.srsran_hip_pdcch_search_sf_dbg(C.byref(self.sf), self.y, self.h, self.noise, self.n, self.cand, res, o["llr"].ctypes.data, o["d"].ctypes.data, so, co,
                                                o["rm"].ctypes.data, o["sym"].ctypes.data) == 0
        assert np.all(o["llr"][2 * self.nsym:] == 77.0) and np.all(o["d"][self.nsym:] == 77.0) and np.all(o["rm"][self.n * 432:] == 77.0)
        assert np.all(o["sym"][self.n * 432:] == 77) and all(np.all(g[self.nsym:] == 77.0) for g in o["x_rx"] + sum(o["x_ce"], []))
        o["llr"], o["d"], o["rm"], o["sym"] = o["llr"][:2 * self.nsym], o["d"][:self.nsym], o["rm"][:self.n * 432], o["sym"][:self.n * 432]
        return res, o


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_gather_equals_the_table_gather(L, c):
    """srsran_hip_regs_pdcch_get on all planes in one launch: copies, exactly; and the planes _dbg hands back are the same copies"""
    r = Region(c)
    planes = r.rx + sum(r.ce, [])
    n = len(planes)
    outs = [np.full(r.nsym + 4, 77.0, np.complex64) for _ in planes]
    grids, d = (C.c_void_p * n)(*[g.ctypes.data for g in planes]), (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    assert L.srsran_hip_regs_pdcch_get(C.byref(r.sf), n, grids, d) == r.nsym
    for g, o in zip(planes, outs):
        assert same_bits(o[:r.nsym], g[c["table"]]) and np.all(o[r.nsym:] == 77.0)
    _, o = r.search_dbg(L)
    for g, x in zip(planes, o["x_rx"] + sum(o["x_ce"], [])):
        assert same_bits(x[:r.nsym], g[c["table"]])


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_soft_bits_are_one_set_of_bits_and_the_reference_to_tolerance(L, c):
    """the stage by itself and the search's llr_out are the same bits, and the same again on a second run; against the reference's soft bits within llr_tol"""
    r = Region(c)
    a, (_, o), b = r.extract(L), r.search_dbg(L), r.extract(L)
    assert same_bits(a, o["llr"]) and same_bits(a, b)
    _, o2 = r.search_dbg(L)
    assert all(same_bits(o[k], o2[k]) for k in ("llr", "d", "rm", "sym"))
    dev = rel_dev(a, c["llr"])
    print("%s: soft bits %.3g of the rms from the reference's (llr_tol %.3g)" % (c["name"], dev, llr_tol()))
    assert dev <= llr_tol()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_search_equals_the_candidate_call_on_its_own_soft_bits(L, c):
    """payload, crc_rem, decoded, mean, rm_f and symbols of every candidate -- noise, zero and wide-range ones included -- bit for bit what
    srsran_hip_pdcch_dci_decode_multi_dbg gives on the call's own llr_out (whose mean rule runs on the host); the plain form gives the same results;
    every recorded DCI comes back with the reference's payload and CRC remainder, and the zero region is not decoded"""
    r = Region(c)
    res, o = r.search_dbg(L)
    ref = (r.capi.HipPdcchRes * r.n)()
    rm, sym = np.full(r.n * 432, 77.0, np.float32), np.full(r.n * 432, 77, np.uint16)
    llr = np.ascontiguousarray(o["llr"])
    assert L.srsran_hip_pdcch_dci_decode_multi_dbg(llr.ctypes.data, llr.size, r.n, r.cand, ref, rm.ctypes.data, sym.ctypes.data) == 0
    for i in range(r.n):
        assert bytes(res[i]) == bytes(ref[i]), (c["name"], i, res[i].mean, ref[i].mean, res[i].decoded, ref[i].decoded)
    assert same_bits(o["rm"], rm) and same_bits(o["sym"], sym)
    assert bytes(r.search(L)) == bytes(res)
    assert {int(x.decoded) for x in res} == {0, 1}
    for i in range(r.n):
        if c["carry"][i]:
            assert res[i].decoded == 1 and res[i].crc_rem == c["crc"][i] and bytes(res[i].payload) == c["bits"][i].tobytes(), (c["name"], i)
        if c["mean"][i] == 0:
            assert res[i].decoded == 0 and res[i].mean == 0 and bytes(res[i].payload) == bytes(144) and res[i].crc_rem == 0, (c["name"], i)
            assert np.all(o["rm"][i * 432:(i + 1) * 432] == 0) and np.all(o["sym"][i * 432:(i + 1) * 432] == 0)


def test_search_sweeps_every_dci_size_on_one_region(L):
    """the test above with a candidate list that sweeps the size: nof_bits 1 .. 128 at CCE 0 of one recorded region of at least 8 CCE, the level rotating
    0 .. 3 -- every length of the rate de-matcher and the chain-back through the kernel that applies the mean rule on the device.  Result, rm and symbol rows bit
    for bit what srsran_hip_pdcch_dci_decode_multi_dbg gives on the call's own llr_out; decoded, crc_rem, payload, rm and symbols what the model gives on it"""
    import conv_model as CM
    import pdcch_map_model as PM

    def busy(c):  # at least 8 CCE, and CCE 0 carries energy at every level (judged on the recorded soft bits, which the device's equal to 1e-6)
        return c["table"].size // 36 >= 8 and all(CM.pdcch_mean(c["llr"], 0, lv) > 0.5 for lv in range(4))

    c = next(c for c in CASES if busy(c))
    cands = [(0, (nof_bits - 1) % 4, nof_bits) for nof_bits in range(1, 129)]
    r = Region(dict(c, cand=np.array(cands, np.uint32)))
    res, o = r.search_dbg(L)
    ref = (r.capi.HipPdcchRes * r.n)()
    rm, sym = np.full(r.n * 432, 77.0, np.float32), np.full(r.n * 432, 77, np.uint16)
    llr = np.ascontiguousarray(o["llr"])
    assert L.srsran_hip_pdcch_dci_decode_multi_dbg(llr.ctypes.data, llr.size, r.n, r.cand, ref, rm.ctypes.data, sym.ctypes.data) == 0
    bad = [cands[i][2] for i in range(r.n) if bytes(res[i]) != bytes(ref[i])]
    assert not bad, "nof_bits whose result rows differ: %s" % bad
    assert same_bits(o["rm"], rm) and same_bits(o["sym"], sym)
    assert bytes(r.search(L)) == bytes(res)
    want = PM.search(llr, cands)
    for i, (w, (_, lv, nof_bits)) in enumerate(zip(want, cands)):
        n3 = 3 * (nof_bits + 16)
        payload = np.frombuffer(bytes(res[i].payload), np.uint8)
        assert w["decoded"] and res[i].decoded == 1 and res[i].crc_rem == w["crc_rem"] and np.float32(res[i].mean) == np.float32(w["mean"]), (c["name"], nof_bits)
        assert np.array_equal(payload[:nof_bits + 16], w["bits"]) and not payload[nof_bits + 16:].any(), (c["name"], nof_bits)
        assert same_bits(o["rm"][i * 432:i * 432 + n3], w["rm"]) and not o["rm"][i * 432 + n3:(i + 1) * 432].any(), (c["name"], nof_bits)
        assert np.array_equal(o["sym"][i * 432:i * 432 + n3], w["sym"]) and not o["sym"][i * 432 + n3:(i + 1) * 432].any(), (c["name"], nof_bits)


def test_four_threads_with_different_regions_give_what_each_gives_alone(L):
    picks = [CASES[0], CASES[3], CASES[4], CASES[7]]
    alone = [(bytes(Region(c).search(L)), Region(c).extract(L).tobytes()) for c in picks]
    got, errors = [None] * 4, []

    def work(i):
        try:
            r = Region(picks[i])
            for _ in range(5):
                got[i] = (bytes(r.search(L)), r.extract(L).tobytes())
                assert got[i] == alone[i]
        except BaseException as e:  # noqa: B036 -- reported by the main thread
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == alone
