"""The soft bits of every PDSCH receive grant path held to the ORACLE's demodulator, soft bit by soft bit, at sizes that leave the demodulator a tail:
srsran_hip_pdsch_decode{,_txdiv,_mimo}{,_csi}{,_dbg} and the _sf forms (include/srsran_amd/phy_chan_abi.h).

The reference's integer demodulator is position dependent (csrc/modem_arith.h: demod_int): 16-QAM and 64-QAM run a vector body over groups of 4 symbols (16-bit soft
bits) or 8 symbols (8-bit) that rounds to nearest and saturates, and a scalar tail over the last n % 4 / n % 8 symbols that truncates and wraps; QPSK saturates in the
body of 16 values and wraps in the tail; BPSK and 256-QAM have one rule.  Every fused front end hands demod_int the symbol's index in the codeword and the codeword's
count itself, so a wrong index or count shows in the last 1 to 7 symbols of a codeword only -- and the other PDSCH grant tests run at multiples of 4, take their
expected soft bits from the library's own demodulator, or look through a decoder that corrects a few soft bits.  This module is what holds the PDSCH paths' soft bits
to the oracle.

Expected side, the same for every path:
  x     the equalised, layer-de-mapped symbols of the library's stage call on the same planes (srsran_predecoding_single; srsran_predecoding_diversity_multi +
        srsran_layerdemap_diversity; srsran_hip_predecoding_mimo; the symbols as given with ce == NULL).  The float equalisers have their own float64 and record
        tests; here the _dbg call's d_out must equal x bit for bit
  e     O.sequence_apply(O.demod_soft(mod, x, width), seed): the oracle's demodulator and descrambler; for the _csi calls csi_model(e, the stage call's CSI row)
  rows  O.sch_decode_tb(tbs, Qm, rv, e, ...) with two half iterations on planes of random complex Gaussian samples: no block decodes (asserted), so the call hands
        every soft-buffer row back.  Transmit diversity passes 2 Qm, as the library does (tb.nl = 2)
Asserted: the _dbg call's e_out equal to e bit for bit, the guard words behind e_out and d_out; for the plain call on a fresh soft buffer and then a second
transmission (rv 1) into the same one: return code 0, crc_ok 0, no code-block flag, the oracle's iteration average within 1e-6, every row of every block equal over its
3 (K + 32) + 12 entries and zero behind them, the spare row zero, nothing written behind the payload's bytes.

The tail must be seen: every case whose modulation and width have a tail rule demodulates x with 16 more symbols behind it on the oracle; the first nbits values must
differ from e, and only inside the tail's symbols.  A case that cannot show this fails (DRAW: which draw of the planes a case takes was chosen on the CPU).  QPSK
parts only where a value leaves the number format: one 8-bit QPSK case per path family has a receive gain (chosen on the CPU with the oracle alone: see GAIN) that
takes the tail's values out of int8 and carries the assertion; the other QPSK cases, BPSK and 256-QAM are compared bit for bit without it.

Sizes: a tile is 2048 symbols, a wave's share 512, one pass of a wave 128 REs on 2 ports and MIMO, 256 on 4 ports.
  one port         7 (all tail in 8 bit), 515 (one pass into a second wave), 2053 (one pass into a second tile); zero forcing, MMSE and ce == NULL
  2-port diversity 6, 514, 2054: n % 4 == 2, n % 8 in {2, 6}; 1 and 2 receive antennas
  4-port diversity 4, 516, 2052: n % 8 == 4.  A multiple of 4 has NO 16-bit tail: those cases are compared bit for bit without the tail assertion
  MIMO             5, 515, 2051, 2054 (CDD refuses an odd count: 6, 514, 2054); (16-QAM, 64-QAM) and (64-QAM, 16-QAM); CDD with MMSE, codebook 1 with zero forcing,
                   codebook 2 with MMSE, one layer on codebook 3; a second codeword skipped by a NULL soft buffer at 515
  _csi calls       515 for one port and MIMO (CDD 514), 514 / 516 for 2- / 4-port diversity
  _sf forms        one cell per family whose srsran_hip_pdsch_nof_re is off the group of 8: odd on one port, 2 mod 4 on a 2-port cell (transmit diversity and MIMO:
                   every count a PRB gives on a symbol of a 2-port cell is even, so a MIMO grant from a grid cannot be odd)
No transport-block stage refused a size: the smallest ones run with tbs 40."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import csi_model as CM
import oracle_api as O
import pdsch_map_model as PM
import spmux_model as M
from grant_helpers import SB, _lib, _matrix, _planes, _rx_softbuffer

pytestmark = pytest.mark.gpu
ITERS = 2  # half iterations: nothing is meant to decode
SCALING = 0.8
MUX, CDD = M.TXSCHEME_SPATIALMUX, M.TXSCHEME_CDD
E_GUARD, C_GUARD, D_GUARD = 7, -7.0, np.complex64(-7 + 7j)
GROUP = {False: 4, True: 8}  # symbols per iteration of the 16-QAM / 64-QAM vector bodies, by llr8
# The receive gain of the QPSK saturation cases.  8-bit QPSK soft bits are trunc(x * -20 sqrt 2): they leave int8 from |Re x|, |Im x| = 4.5 on.  Planes of unit
# variance through these equalisers (taps around 0.9, scaling 0.8) give components of standard deviation about 1: with the planes scaled by 40 a component stays
# inside +-4.5 with probability 0.09.  The oracle alone, on the CPU, 20 draws of symbols of standard deviation 39 per component: of the 6 tail values of 515 symbols
# between 4 and 6 differed between the two rules, of the 4 of 514 symbols 3 or 4, of the 8 of 516 symbols 6 to 8.
GAIN = 40.0

#                  kind     ports nrx  one port: noise_estimate (None: ce == NULL); MIMO: (scheme, layers, codebook_idx, decoder, noise_estimate)
PATHS = {
    "one_port_zf": ("single", 1, 1, 0.0),
    "one_port_mmse": ("single", 1, 1, 0.02),
    "one_port_pre": ("single", 1, 1, None),
    "txdiv_2x1": ("txdiv", 2, 1, None),
    "txdiv_2x2": ("txdiv", 2, 2, None),
    "txdiv_4x1": ("txdiv", 4, 1, None),
    "txdiv_4x2": ("txdiv", 4, 2, None),
    "cdd_mmse": ("mimo", 2, 2, (CDD, 2, 0, M.MMSE, 0.05)),
    "mux2_cb1_zf": ("mimo", 2, 2, (MUX, 2, 1, M.ZF, 0.0)),
    "mux2_cb2_mmse": ("mimo", 2, 2, (MUX, 2, 2, M.MMSE, 0.05)),
    "mux1_cb3": ("mimo", 2, 2, (MUX, 1, 3, M.MMSE, 0.0)),
}
SIZES = {
    "one_port_zf": (7, 515, 2053), "one_port_mmse": (7, 515, 2053), "one_port_pre": (7, 515, 2053),
    "txdiv_2x1": (6, 514, 2054), "txdiv_2x2": (6, 514, 2054),
    "txdiv_4x1": (4, 516, 2052), "txdiv_4x2": (4, 516, 2052),  # n % 8 == 4; no 16-bit tail
    "cdd_mmse": (6, 514, 2054),  # (CDD refuses an odd count)
    "mux2_cb1_zf": (5, 515, 2051, 2054), "mux2_cb2_mmse": (5, 515, 2051, 2054), "mux1_cb3": (5, 515, 2051, 2054),
}
CSI_SIZE = {"one_port_mmse": 515, "one_port_pre": 515, "txdiv_2x1": 514, "txdiv_2x2": 514, "txdiv_4x1": 516, "txdiv_4x2": 516, "cdd_mmse": 514, "mux2_cb1_zf": 515,
            "mux2_cb2_mmse": 515, "mux1_cb3": 515}
SF_PATHS = {"one_port_mmse": "prb15_sf0_one_port", "txdiv_2x2": "prb15_sf0_two_ports", "mux2_cb2_mmse": "prb15_sf0_two_ports"}


def family(path):
    kind, ports, _, _ = PATHS[path]
    return {"single": "one_port", "mimo": "mimo"}.get(kind, "txdiv_%d_ports" % ports)


def ncw_of(path):
    kind, _, _, detail = PATHS[path]
    return detail[1] if kind == "mimo" else 1


def _build_cases():
    """(group, path, nof_re, mods, llr8, gain, skip): group "plain" / "csi" / "sf" (nof_re None: the cell's count); mods per codeword; skip: the codeword without a
    soft buffer"""
    cases = []

    def both_qams(group, path, n, llr8):
        if ncw_of(path) == 2:
            cases.extend((group, path, n, mods, llr8, None, None) for mods in ((2, 3), (3, 2)))
        else:
            cases.extend((group, path, n, (mod,), llr8, None, None) for mod in (2, 3))

    for path in PATHS:
        for n in SIZES[path]:
            for llr8 in (False, True):
                both_qams("plain", path, n, llr8)
    # QPSK, 8 bit, with the gain that takes the tail out of int8: one per path family
    cases += [("plain", "one_port_mmse", 515, (1,), True, GAIN, None), ("plain", "txdiv_2x2", 514, (1,), True, GAIN, None),
              ("plain", "txdiv_4x1", 516, (1,), True, GAIN, None), ("plain", "mux2_cb2_mmse", 515, (1, 1), True, GAIN, None)]
    # the other store widths (no tail assertion): QPSK at unit gain, 256-QAM and BPSK
    cases += [("plain", "one_port_zf", 515, (1,), False, None, None), ("plain", "one_port_pre", 2053, (4,), True, None, None),
              ("plain", "txdiv_2x1", 514, (4,), False, None, None), ("plain", "txdiv_4x2", 516, (0,), True, None, None),
              ("plain", "mux2_cb1_zf", 2051, (4, 0), False, None, None), ("plain", "mux2_cb1_zf", 515, (0, 4), True, None, None)]
    # a second codeword skipped by a NULL soft buffer, on an odd size
    cases += [("plain", "mux2_cb2_mmse", 515, (2, 3), False, None, 1), ("plain", "mux2_cb1_zf", 515, (3, 2), True, None, 1)]
    for path, n in CSI_SIZE.items():
        for llr8 in (False, True):
            both_qams("csi", path, n, llr8)
    for path in SF_PATHS:
        for llr8 in (False, True):
            both_qams("sf", path, None, llr8)
    return cases


CASES = _build_cases()
# Which draw of the random planes a case takes (inputs_of; 0 where it is not listed).  Whether the two rules part on a tail value is a matter of its fraction (one
# half of the values) or of its size, so with one to three tail symbols a few draws leave the tail nothing to decide.  These were chosen on the CPU, before any run on
# the device: the first draw on which float64 models of the equalisers (the oracle's predecoding_single, test_gpu_txdiv._ref64, spmux_model.model64) give symbols whose
# tail is seen, and still is with the symbols scaled by 1 +- 1e-5.
DRAW = {"csi_cdd_mmse_514_m32_8bit": 1, "csi_mux2_cb2_mmse_515_m23_8bit": 1, "plain_cdd_mmse_514_m32_16bit": 1, "plain_mux2_cb1_zf_5_m23_16bit": 2,
        "plain_one_port_pre_2053_m3_16bit": 3, "sf_mux2_cb2_mmse_grid_m32_8bit": 1, "sf_one_port_mmse_grid_m3_8bit": 1}


def _id(c):
    group, path, n, mods, llr8, gain, skip = c
    return "%s_%s_%s_m%s_%s%s%s" % (group, path, "grid" if n is None else n, "".join(map(str, mods)), "8bit" if llr8 else "16bit", "_gain" if gain else "",
                                    "" if skip is None else "_skip%d" % skip)


def _seed(k):
    return O.pdsch_seed(0x1234, k, 10, 301)


def tbs_of(mod, nof_re):
    """small transport blocks already in use in the suite: one code block that the soft bits fill partly (puncturing) or more than once (repetition), two code
    blocks at the sizes of a second tile"""
    if nof_re < 16:
        return 40
    if nof_re < 1000:
        return {2: 600, 3: 1544, 4: 1544}.get(mod, 328)
    return 6200 if mod >= 2 else 1544


def has_tail(mod, llr8, nof_re):
    return mod in (2, 3) and nof_re % GROUP[llr8] != 0


@functools.lru_cache(maxsize=None)
def sf_cell(name):
    """15 PRB, subframe 0, PRBs 2, 4 and 5: PRB 4 is the lower half PRB under the PBCH, which gives 5 (one port) and 4 + 6 + 6 + 6 (two ports) REs on the PBCH's four
    symbols"""
    prb = np.zeros((2, 15), np.uint8)
    prb[:, [2, 4, 5]] = 1
    return PM.make(15, 1 if name == "prb15_sf0_one_port" else 2, 8, prb, sf_idx=0, lstart=3)


def sf_count_is_off_the_group(path, n):
    return n % 2 == 1 if family(path) == "one_port" else n % 4 == 2


def _aligned(x):
    a = O.aligned_empty(x.size, np.complex64)
    a[:] = x
    return a


def oracle_bits(mod, x, llr8, seed):
    return O.sequence_apply(O.demod_soft(mod, _aligned(x), "b" if llr8 else "s"), seed)


def tail_is_seen(mod, x, llr8, seed, e, more):
    """the same symbols with 16 more behind them: the soft bits of x must change, and only in the symbols (QPSK: the values) the tail rule covers"""
    n, Qm = x.size, O.QM[mod]
    body = oracle_bits(mod, np.concatenate([x, more]), llr8, seed)[:n * Qm]
    first = 2 * n - (2 * n) % 16 if mod == 1 else (n - n % GROUP[llr8]) * Qm
    diff = np.flatnonzero(body != e)
    assert diff.size > 0, "the tail rule changes no soft bit of this input: the case does not reach the edge it is for"
    assert diff[0] >= first, (int(diff[0]), first)
    return diff.size


# ---- the library's side

def _stage(lib, capi, path, y, h, csi_in):
    """the stage call of the path on the planes: ([x per codeword], [CSI row per codeword])"""
    kind, ports, nrx, detail = PATHS[path]
    n = y.shape[1]
    if kind == "single":
        if detail is None:
            return [y[0]], [csi_in]
        x, csi = np.zeros(n, np.complex64), np.full(n + 4, C_GUARD, np.float32)
        assert lib.srsran_predecoding_single(O.P(y[0]), O.P(h[0][0]), O.P(x), O.P(csi), n, SCALING, detail) == n
        return [x], [csi[:n]]
    if kind == "txdiv":
        xl, csi = np.zeros((ports, n // ports), np.complex64), np.full(n + 4, C_GUARD, np.float32)
        assert lib.srsran_predecoding_diversity_multi(_planes(capi, list(y)), _matrix(capi, h), _planes(capi, list(xl)), (C.c_void_p * 2)(csi.ctypes.data, None), nrx, ports, n,
                                                      SCALING) == n // ports
        x = np.zeros(n, np.complex64)
        assert lib.srsran_layerdemap_diversity(_planes(capi, list(xl)), O.P(x), ports, n // ports) == n
        return [x], [csi[:n]]
    scheme, layers, cb, dec, noise = detail
    x, csi = np.zeros((2, n), np.complex64), np.full((2, n + 4), C_GUARD, np.float32)
    assert lib.srsran_hip_predecoding_mimo(_planes(capi, list(y)), _matrix(capi, h), _planes(capi, list(x)), (C.c_void_p * 2)(csi[0].ctypes.data, csi[1].ctypes.data), 2, 2, layers,
                                           cb, n, scheme, SCALING, noise, dec) == 0, capi.last_error()
    # (two-layer zero forcing: the stage writes row 0 only, all 1.0; the grant call uses 1.0 for row 1 as well)
    return [x[k] for k in range(layers)], [np.ones(n, np.float32) if np.all(csi[k, :n] == C_GUARD) else csi[k, :n] for k in range(layers)]


def _grant_call(lib, capi, path, y, h, csi_in, tbm, rv, llr8, sbs, weight, dbg, skip=None, sfd=None):
    """one grant call of the path: plain or _csi (weight), with or without _dbg, on planes y [nrx][n], h [ports][nrx][n] -- or, with a subframe description sfd, the _sf
    form on grids.  sbs: the soft buffers per codeword.  Returns [(res, data, d_out, e_out) per codeword]; d_out / e_out keep their guard words"""
    kind, ports, nrx, detail = PATHS[path]
    nof_re = y.shape[1] if sfd is None else PM.indices(sfd).size
    dt = np.int8 if llr8 else np.int16
    ncw = len(tbm)
    data = [np.full(tbs // 8 + 16, 0xA5, np.uint8) for _, tbs in tbm]
    d_out = [np.full(nof_re + 4, D_GUARD, np.complex64) for _ in tbm]
    e_out = [np.full(nof_re * O.QM[mod] + 16, E_GUARD, dt) for mod, _ in tbm]
    tbs_ = [capi.HipGrantTb(mod, tbs, rv, nof_re, _seed(k), ITERS, 1 if llr8 else 0, 2 if kind == "txdiv" else 1) for k, (mod, tbs) in enumerate(tbm)]
    sf = () if sfd is None else (C.byref(PM.to_struct(capi, sfd, 1 if weight else 0)),)
    res = (capi.HipGrantRes * 2)(capi.HipGrantRes(7, 7.0, 7.0), capi.HipGrantRes(7, 7.0, 7.0))
    if kind == "single":
        ce = detail is not None
        g = capi.HipPdschRx(tbs_[0], SCALING if ce else 1.0, detail if ce else 0.0)
        head = (C.byref(g),) + sf + (O.P(y[0]), O.P(h[0][0]) if ce else None)
        tail = (C.byref(sbs[0][0]), O.P(data[0]), res)
        dbg_out = (O.P(d_out[0]), O.P(e_out[0]))
        if sfd is not None:
            rc = lib.srsran_hip_pdsch_decode_sf_dbg(*head, *tail, *dbg_out, None, None, None) if dbg else lib.srsran_hip_pdsch_decode_sf(*head, *tail)
        elif weight:
            head += (None if ce else O.P(csi_in),)
            rc = lib.srsran_hip_pdsch_decode_csi_dbg(*head, *tail, *dbg_out, None) if dbg else lib.srsran_hip_pdsch_decode_csi(*head, *tail)
        else:
            rc = lib.srsran_hip_pdsch_decode_dbg(*head, *tail, *dbg_out) if dbg else lib.srsran_hip_pdsch_decode(*head, *tail)
    elif kind == "txdiv":
        g = capi.HipPdschTxdivRx(tbs_[0], ports, nrx, SCALING, 0)
        args = (C.byref(g),) + sf + (_planes(capi, list(y)), _matrix(capi, h), C.byref(sbs[0][0]), O.P(data[0]), res)
        dbg_out = (O.P(d_out[0]), O.P(e_out[0]))
        if sfd is not None:
            rc = lib.srsran_hip_pdsch_decode_txdiv_sf_dbg(*args, *dbg_out, None, None, None) if dbg else lib.srsran_hip_pdsch_decode_txdiv_sf(*args)
        elif weight:
            rc = lib.srsran_hip_pdsch_decode_txdiv_csi_dbg(*args, *dbg_out, None) if dbg else lib.srsran_hip_pdsch_decode_txdiv_csi(*args)
        else:
            rc = lib.srsran_hip_pdsch_decode_txdiv_dbg(*args, *dbg_out) if dbg else lib.srsran_hip_pdsch_decode_txdiv(*args)
    else:
        scheme, layers, cb, dec, noise = detail
        g = capi.HipPdschMimoRx((capi.HipGrantTb * 2)(*tbs_), ncw, layers, scheme, cb, dec, 2, SCALING, noise)
        sbp = (C.POINTER(capi.SoftbufferRx) * 2)(*[None if k == skip else C.pointer(sbs[k][0]) for k in range(ncw)])
        args = (C.byref(g),) + sf + (_planes(capi, list(y)), _matrix(capi, h), sbp, (C.c_void_p * 2)(*[a.ctypes.data for a in data]), res)
        dbg_out = ((C.c_void_p * 2)(*[a.ctypes.data for a in d_out]), (C.c_void_p * 2)(*[None if k == skip else e_out[k].ctypes.data for k in range(ncw)]))
        if sfd is not None:
            rc = lib.srsran_hip_pdsch_decode_mimo_sf_dbg(*args, *dbg_out, None, None, None) if dbg else lib.srsran_hip_pdsch_decode_mimo_sf(*args)
        elif weight:
            rc = lib.srsran_hip_pdsch_decode_mimo_csi_dbg(*args, *dbg_out, None) if dbg else lib.srsran_hip_pdsch_decode_mimo_csi(*args)
        else:
            rc = lib.srsran_hip_pdsch_decode_mimo_dbg(*args, *dbg_out) if dbg else lib.srsran_hip_pdsch_decode_mimo(*args)
    assert rc == 0, (path, weight, dbg, capi.last_error())
    if ncw == 1:
        assert kind != "mimo" or (res[1].crc_ok == 0 and res[1].avg_iterations_block == 0.0 and np.isnan(res[1].epre))
    return [(res[k], data[k], d_out[k], e_out[k]) for k in range(ncw)]


def _planes_of(rng, path, n, gain):
    """received planes of random complex Gaussian samples and well-conditioned estimates (transmit diversity: constant over a pair / quad, as its combiner assumes)"""
    kind, ports, nrx, _ = PATHS[path]
    y = np.ascontiguousarray((M.cn(rng, (nrx, n)) * (gain or 1.0)).astype(np.complex64))
    if kind == "mimo":
        return y, M.channel(rng, n)
    group = ports if kind == "txdiv" else 1
    t = 0.9 + 0.1 * (rng.standard_normal((ports, nrx, n // group)) + 1j * rng.standard_normal((ports, nrx, n // group)))
    return y, np.ascontiguousarray(np.repeat(t, group, axis=2).astype(np.complex64))


def nof_re_of(case):
    return PM.indices(sf_cell(SF_PATHS[case[1]])).size if case[2] is None else case[2]


def inputs_of(case):
    """what the two transmissions of a case receive, from the case's name and its entry in DRAW alone: per transmission (y, h, gy, gh, csi_in, more) -- the planes, what
    the call is given (the planes, or grids that are random everywhere and hold the planes at the model's indices), the caller's CSI row of the weighted ce == NULL
    form, and per codeword the 16 symbols the tail check puts behind x"""
    group, path, _, mods, _, gain, _ = case
    kind, ports, nrx, detail = PATHS[path]
    nof_re = nof_re_of(case)
    rng = np.random.default_rng([zlib.crc32(_id(case).encode()), DRAW.get(_id(case), 0)])
    out = []
    for _ in range(2):
        if group != "sf":
            y, h = _planes_of(rng, path, nof_re, gain)
            gy, gh = y, h
        else:
            sfd = sf_cell(SF_PATHS[path])
            pts, idx = PM.grid_points(sfd), PM.indices(sfd)
            gy = np.ascontiguousarray(M.cn(rng, (nrx, pts)).astype(np.complex64))
            gh = np.ascontiguousarray((0.9 + 0.3 * M.cn(rng, (ports, nrx, pts))).astype(np.complex64))
            y, h = np.ascontiguousarray(gy[:, idx]), np.ascontiguousarray(gh[:, :, idx])
        csi_in = rng.uniform(0.05, 3.0, nof_re).astype(np.float32) if group == "csi" and kind == "single" and detail is None else None
        out.append((y, h, gy, gh, csi_in, [M.cn(rng, 16).astype(np.complex64) for _ in mods]))
    return out


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_pdsch_grant_soft_bits_against_the_oracle(hiplib, case):
    lib, capi = _lib()
    group, path, _, mods, llr8, gain, skip = case
    kind, ports, nrx, detail = PATHS[path]
    weight = group == "csi"
    dt = np.int8 if llr8 else np.int16
    nof_re = nof_re_of(case)
    sfd = sf_cell(SF_PATHS[path]) if group == "sf" else None
    if sfd is not None:
        assert lib.srsran_hip_pdsch_nof_re(C.byref(PM.to_struct(capi, sfd))) == nof_re and sf_count_is_off_the_group(path, nof_re), nof_re
    tbm = tuple((mod, tbs_of(mod, nof_re)) for mod in mods)
    segs = [O.cbsegm(tbs) for _, tbs in tbm]
    sbs = [_rx_softbuffer(capi, seg["C"] + 1, dt) for seg in segs]  # (one row more than the block has: it stays zero)
    soft = [np.zeros((seg["C"], SB), dt) for seg in segs]
    crc = [np.zeros(seg["C"], np.uint8) for seg in segs]
    seen = []
    for rv, (y, h, gy, gh, csi_in, more) in enumerate(inputs_of(case)):
        xs, csis = _stage(lib, capi, path, y, h, csi_in)
        want = []
        for k, (mod, tbs) in enumerate(tbm):
            e = oracle_bits(mod, xs[k], llr8, _seed(k))
            if rv == 0 and (has_tail(mod, llr8, nof_re) or (mod == 1 and gain)):  # on the transmission whose e_out is compared below
                seen.append(tail_is_seen(mod, xs[k], llr8, _seed(k), e, more[k]))
            want.append(CM.csi_model(e, csis[k], mod, llr8) if weight else e)
        if rv == 0:  # the intermediate results, on soft buffers of their own
            spare = [_rx_softbuffer(capi, seg["C"], dt) for seg in segs]
            for k, (res, data, d_out, e_out) in enumerate(_grant_call(lib, capi, path, gy, gh, csi_in, tbm, rv, llr8, spare, weight, True, skip, sfd)):
                nbits = nof_re * O.QM[mods[k]]
                if kind == "single" and detail is None:  # ce == NULL: d_out is never written
                    assert np.all(d_out == D_GUARD)
                else:
                    assert np.array_equal(np.ascontiguousarray(d_out[:nof_re]).view(np.uint32), np.ascontiguousarray(xs[k]).view(np.uint32)), (k, "d_out")
                    assert np.all(d_out[nof_re:] == D_GUARD), k
                if k == skip:
                    assert np.all(e_out == E_GUARD), k
                    continue
                bad = np.flatnonzero(e_out[:nbits] != want[k])
                assert bad.size == 0, "codeword %d: %d of %d soft bits differ, the first at %d (symbol %d of %d): %d, the oracle has %d" % (
                    k, bad.size, nbits, bad[0], bad[0] // O.QM[mods[k]], nof_re, e_out[bad[0]], want[k][bad[0]])
                assert np.all(e_out[nbits:] == E_GUARD), k
        got = _grant_call(lib, capi, path, gy, gh, csi_in, tbm, rv, llr8, sbs, weight, False, skip, sfd)
        for k, (mod, tbs) in enumerate(tbm):
            res, data, d_out, e_out = got[k]
            sb, rows, _, flags = sbs[k]
            assert np.all(d_out == D_GUARD) and np.all(e_out == E_GUARD), (rv, k)
            if k == skip:  # res = {0, 0, NAN}, the payload and the rows untouched
                assert res.crc_ok == 0 and res.avg_iterations_block == 0.0 and np.isnan(res.epre) and np.all(data == 0xA5), (rv, k)
                assert not any(r.any() for r in rows), (rv, k)
                continue
            seg, nb = segs[k], segs[k]["C"]
            ret, _, avg = O.sch_decode_tb(tbs, O.QM[mod] * (2 if kind == "txdiv" else 1), rv, want[k], soft[k], crc[k], ITERS)
            assert ret == -1 and not crc[k].any(), (rv, k, ret, crc[k])  # the precondition: no block decodes, so every row comes back
            assert res.crc_ok == 0 and not sb.tb_crc and not flags.any(), (rv, k)
            assert abs(res.avg_iterations_block - avg) < 1e-6, (rv, k, res.avg_iterations_block, avg)
            for i in range(nb):
                span = 3 * ((seg["K1"] if i < seg["C1"] else seg["K2"]) + 32) + 12
                bad = np.flatnonzero(rows[i][:span] != soft[k][i][:span])
                assert bad.size == 0, "rv %d codeword %d block %d: %d of %d entries differ, the first at %d: %d, the oracle has %d" % (
                    rv, k, i, bad.size, span, bad[0], rows[i][bad[0]], soft[k][i][bad[0]])
                assert not rows[i][span:].any() and not soft[k][i][span:].any(), (rv, k, i)
            assert not rows[nb].any(), (rv, k)
            assert np.all(data[tbs // 8 + (6 if nb > 1 else 3):] == 0xA5), (rv, k)
    print("%s: soft bits that the tail rule decides, per codeword: %s" % (_id(case), seen))
