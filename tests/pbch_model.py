"""numpy model of PBCH / MIB decoding as the reference runs it (phch/pbch.c): the RE map of srsran_pbch_get, the three control-channel equalisers
(pdcch_map_model.equalise; the one-port one takes the WHOLE noise estimate here), decode_frame (pbch.c:399-434) on top of conv_model, and srsran_pbch_decode
(:444-557) with the state it carries from call to call.  float32, one rounding per operation.  tests/golden/pbch_ref.npz holds what the reference itself
gave (tools/gen_golden_pbch.py).

A cell is a dict(nof_prb, nof_ports, id, cp_nsymb); nof_ports 0 searches 1, 2 and 4.  A state is dict(frame_idx, llr float32[4, nof_bits])."""
import numpy as np

import conv_model as CM
import pdcch_map_model as PM

F32 = np.float32
CRC_MASK = {1: 0x0000, 2: 0xFFFF, 4: 0x5555}  # srsran_crc_mask as 16-bit words, first bit highest
_SEQ = {}


def cell(nof_prb, nof_ports, cell_id, cp_nsymb=7):
    return dict(nof_prb=nof_prb, nof_ports=nof_ports, id=cell_id, cp_nsymb=cp_nsymb)


def as_row(c):
    return np.array([c["nof_prb"], c["nof_ports"], c["id"], c["cp_nsymb"]], np.uint32)


def from_row(row):
    return dict(zip(("nof_prb", "nof_ports", "id", "cp_nsymb"), (int(v) for v in row)))


def nof_re(c):
    return 240 if c["cp_nsymb"] == 7 else 216


def rows_table(c):
    """(symbol of slot 1, sub-carrier among the 72) of every RE srsran_pbch_get reads, in its order"""
    o, out = c["id"] % 3, []
    for row in range(4):
        skips = row < 2 or (c["cp_nsymb"] == 6 and row == 3)
        out += [(row, j) for j in range(72) if not (skips and j % 3 == o)]
    return out


def table(c):
    """indices into the grid of slot 1 (rows of 12 nof_prb)"""
    k0 = c["nof_prb"] * 6 - 36
    return np.array([r * 12 * c["nof_prb"] + k0 + j for r, j in rows_table(c)], np.uint32)


def staged_table(c):
    """indices into the 4 x 72 rows a call stages"""
    return np.array([r * 72 + j for r, j in rows_table(c)], np.uint32)


def slot1_rows(c, grid):
    """the 4 x 72 points of a whole-subframe grid that the channel lies on"""
    g = np.asarray(grid, np.complex64).reshape(2 * c["cp_nsymb"], 12 * c["nof_prb"])
    k0 = c["nof_prb"] * 6 - 36
    return g[c["cp_nsymb"]:c["cp_nsymb"] + 4, k0:k0 + 72].copy()


def combos(f):
    """the (nb, dst, src) of frame_idx f in the reference's order: 4, 11, 20 or 30"""
    return [(nb, dst, src) for nb in range(f) for dst in range(4 - nb) for src in range(f - nb)]


def nant_list(c):
    return [1, 2, 4] if c["nof_ports"] == 0 else [c["nof_ports"]]


def sequence(cell_id, n=1920):
    """TS 36.211 7.2 with c_init = cell_id"""
    if cell_id not in _SEQ:
        x1, x2 = [0] * (1600 + 1920 + 31), [0] * (1600 + 1920 + 31)
        x1[0] = 1
        for i in range(31):
            x2[i] = (cell_id >> i) & 1
        for k in range(1600 + 1920):
            x1[k + 31] = x1[k + 3] ^ x1[k]
            x2[k + 31] = x2[k + 3] ^ x2[k + 2] ^ x2[k + 1] ^ x2[k]
        _SEQ[cell_id] = np.array([x1[k + 1600] ^ x2[k + 1600] for k in range(1920)], np.uint8)
    return _SEQ[cell_id][:n]


def mib_unpack(payload):
    """srsran_pbch_mib_unpack -> (nof_prb, phich_length, phich_resources, sfn)"""
    b = [int(v) & 1 for v in payload]
    bw = b[0] << 2 | b[1] << 1 | b[2]
    sfn = 0
    for v in b[6:14]:
        sfn = sfn << 1 | v
    return (6 if bw == 0 else 15 if bw == 1 else (bw - 1) * 25), b[3], b[4] << 1 | b[5], sfn << 2


def mib_pack(nof_prb, phich_length, phich_resources, sfn):
    """srsran_pbch_mib_pack (inputs only)"""
    bw = 0 if nof_prb <= 6 else 1 if nof_prb <= 15 else 1 + nof_prb // 25
    bits = [(bw >> 2) & 1, (bw >> 1) & 1, bw & 1, phich_length, (phich_resources >> 1) & 1, phich_resources & 1] + [((sfn >> 2) >> (7 - i)) & 1 for i in range(8)]
    return np.array(bits + [0] * 10, np.uint8)


# ---------------------------------------------------------------------------------------------------------------- front end
def equalise(rx_rows, ce_rows, c, nant, noise_estimate):
    """rx_rows [4, 72], ce_rows [port][4, 72] -> d (complex64[nof_re]) of antenna hypothesis nant"""
    t = staged_table(c)
    y = np.asarray(rx_rows, np.complex64).ravel()[t][None, :]
    h = np.array([[np.asarray(ce_rows[p], np.complex64).ravel()[t]] for p in range(nant)])
    # pdcch_map_model halves its one-port noise estimate (pdcch.c:471); the PBCH hands over the whole one (pbch.c:508): twice the value is exact
    return PM.equalise(y, h, nant, F32(noise_estimate) * F32(2) if nant == 1 else 0)


def soft_bits(d):
    """srsran_demod_soft_demodulate, QPSK to float"""
    d = np.asarray(d, np.complex64)
    llr = np.empty(2 * d.size, F32)
    k = F32(-PM.SQRT2)
    llr[0::2], llr[1::2] = d.real * k, d.imag * k
    return llr


# ---------------------------------------------------------------------------------------------------------------- decode_frame
def rm_rx_fast(temp, coded_len=120):
    """conv_model.rm_rx_owner with the output positions side by side: the same sums in the same order"""
    temp = np.asarray(temp, F32)
    first = np.array([CM.rm_rank(o, coded_len) for o in range(coded_len)])
    t = np.full(coded_len, CM.RX_NULL, F32)
    for j in range((temp.size + coded_len - 1) // coded_len):
        k = first + j * coded_len
        ok = k < temp.size
        v = np.where(ok, temp[np.minimum(k, temp.size - 1)], CM.RX_NULL).astype(F32)
        empty = t == CM.RX_NULL
        add = ok & ~empty & (v != CM.RX_NULL)
        t = np.where(ok & empty, v, np.where(add, (t + v).astype(F32), t)).astype(F32)
    return np.where(t == CM.RX_NULL, F32(0), t).astype(F32)


def decode_frame(llr, src, dst, n, nof_bits, cell_id):
    """-> dict(rm_f float32[120] behind the product with 1 / (2 n), sym uint16[120], bits uint8[40], crc_rem, ones)"""
    llr = np.asarray(llr, F32).reshape(-1)
    temp = np.full(4 * nof_bits, CM.RX_NULL, F32)
    w = llr[src * nof_bits:(src + n) * nof_bits].copy()
    c = sequence(cell_id)[dst * nof_bits:(dst + n) * nof_bits].astype(bool)
    w[c] = -w[c]
    temp[dst * nof_bits:(dst + n) * nof_bits] = w
    rm = (rm_rx_fast(temp) * F32(1.0 / float(F32(2) * F32(n)))).astype(F32)
    sym = CM.quant_f(rm)
    bits = CM.decode(sym, 40, True)["bits"]
    parity = int(sum(int(b) << (15 - i) for i, b in enumerate(bits[24:])))
    return dict(rm_f=rm, sym=sym, bits=bits, crc_rem=parity ^ CM.crc16(bits[:24]), ones=int(bits[:24].sum()))


def verdict(r, nant):
    return r["crc_rem"] == CRC_MASK[nant] and r["ones"] != 0


def try_frames(c, llr, f):
    nof_bits = 2 * nof_re(c)
    return [decode_frame(llr, src, dst, nb + 1, nof_bits, c["id"]) for nb, dst, src in combos(f)]


# ---------------------------------------------------------------------------------------------------------------- the call
def new_state(c):
    return dict(frame_idx=0, llr=np.zeros((4, 2 * nof_re(c)), F32))


def decode(c, state, rx_rows, ce_rows, noise_estimate, stop_at_hit=True):
    """srsran_pbch_decode -> (res, new state, dbg).  res: dict(ret, nof_tx_ports, sfn_offset, src, dst, nb, payload); dbg: dict(d, llr_new: per antenna
    hypothesis tried, tried: the (nant, nb, dst, src) the reference saw before its return, with rows: their decode_frame results).
    The library's state keeps the LAST hypothesis's newest row (its waves are independent); the reference's keeps the hit's on a hit, in a row that is never
    read again.  With stop_at_hit the model does as the reference."""
    nof_bits = 2 * nof_re(c)
    f = state["frame_idx"] + 1
    llr = state["llr"].copy()
    res = dict(ret=0, nof_tx_ports=0, sfn_offset=0, src=0, dst=0, nb=0, payload=np.zeros(24, np.uint8))
    dbg = dict(d={}, llr_new={}, tried=[], rows=[])
    for nant in nant_list(c):
        d = equalise(rx_rows, ce_rows, c, nant, noise_estimate)
        dbg["d"][nant] = d
        llr[f - 1] = soft_bits(d)
        dbg["llr_new"][nant] = llr[f - 1].copy()
        if res["ret"]:
            continue
        for nb, dst, src in combos(f):
            r = decode_frame(llr, src, dst, nb + 1, nof_bits, c["id"])
            dbg["tried"].append((nant, nb, dst, src))
            dbg["rows"].append(r)
            if verdict(r, nant):
                res = dict(ret=1, nof_tx_ports=nant, sfn_offset=dst - src + f - 1, src=src, dst=dst, nb=nb, payload=r["bits"][:24].copy())
                break
        if res["ret"] and stop_at_hit:
            break
    out = dict(frame_idx=0 if res["ret"] else f, llr=llr)
    if out["frame_idx"] == 4:
        out["llr"][:3] = out["llr"][1:].copy()
        out["frame_idx"] = 3
    return res, out, dbg


# ---------------------------------------------------------------------------------------------------------------- the record (tests/golden/pbch_ref.npz)
CALL_FIELDS = ("rx_rows", "ce_rows", "noise", "f_in", "ret", "ports", "off", "payload", "comb", "f_out", "llr", "d", "d_nant", "sent")


def record_sequences(d):
    """-> [dict(name, cell, full, pilots, calls: [dict of CALL_FIELDS (+ rx, the whole received grid, where full)])]"""
    out = []
    for si, name in enumerate(d["c_names"]):
        full = bool(d["c_full"][si])
        calls = []
        for i in range(int(d["c_ncalls"][si])):
            c = {k: d["c_%s_%d_%d" % (k, si, i)] for k in CALL_FIELDS}
            if full:
                c["rx"] = d["c_rx_%d_%d" % (si, i)]
            calls.append(c)
        out.append(dict(name=str(name), cell=from_row(d["c_cells"][si]), full=full, pilots=(d["c_pilots0_%d" % si], d["c_pilots1_%d" % si]) if full else None,
                        calls=calls))
    return out


def state_before(c, seq, i):
    """the reference's state in front of call i of a recorded sequence"""
    st = new_state(c)
    if i > 0:
        prev = seq["calls"][i - 1]
        st["frame_idx"] = int(prev["f_out"])
        st["llr"][:st["frame_idx"]] = prev["llr"]
    assert st["frame_idx"] == int(seq["calls"][i]["f_in"])
    return st
