"""A literal numpy restatement of the reference's PUSCH transmit side with control information: srsran_ulsch_encode (lib/src/phy/phch/sch.c:1194-1337, with
ulsch_interleave :932-990 and the positions of uci.c:364-416) and what srsran_pusch_encode does with its result (pusch.c:299-340: scrambling, the placeholder /
repetition fix-up, modulation, transform precoding, pusch_put).  Every stage is returned.  The two loops over the ACK / RI bits -- the write of sch.c:1321-1332
and the fix-up of pusch.c:317-331 -- are written as the reference writes them, over the list in list order (RI first); nothing here knows the closed form the
kernel uses.  The transport block's coded bits, the scrambling sequence and the constellation come from the oracle (tests/oracle_api.py); the transform is the
float64 FFT tests/test_gpu_chan.py uses.

Also here: encode_ri_ack (uci.c:457-486, 1 and 2 bits), the repetition of srsran_uci_encode_ack_ri (uci.c:603-610) and uci_ack_scramble_tdd (uci.c:546-579), so
that the tests feed the type patterns the reference's encoders produce.  The block codes (more than two ACK bits, CQI) are not restated: the library does not
build them either."""
import numpy as np

import oracle_api as O

UCI_BIT_0, UCI_BIT_1, UCI_BIT_REPETITION, UCI_BIT_PLACEHOLDER = 0, 1, 2, 3
ACK_COLS = {True: (2, 3, 8, 9), False: (1, 2, 6, 7)}
RI_COLS = {True: (1, 4, 7, 10), False: (0, 3, 5, 8)}
W_SCRAM = ((1, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 0), (1, 0, 0, 1))  # Table 5.2.2.6-A


# ---- the small encoders ------------------------------------------------------------------------------------------------------------------------------------

def encode_ri_ack(data, O_ack, Qm):
    """uci.c:457-486: the types of one period"""
    t = []
    if O_ack == 1:
        t.append(UCI_BIT_1 if data[0] else UCI_BIT_0)
        t.append(UCI_BIT_REPETITION)
        while len(t) < Qm:
            t.append(UCI_BIT_PLACEHOLDER)
    elif O_ack == 2:
        x = data[0] ^ data[1]
        for a, b, end in ((data[0], data[1], Qm), (x, data[0], 2 * Qm), (data[1], x, 3 * Qm)):
            t.append(UCI_BIT_1 if a else UCI_BIT_0)
            t.append(UCI_BIT_1 if b else UCI_BIT_0)
            while len(t) < end:
                t.append(UCI_BIT_PLACEHOLDER)
    return t


def uci_ack_scramble_tdd(types, O_ack, N_bundle):
    """uci.c:548-579, in place on a list of types"""
    if N_bundle == 0:
        return types
    wi = (N_bundle - 1) % 4
    m = 1 if O_ack == 1 else 3
    q_m1 = types[0]
    k = 0
    for i in range(len(types)):
        if types[i] == UCI_BIT_REPETITION:
            if i > 0:
                types[i] = ((1 if q_m1 == UCI_BIT_1 else 0) + W_SCRAM[wi][k // m]) % 2
            k = (k + 1) % (4 * m)
        elif types[i] == UCI_BIT_PLACEHOLDER:
            pass
        else:
            q_m1 = types[i]
            types[i] = ((1 if types[i] == UCI_BIT_1 else 0) + W_SCRAM[wi][k // m]) % 2
            k = (k + 1) % (4 * m)
    return types


def ack_ri_types(data, O_ack, Qm, Q_prime, N_bundle=0, is_ri=False):
    """srsran_uci_encode_ack_ri for 1 or 2 bits (uci.c:603-628): the period repeated over Q_prime symbols (what runs over is ignored), TDD scrambling for ACK"""
    enc = encode_ri_ack(data, O_ack, Qm)
    t = []
    while len(t) < Q_prime * Qm:
        t.extend(enc)
    t = t[:Q_prime * Qm]
    if t and not is_ri and N_bundle:
        uci_ack_scramble_tdd(t, O_ack, N_bundle)
    return np.array(t, np.uint8)


def long_ack_types(code_word, Qm, Q_prime):
    """encode_ack_long (uci.c:488-510) behind its block code: the 32 coded bits repeated, types 0 / 1 only"""
    cw = np.asarray(code_word, np.uint8)
    assert cw.size == 32
    return cw[np.arange(Q_prime * Qm) % 32].copy()


# ---- srsran_ulsch_encode -------------------------------------------------------------------------------------------------------------------------------------

def positions(n, Qm, H, cols, sets):
    """uci.c:364-416: the Qm positions of ACK / RI symbol n in q_bits"""
    rows = H // cols
    assert rows >= 1 + n // 4
    row = rows - 1 - n // 4
    col = sets[cols > 10][(3 * n) % 4]
    return [row * Qm + rows * col * Qm + k for k in range(Qm)]


def ulsch_encode(e, cqi_bits, ri_types, ack_types, H, cols, Qm):
    """sch.c:1194-1337 behind the block codes.  e: the transport block's (H - Q'ri - Q'cqi) Qm coded bits (uint8, one per entry); cqi_bits: Q'cqi Qm; ri_types,
    ack_types: Q' Qm type bytes each.  Returns (q_bits uint8 [H Qm], the ack_ri_bits list [(position, type)]: RI first, then ACK)"""
    e, cqi_bits, ri_types, ack_types = (np.asarray(a, np.uint8) for a in (e, cqi_bits, ri_types, ack_types))
    Qr, Qa, Qc = ri_types.size // Qm, ack_types.size // Qm, cqi_bits.size // Qm
    rows = H // cols
    assert e.size == (H - Qr - Qc) * Qm
    g = np.concatenate([cqi_bits, e])  # the CQI code word in front, the transport block at bit offset Q'cqi Qm (encode_tb_off)
    lst = []
    for n in range(Qr):
        for k, p in enumerate(positions(n, Qm, H, cols, RI_COLS)):
            lst.append((p, int(ri_types[n * Qm + k])))
    # ulsch_interleave: whole symbols row by row, around the symbols whose first bit is an RI position
    ri_present = np.zeros(H * Qm, bool)
    for p, _ in lst:
        ri_present[p] = True
    q = np.zeros(H * Qm, np.uint8)
    rd = 0
    for j in range(rows):
        for i in range(cols):
            k = (i * rows + j) * Qm
            if ri_present[k]:
                continue
            q[k:k + Qm] = g[rd:rd + Qm]
            rd += Qm
    assert rd == g.size
    for n in range(Qa):
        for k, p in enumerate(positions(n, Qm, H, cols, ACK_COLS)):
            lst.append((p, int(ack_types[n * Qm + k])))
    for p, t in lst:  # sch.c:1321-1332
        assert p < H * Qm
        q[p] = 1 if t == UCI_BIT_1 else 0
    return q, lst


# ---- srsran_pusch_encode behind srsran_ulsch_encode --------------------------------------------------------------------------------------------------------

def scramble_and_fix(q, lst, seed):
    """pusch.c:308-331: (scrambled bits before the fix-up, after it)"""
    scr = q ^ O.sequence_bits(seed, q.size)
    d = scr.copy()
    for p, t in lst:
        if t == UCI_BIT_PLACEHOLDER:
            d[p] = 1
        elif t == UCI_BIT_REPETITION:
            if p > 1:
                d[p] = d[p - 1]
    return scr, d


def put_grid(grid, z, cp_nsymb, n_prb, L_prb, shortened):
    """pusch.c:48-100 pusch_put: the rows of z into grid [2 cp_nsymb, 12 nof_prb], skipping each slot's reference symbol and, when shortened, the last symbol"""
    L_ref = 3 if cp_nsymb == 7 else 2
    row = 0
    for slot in range(2):
        nl = cp_nsymb - (1 if (shortened and slot == 1) else 0)
        for l in range(nl):
            if l == L_ref:
                continue
            a = 12 * n_prb[slot]
            grid[l + slot * cp_nsymb, a:a + 12 * L_prb] = z[row]
            row += 1
    assert row == z.shape[0]
    return grid


def pusch_encode(mod, e, cqi_bits, ri_types, ack_types, cols, L_prb, seed):
    """every stage of srsran_pusch_encode: dict with q_ulsch (srsran_ulsch_encode's bits), lst, q_scr (scrambled, before the fix-up), q_tx (after it: q->q),
    d (q->d), z (q->z as [cols, 12 L_prb])"""
    Qm = O.QM[mod]
    nsc = 12 * L_prb
    H = cols * nsc
    q, lst = ulsch_encode(e, cqi_bits, ri_types, ack_types, H, cols, Qm)
    scr, tx = scramble_and_fix(q, lst, seed)
    d = O.modulate_bytes(mod, np.packbits(tx), H * Qm)
    z = (np.fft.fft(d.reshape(cols, nsc).astype(np.complex128), axis=1) / np.sqrt(nsc)).astype(np.complex64)  # srsran_dft_precoding, tx: forward, normalised
    return dict(q_ulsch=q, lst=lst, q_scr=scr, q_tx=tx, d=d, z=z)
