"""Integer / float32 numpy model of the LTE convolutional-code receive chain as the reference runs it on an AVX2 host: the rate de-matcher
(srsran_rm_conv_rx, fec/turbo/rm_conv.c:93-152), the quantisers of srsran_viterbi_decode_f / _s (fec/convolutional/viterbi.c:548-606), the 16-bit 64-state
decoder (viterbi37_avx2_16bit.c:201-351 driven by decode37_avx2_16bit, viterbi.c:129-157) and the 16-bit CRC of srsran_pdcch_dci_decode (phch/pdcch.c:335-368).
The transmit side ((133, 171, 165) encoder, srsran_rm_conv_tx) is here only to make inputs.

The decoder is stated twice: step_intrinsics() restates the AVX2 intrinsics one by one (permute, unpack, pack, movemask, byte swap, the normalisation
block with its 16-byte lane shift), step() is the plain form the kernel runs (lane s is new state s, bit s of the decision word is state s).
tests/test_conv_golden.py shows that they are the same mapping; the record (tests/golden/conv_ref.npz) holds what the reference itself gave.

What the restatement shows and the record confirms:
  * the start metrics are all 0 with and without tail biting: init_viterbi37_avx2_16bit fills metrics1 with 63 and then calls clear_v37_avx2_16bit, which
    zeroes it again, so without tail biting state 0 gets no head start either;
  * the normalisation never subtracts: _mm256_srli_si256(x, 16) shifts each 128-bit lane out completely, the minimum comes out 0; the metrics wrap mod 2^16;
  * the chain-back reads decision word t = nbits + 6 ("look past tail").  With tail biting 3 L steps were run, so the six words 3 L .. 3 L + 5 are the zeros
    clear_v37 left: the first six chain-back steps shift zeros in, whatever the best state was, and the chain-back proper starts from state 0 at step
    3 L - 1.  The best state is computed and has no effect on the bits.
"""
import numpy as np

POLY = (0x6D, 0x4F, 0x57)  # (133, 171, 165) octal: lte convolutional code, phch/pdcch.c, phch/pbch.c
RX_NULL = np.float32(10000.0)  # SRSRAN_RX_NULL
TX_NULL = 100  # SRSRAN_TX_NULL
NCOLS = 32
PERM = np.array([1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30])
PERM_INV = np.array([16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14, 17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15])
DEFAULT_GAIN_16 = np.float32(1000.0)
QUANT_CONTRACTED = True  # the reference's quantiser sum is one fused multiply-add (-mfma -O3): decided by the record, asserted by tools/gen_golden_conv.py


def parity(x):
    return bin(int(x)).count("1") & 1


# ---------------------------------------------------------------------------------------------------------------- transmit side (inputs only)
def encode(bits, tail_biting=True):
    """srsran_convcoder_encode, K = 7, R = 3"""
    bits = np.asarray(bits, np.uint8)
    L = bits.size
    sr = 0
    if tail_biting:
        for i in range(L - 6, L):
            sr = (sr << 1) | int(bits[i] & 1)
    n = L if tail_biting else L + 6
    out = np.zeros(3 * n, np.uint8)
    for i in range(n):
        sr = ((sr << 1) | (int(bits[i] & 1) if i < L else 0)) & 0x7F
        for j in range(3):
            out[3 * i + j] = parity(sr & POLY[j])
    return out


def rm_geometry(coded_len):
    nrows = (coded_len // 3 - 1) // NCOLS + 1
    K_p = nrows * NCOLS
    return nrows, K_p, max(K_p - coded_len // 3, 0)


def rm_tx(coded, E):
    """srsran_rm_conv_tx"""
    coded = np.asarray(coded, np.uint8)
    nrows, K_p, ndummy = rm_geometry(coded.size)
    tmp = []
    for s in range(3):
        for j in range(NCOLS):
            for i in range(nrows):
                p = i * NCOLS + PERM[j]
                tmp.append(TX_NULL if p < ndummy else int(coded[(p - ndummy) * 3 + s]))
    out, j = [], 0
    while len(out) < E:
        if tmp[j] != TX_NULL:
            out.append(tmp[j])
        j = (j + 1) % (3 * K_p)
    return np.array(out, np.uint8)


def crc16(bits):
    """srsran_crc_checksum with SRSRAN_LTE_CRC16 (0x11021) on one bit per byte"""
    crc = 0
    for b in bits:
        crc = ((crc << 1) ^ (0x1021 if ((crc >> 15) & 1) ^ int(b & 1) else 0)) & 0xFFFF
    return crc


def dci_encode(payload, rnti, E):
    """srsran_pdcch_dci_encode: CRC attached and masked with the RNTI, encoder, rate matcher.  payload: nof_bits bits"""
    payload = np.asarray(payload, np.uint8)
    c = crc16(payload) ^ rnti
    data = np.concatenate([payload, np.array([(c >> (15 - i)) & 1 for i in range(16)], np.uint8)])
    return rm_tx(encode(data, True), E)


# ---------------------------------------------------------------------------------------------------------------- rate de-matcher
def rm_rx(llr, coded_len):
    """srsran_rm_conv_rx as written: float32 sums in the order of the input, the SRSRAN_RX_NULL comparisons included"""
    llr = np.asarray(llr, np.float32)
    nrows, K_p, ndummy = rm_geometry(coded_len)
    tmp = np.full(3 * K_p, RX_NULL, np.float32)
    k = j = 0
    while k < llr.size:
        d_i, d_j = (j % K_p) // nrows, (j % K_p) % nrows
        if d_j * NCOLS + PERM[d_i] >= ndummy:
            if tmp[j] == RX_NULL:
                tmp[j] = llr[k]
            elif llr[k] != RX_NULL:
                tmp[j] = np.float32(tmp[j] + llr[k])
            k += 1
        j = (j + 1) % (3 * K_p)
    out = np.zeros(coded_len, np.float32)
    for i in range(coded_len // 3):
        d_i, d_j = (i + ndummy) // NCOLS, (i + ndummy) % NCOLS
        for s in range(3):
            o = tmp[K_p * s + PERM_INV[d_j] * nrows + d_i]
            out[3 * i + s] = o if o != RX_NULL else np.float32(0)
    return out


def rm_rank(o, coded_len):
    """the kernel's form: the index of the first input that lands on output position o; the others follow every coded_len inputs"""
    nrows, K_p, ndummy = rm_geometry(coded_len)
    i, s = o // 3, o % 3
    row, col = (i + ndummy) // NCOLS, PERM_INV[(i + ndummy) % NCOLS]
    dummies = s * ndummy + sum(1 for c in range(col) if PERM[c] < ndummy) + (1 if row > 0 and PERM[col] < ndummy else 0)
    return K_p * s + col * nrows + row - dummies


def rm_rx_owner(llr, coded_len):
    """each output position walks its own contributions in increasing k: the same sums in the same order"""
    llr = np.asarray(llr, np.float32)
    out = np.zeros(coded_len, np.float32)
    for o in range(coded_len):
        t = RX_NULL
        for k in range(rm_rank(o, coded_len), llr.size, coded_len):
            if t == RX_NULL:
                t = llr[k]
            elif llr[k] != RX_NULL:
                t = np.float32(t + llr[k])
        out[o] = t if t != RX_NULL else np.float32(0)
    return out


# ---------------------------------------------------------------------------------------------------------------- quantisers
def fma32(a, b, c):
    """float32 fused multiply-add, correctly rounded: the product is exact in float64, the sum is rounded to odd there (TwoSum gives the error) and then
    once to float32"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def quant_f(x, gain_quant=DEFAULT_GAIN_16, contracted=None):
    """srsran_viterbi_decode_f's front end: max = 1e-9 raised by every fabs, srsran_vec_quant_fus(x, ., gain_quant / max, 32767.5, 65535)"""
    x = np.asarray(x, np.float32)
    mx = max(np.float32(1e-9), np.max(np.abs(x))) if x.size else np.float32(1e-9)
    gain = np.float32(np.float32(gain_quant) / np.float32(mx))
    with np.errstate(over="ignore", invalid="ignore"):
        if QUANT_CONTRACTED if contracted is None else contracted:
            v = fma32(np.full(x.shape, gain, np.float32), x, np.float32(32767.5))
        else:
            v = (np.float32(32767.5) + (gain * x).astype(np.float32)).astype(np.float32)
    return np.clip(np.trunc(v.astype(np.float64)), 0, 65535).astype(np.uint16)


def quant_s(x):
    """srsran_viterbi_decode_s's front end: srsran_vec_quant_sus(x, ., 1, 32767, 65535)"""
    return np.clip(32767 + np.asarray(x, np.int16).astype(np.int64), 0, 65535).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- decoder
def sign_table():
    """Branchtab37_sse2[k].c[i], set_viterbi37_polynomial_avx2_16bit"""
    return np.array([[65535 if parity((2 * i) & POLY[k]) else 0 for i in range(32)] for k in range(3)], np.uint16)


SIGNS = sign_table()


def step(old, s0, s1, s2):
    """one trellis step in the plain form: (new metrics uint16[64], decision word with bit s = state s, whether an add left 16 bits)"""
    t = [SIGNS[k].astype(np.uint32) ^ np.uint32(s) for k, s in enumerate((s0, s1, s2))]
    m = (t[0] + t[1] + 1) >> 1
    metric = ((t[2] + m + 1) >> 1) >> 3
    m_metric = 8191 - metric
    a, c = old[:32].astype(np.uint32), old[32:].astype(np.uint32)
    carry = bool(np.any(np.maximum(a, c) + 8191 > 0xFFFF) and np.any(np.concatenate([a + metric, c + m_metric, a + m_metric, c + metric]) > 0xFFFF))
    m0, m1, m2, m3 = (a + metric) & 0xFFFF, (c + m_metric) & 0xFFFF, (a + m_metric) & 0xFFFF, (c + metric) & 0xFFFF
    d0 = ((m0 - m1) & 0xFFFF).astype(np.uint16).view(np.int16) > 0
    d1 = ((m2 - m3) & 0xFFFF).astype(np.uint16).view(np.int16) > 0
    new = np.empty(64, np.uint16)
    new[0::2] = np.where(d0, m1, m0)
    new[1::2] = np.where(d1, m3, m2)
    dec = np.zeros(64, np.uint8)
    dec[0::2], dec[1::2] = d0, d1
    return new, int(np.packbits(dec, bitorder="little").view(np.uint64)[0]), carry


# -- the AVX2 intrinsics on arrays of 16 uint16 (one __m256i)
def _avg_epu16(a, b):
    return ((a.astype(np.uint32) + b.astype(np.uint32) + 1) >> 1).astype(np.uint16)


def _permute4x64_216(a):  # imm 216 = 0b11011000: quadwords 0, 2, 1, 3
    q = a.reshape(4, 4)
    return np.concatenate([q[0], q[2], q[1], q[3]])


def _unpack_epi16(a, b, hi):
    out = np.empty(16, np.uint16)
    for lane in range(2):
        src = lane * 8 + (4 if hi else 0)
        for k in range(4):
            out[lane * 8 + 2 * k], out[lane * 8 + 2 * k + 1] = a[src + k], b[src + k]
    return out


def _packus_epi16(a, b):  # 32 bytes: per 128-bit lane, 8 from a then 8 from b, signed words saturated to 0..255
    sat = lambda v: np.clip(v.view(np.int16).astype(np.int32), 0, 255).astype(np.uint8)  # noqa: E731
    return np.concatenate([sat(a[0:8]), sat(b[0:8]), sat(a[8:16]), sat(b[8:16])])


def _movemask_epi8(x):
    return int(sum(int(v >> 7) << i for i, v in enumerate(x)))


def _srli_si256(a, nbytes):  # a BYTE shift inside each 128-bit lane; 16 or more gives zero
    by = a.view(np.uint8).reshape(2, 16)
    out = np.zeros((2, 16), np.uint8)
    if nbytes < 16:
        out[:, :16 - nbytes] = by[:, nbytes:]
    return out.reshape(-1).view(np.uint16).copy()


def step_intrinsics(old, s0, s1, s2):
    """update_viterbi37_blk_avx2_16bit's loop body, intrinsic by intrinsic: (new metrics, the 8 bytes of decision_t)"""
    ov = old.reshape(4, 16)
    nv = np.zeros((4, 16), np.uint16)
    dbytes = np.zeros(8, np.uint8)
    syms = [np.full(16, s, np.uint16) for s in (s0, s1, s2)]
    for i in range(2):
        bt = [SIGNS[k][16 * i:16 * i + 16] for k in range(3)]
        m0 = _avg_epu16(bt[0] ^ syms[0], bt[1] ^ syms[1])
        metric = _avg_epu16(bt[2] ^ syms[2], m0) >> 3
        m_metric = (np.uint16(8191) - metric).astype(np.uint16)
        m0, m3 = ov[i] + metric, ov[2 + i] + metric  # uint16: wraps
        m1, m2 = ov[2 + i] + m_metric, ov[i] + m_metric
        d0 = np.where((m0 - m1).view(np.int16) > 0, 0xFFFF, 0).astype(np.uint16)
        d1 = np.where((m2 - m3).view(np.int16) > 0, 0xFFFF, 0).astype(np.uint16)
        sv0 = (d0 & m1) | (~d0 & m0)
        sv1 = (d1 & m3) | (~d1 & m2)
        d0, d1 = _permute4x64_216(d0), _permute4x64_216(d1)
        packed = _packus_epi16(_unpack_epi16(d0, d1, False) >> 8, _unpack_epi16(d0, d1, True) >> 8)
        w = _movemask_epi8(packed)
        c = [(w >> (8 * b)) & 0xFF for b in range(4)]
        c[1], c[2] = c[2], c[1]
        dbytes[4 * i:4 * i + 4] = c
        sv0, sv1 = _permute4x64_216(sv0), _permute4x64_216(sv1)
        nv[2 * i], nv[2 * i + 1] = _unpack_epi16(sv0, sv1, False), _unpack_epi16(sv0, sv1, True)
    if nv[0][0] > 12288:  # "see if we need to normalize"
        adj = nv[0].copy()
        for i in range(1, 4):
            adj = np.minimum(adj, nv[i])
        for nbytes in (16, 8, 4):
            adj = np.minimum(adj, _srli_si256(adj, nbytes))
        nv = (nv - adj[0]).astype(np.uint16)
    return nv.reshape(-1), dbytes


def decision_bit(dbytes, state):
    """how chainback_viterbi37_avx2_16bit reads a decision_t (:147)"""
    return (int(dbytes[state // 8]) >> (state % 8)) & 1


def decode(sym, L, tail_biting=True, stepper=None):
    """decode37_avx2_16bit on uint16 symbols (3 L with tail biting, 3 (L + 6) without).
    -> dict(bits uint8[L], best_state, metrics uint16[64], best_moot: the best state had no effect on any bit, wrapped: an add left 16 bits)"""
    sym = np.asarray(sym, np.uint16)
    # init_viterbi37_avx2_16bit writes 63 into metrics1 and then calls clear_v37, which zeroes both metric buffers: every start metric is 0, and the
    # "bias" of the known start state without tail biting (c[0] = 0) changes nothing
    old = np.zeros(64, np.uint16)
    nsteps = 3 * L if tail_biting else L + 6
    stream = np.tile(sym[:3 * L], 3) if tail_biting else sym[:3 * (L + 6)]
    words, wrapped = [], False
    for t in range(nsteps):
        if stepper is None:
            old, w, carry = step(old, int(stream[3 * t]), int(stream[3 * t + 1]), int(stream[3 * t + 2]))
            wrapped = wrapped or carry
        else:
            old, by = stepper(old, int(stream[3 * t]), int(stream[3 * t + 1]), int(stream[3 * t + 2]))
            w = int(sum(int(b) << (8 * i) for i, b in enumerate(by)))
        words.append(w)
    best, minm = 0, 65535
    for i in range(64):  # an unsigned minimum with <=: the last index among equals
        if int(old[i]) <= minm:
            best, minm = i, int(old[i])

    def chainback(nbits, endstate):
        data = np.zeros(nbits, np.uint8)
        endstate = (endstate % 64) << 2
        for n in range(nbits - 1, -1, -1):
            w = words[n + 6] if n + 6 < nsteps else 0  # past the steps that ran: the zeros clear_v37 left (the allocation holds len + 6 words)
            k = (w >> (endstate >> 2)) & 1
            endstate = (endstate >> 1) | (k << 7)
            data[n] = k
        return data

    if tail_biting:
        full = chainback(3 * L, best)
        bits = full[L:2 * L].copy()
        moot = np.array_equal(full, chainback(3 * L, 0))
    else:
        bits = chainback(L, 0)
        moot = True
    return dict(bits=bits, best_state=best, metrics=old, best_moot=moot, wrapped=wrapped)


def dci_decode(llr, nof_bits, gain_quant=DEFAULT_GAIN_16):
    """srsran_pdcch_dci_decode on the E soft bits of one candidate -> dict(rm, sym, bits[nof_bits + 16], crc_rem, best_state, metrics)"""
    L = nof_bits + 16
    rm = rm_rx(llr, 3 * L)
    sym = quant_f(rm, gain_quant)
    r = decode(sym, L, True)
    p_bits = int(sum(int(b) << (15 - i) for i, b in enumerate(r["bits"][nof_bits:])))
    r.update(rm=rm, sym=sym, crc_rem=p_bits ^ crc16(r["bits"][:nof_bits]))
    return r


def pdcch_mean(llr, ncce, Lagg):
    """the rule of srsran_pdcch_decode_msg (pdcch.c:388-393): a double sum of fabsf in index order, divided by the number of soft bits"""
    e_bits = 72 << Lagg
    mean = 0.0
    for v in np.abs(np.asarray(llr, np.float32)[72 * ncce:72 * ncce + e_bits]):
        mean += float(v)
    return mean / e_bits
