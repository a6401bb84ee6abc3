"""numpy restatement of the reference's CSI weighting of a PDSCH codeword's soft bits, csi_correction (lib/src/phy/phch/pdsch.c:523-618), in its LV_HAVE_SSE
build (what oracle/Makefile builds and an x86 host runs).  tests/test_csi_golden.py holds it to a record of the reference's own function
(tests/golden/csi_ref.npz, tools/gen_golden_csi.py); tests/test_gpu_pdsch_csi.py holds the library's kernel to it, bit for bit.

    e' = csi_model(e, csi, mod, llr8)        e: nof_re * Qm soft bits (int16, int8 with llr8), csi: nof_re floats, mod: srsran_mod_t (0 BPSK .. 4 256-QAM)

float32 where the reference computes in float, one rounding per operation:
  c_max = the row's largest entry (srsran_vec_max_fi)
  8-bit:                 e' = trunc((float)e * (c[s] / c_max))
  16-bit, vector body:   w = saturate_int16(rint(c[t] * (32767.0f / c_max)))   (_mm_cvtps_pi16: to nearest even), e' = (e * w) >> 16 (_mm_mulhi_pi16: floors)
  16-bit, left over:     e' = trunc((float)e * (c[s] / c_max))                   not halved
The vector body takes 16-QAM and 256-QAM whole and QPSK / 64-QAM in pairs of symbols (a, b); the last symbol of an odd QPSK / 64-QAM codeword and every symbol
of BPSK are left over.  t, the symbol whose weight a bit takes: its own for 16-QAM and 256-QAM; the OTHER symbol of the pair for QPSK (_mm_blend_ps(_csi1,
_csi2, 3)); for the 12 bits of a 64-QAM pair a a a a | b b a a | b b b b.  (One symbol of QPSK / 64-QAM overruns in the reference; here it is left over.)"""
import numpy as np

QM = {0: 1, 1: 2, 2: 4, 3: 6, 4: 8}


def weight_symbol(n, mod):
    """t[s, k]: the symbol whose weight bit k of symbol s takes in the vector body; vec[s]: symbol s is covered by the vector body"""
    qm = QM[mod]
    s = np.arange(n)[:, None] + np.zeros((1, qm), np.int64)
    vec = np.ones(n, bool)
    if mod == 0:
        vec[:] = False
    elif mod == 1:
        vec = (np.arange(n) | 1) < n
        s = s ^ 1
    elif mod == 3:
        vec = (np.arange(n) | 1) < n
        pair = np.array([0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1]).reshape(2, 6)  # bits of a, bits of b
        s = (s & ~1) + pair[np.arange(n) & 1]
    return np.where(vec[:, None], s, np.arange(n)[:, None]).astype(np.int64), vec


def csi_model(e, csi, mod, llr8):
    qm = QM[mod]
    e = np.asarray(e)
    assert e.dtype == (np.int8 if llr8 else np.int16) and e.ndim == 1 and e.size % qm == 0
    n = e.size // qm
    c = np.asarray(csi, np.float32)[:n]
    c_max = c[np.argmax(c)]
    E = e.reshape(n, qm)
    with np.errstate(all="ignore"):
        left = (E.astype(np.float32) * (c / c_max)[:, None]).astype(np.int32)  # float32 quotient, float32 product, truncation toward zero
        if llr8:
            return left.astype(np.int8).reshape(-1)
        t, vec = weight_symbol(n, mod)
        w = np.clip(np.rint(c * (np.float32(32767.0) / c_max)), -32768, 32767).astype(np.int32)
        body = (E.astype(np.int32) * w[t]) >> 16
    return np.where(vec[:, None], body, left).astype(np.int16).reshape(-1)
