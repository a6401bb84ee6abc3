"""A numpy restatement of the PDCCH search's front end (include/srsran_amd/phy_conv_abi.h: srsran_hip_pdcch_sf_t): the REG map of the control region
(srsran_regs_init_opts and what it calls, phch/regs.c:692-781, as written and with its quirks -- srslte_amd/csrc/pdcch_map.h states the rules) and
srsran_pdcch_extract_llr (pdcch.c:424-487) in float32 with the operation order of pdcch_front_kernel (srslte_amd/csrc/pdcch_kernels.hip): every product, sum
and quotient rounded once.  The decode of a candidate is tests/conv_model.py's."""
import numpy as np

import conv_model as CM

F32 = np.float32
FIELDS = ["cell_nof_prb", "cell_nof_ports", "cell_id", "cp_nsymb", "phich_length", "phich_resources", "phich_mi", "mbsfn_or_sf1_6_tdd", "cfi", "sf_idx", "nof_rx"]
PERM = CM.PERM
NG = [F32(1) / F32(6), F32(1) / F32(2), F32(1), F32(2)]


def describe(nof_prb, ports, cell_id, cfi, cp_nsymb=7, phich_length=0, phich_resources=2, phich_mi=1, mbsfn=0, sf_idx=0, nof_rx=1):
    return dict(zip(FIELDS, [nof_prb, ports, cell_id, cp_nsymb, phich_length, phich_resources, phich_mi, mbsfn, cfi, sf_idx, nof_rx]))


def as_row(sf):
    return np.array([sf[f] for f in FIELDS], np.uint32)


def from_row(row):
    return {f: int(v) for f, v in zip(FIELDS, row)}


def nof_ctrl_symbols(sf):
    return sf["cfi"] + (1 if sf["cell_nof_prb"] <= 10 else 0)


def reg_table(sf):
    """-> the 4 nregs grid indices k + l 12 nof_prb in the order srsran_regs_pdcch_get reads them (uint32)"""
    nof_prb, cid = sf["cell_nof_prb"], sf["cell_id"]
    vo, max_ctrl = cid % 3, 4 if nof_prb <= 10 else 3
    n = [2, 2 if sf["cell_nof_ports"] == 4 else 3, 3, 3 if sf["cp_nsymb"] == 7 else 2][:max_ctrl]
    total = nof_prb * sum(n)
    regs = []  # [l, k0, [k0..k3], assigned]
    j, i, prb, jmax = [0] * 4, 0, 0, 0
    while len(regs) < total:
        if n[i] == 3 or (n[i] == 2 and jmax != 1):
            if n[i] == 2:  # six REs less the two at vo and vo + 3, on any port count
                k0 = prb * 12 + j[i] * 6
                k = [k0 + t for t in range(vo)] + [k0 + t + vo + 1 for t in range(2)]
                k += [k0 + vo + 3 + t + 1 for t in range(4 - len(k))]
            else:
                k0 = prb * 12 + j[i] * 4
                k = [k0 + t for t in range(4)]
            regs.append([i, k0, k, False])
            j[i] += 1
        i += 1
        if i == max_ctrl:
            i, jmax = 0, jmax + 1
        if jmax == 3:
            prb, j, jmax = prb + 1, [0] * 4, 0
    # PCFICH
    k_hat = 6 * (cid % (2 * nof_prb))
    for q in range(4):
        kk = (k_hat + (q * nof_prb // 2) * 6) % (nof_prb * 12)
        r = next(r for r in regs if r[0] == 0 and r[1] == kk)
        assert not r[3]
        r[3] = True
    # PHICH
    if sf["phich_mi"] > 0:
        units = sf["phich_mi"] * int(np.ceil(F32(NG[sf["phich_resources"]] * F32(F32(nof_prb) / F32(8)))))
        per = [[r for r in regs if r[0] == l and not r[3]] for l in range(3)]
        c = [len(p) for p in per]
        ext = sf["phich_length"] == 1
        alt = ext and sf["mbsfn_or_sf1_6_tdd"]
        for mi in range(units):
            for q in range(3):
                li = 0 if not ext else ((mi // 2 + q + 1) % 2 if alt else q)
                ni = ((cid * c[li] // c[1 if alt else 0]) + mi + q * c[li] // 3) % c[li]
                per[li][ni][3] = True
    # PDCCH (the reference lays out all three regions whatever the cfi, and divides by each one's REG count)
    assert all(any(r[0] < c + (1 if nof_prb <= 10 else 0) and not r[3] for r in regs) for c in (1, 2, 3)), "the PHICH leaves a region without REGs"
    tmp = [r for r in regs if r[0] < nof_ctrl_symbols(sf) and not r[3]]
    N = len(tmp)
    nrows = (N - 1) // 32 + 1
    ndummy = 32 * nrows - N
    order, k = [None] * N, 0
    for col in range(32):
        for row in range(nrows):
            if row * 32 + PERM[col] >= ndummy:
                kp = (N + k - (cid % N)) % N if k < cid else (k - cid) % N
                order[row * 32 + PERM[col] - ndummy] = tmp[kp]
                k += 1
    nregs = (N // 9) * 9
    return np.array([kk + r[0] * nof_prb * 12 for r in order[:nregs] for kk in r[2]], np.uint32)


# ---- the front end, float32, one rounding per operation
def _cmul_conj(h, y):
    """conj(h) y -> (re, im)"""
    return h.real * y.real + h.imag * y.imag, h.real * y.imag - h.imag * y.real


def _mul_conj(h, y):
    """h conj(y) -> (re, im)"""
    return h.real * y.real + h.imag * y.imag, h.imag * y.real - h.real * y.imag


def _sq(h):
    return h.real * h.real + h.imag * h.imag


SQRT2 = 1.41421356237309504880


def _quot(v, den):
    """x / den * M_SQRT2 as the C expression evaluates it: float quotient, product in double, rounded once to float"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((v / den).astype(np.float64) * SQRT2).astype(F32)


def equalise(y, h, ports, noise_estimate):
    """y[rx][n], h[port][rx][n] complex64 (extracted REs) -> the n equalised symbols in the order of d (complex64)"""
    y, h = np.asarray(y, np.complex64), np.asarray(h, np.complex64)
    nof_rx, n = y.shape
    if ports == 1:
        noise = F32(noise_estimate) / F32(2)
        xr, xi, g = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
        for a in range(nof_rx):
            pr, pi = _cmul_conj(h[0][a], y[a])
            xr, xi, g = (pr if a == 0 else xr + pr), (pi if a == 0 else xi + pi), (_sq(h[0][a]) if a == 0 else g + _sq(h[0][a]))
        if noise > 0:
            g = g + noise
        with np.errstate(divide="ignore", invalid="ignore"):
            return (xr / g + 1j * (xi / g)).astype(np.complex64)
    d = np.zeros(n, np.complex64)
    if ports == 2:
        m = n // 2
        x0r, x0i, x1r, x1i, g = [np.zeros(m, F32) for _ in range(5)]
        for a in range(nof_rx):
            r0, r1 = y[a][0::2], y[a][1::2]
            ha, hb, hc, hd = h[0][a][0::2], h[1][a][1::2], h[1][a][0::2], h[0][a][1::2]
            p0r, p0i = _cmul_conj(ha, r0)
            p1r, p1i = _mul_conj(hb, r1)
            q0r, q0i = _cmul_conj(hd, r1)
            q1r, q1i = _mul_conj(hc, r0)
            x0r, x0i = x0r + (p0r + p1r), x0i + (p0i + p1i)
            x1r, x1i = x1r + (q0r - q1r), x1i + (q0i - q1i)
            g = g + (((ha.real * ha.real + ha.imag * ha.imag) + hb.real * hb.real) + hb.imag * hb.imag)
            g = np.where(g == 0, F32(1e-4), g).astype(F32)
        d[0::2] = _quot(x0r, g) + 1j * _quot(x0i, g)
        d[1::2] = _quot(x1r, g) + 1j * _quot(x1i, g)
        return d
    # four ports, the body without CSI (precoding.c:465-498): ports 0 / 2 at 4i, ports 1 / 3 at 4i + 2, one gain per pair of layers
    m = n // 4
    x = [[np.zeros(m, F32), np.zeros(m, F32)] for _ in range(4)]
    g02, g13 = np.zeros(m, F32), np.zeros(m, F32)
    for a in range(nof_rx):
        h0, h1, h2, h3 = h[0][a][0::4], h[1][a][2::4], h[2][a][0::4], h[3][a][2::4]
        r = [y[a][t::4] for t in range(4)]
        g02 = g02 + (((h0.real * h0.real + h0.imag * h0.imag) + h2.real * h2.real) + h2.imag * h2.imag)
        g13 = g13 + (((h1.real * h1.real + h1.imag * h1.imag) + h3.real * h3.real) + h3.imag * h3.imag)
        for layer, (hp, hq, ra, rb) in enumerate([(h0, h2, r[0], r[1]), (h0, h2, r[0], r[1]), (h1, h3, r[2], r[3]), (h1, h3, r[2], r[3])]):
            if layer % 2 == 0:  # conj(hp) ra + hq conj(rb)
                ar, ai = _cmul_conj(hp, ra)
                br, bi = _mul_conj(hq, rb)
                x[layer][0], x[layer][1] = x[layer][0] + (ar + br), x[layer][1] + (ai + bi)
            else:  # conj(hp) rb - hq conj(ra)
                ar, ai = _cmul_conj(hp, rb)
                br, bi = _mul_conj(hq, ra)
                x[layer][0], x[layer][1] = x[layer][0] + (ar - br), x[layer][1] + (ai - bi)
    for layer in range(4):
        g = g02 if layer < 2 else g13
        d[layer::4] = _quot(x[layer][0], g) + 1j * _quot(x[layer][1], g)
    return d


def soft_bits(d, sf):
    """QPSK soft bits of the equalised symbols (x (float)-sqrt 2), descrambled with c_init = sf_idx 512 + cell_id"""
    import oracle_api as O

    d = np.asarray(d, np.complex64)
    llr = np.empty(2 * d.size, F32)
    k = F32(-SQRT2)
    llr[0::2], llr[1::2] = d.real * k, d.imag * k
    c = O.sequence_bits(sf["sf_idx"] * 512 + sf["cell_id"], llr.size).astype(bool)
    llr[c] = -llr[c]
    return llr


def extract_llr(sf, grids, ce, noise_estimate, table=None):
    """grids[rx], ce[port][rx]: whole grids (1-D or rows x 12 nof_prb) -> dict(sym[rx], ce[port][rx] extracted planes, d, llr)"""
    t = reg_table(sf) if table is None else table
    y = np.array([np.asarray(g, np.complex64).ravel()[t] for g in grids])
    h = np.array([[np.asarray(g, np.complex64).ravel()[t] for g in row] for row in ce])
    d = equalise(y, h, sf["cell_nof_ports"], noise_estimate)
    return dict(sym=y, ce=h, d=d, llr=soft_bits(d, sf))


def search(llr, cands):
    """the mean rule and the decode of every candidate (ncce, L, nof_bits) -> list of dict(mean, decoded, bits, crc_rem)"""
    out = []
    for ncce, L, nof_bits in cands:
        mean = CM.pdcch_mean(llr, ncce, L)
        r = dict(mean=mean, decoded=mean > 0.3, bits=None, crc_rem=0)
        if r["decoded"]:
            m = CM.dci_decode(llr[72 * ncce:72 * ncce + (72 << L)], nof_bits)
            r.update(bits=m["bits"], crc_rem=m["crc_rem"], rm=m["rm"], sym=m["sym"])
        out.append(r)
    return out
