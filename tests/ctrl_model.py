"""A numpy restatement of the PCFICH and PHICH receivers (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pcfich_table / _phich_ngroups / _phich_table,
srsran_hip_pcfich_decode, srsran_hip_phich_decode_multi): the REs of the two channels (regs_pcfich_init and regs_phich_init, phch/regs.c:249-390, 492-523, as
written -- srslte_amd/csrc/pdcch_map.h states the rules) and srsran_pcfich_decode / srsran_phich_decode (pcfich.c:118-222, phich.c:147-312) in float32 with the
operation order of ctrl_kernel (srslte_amd/csrc/ctrl_kernels.hip): every product, sum and quotient rounded once, every sum in index order from 0.  The
equalisers of two and four ports are the PDCCH model's (tests/pdcch_map_model.py); the one-port one is restated here because the noise estimate is NOT halved."""
import numpy as np

import pdcch_map_model as PM

F32 = np.float32
CFI_TABLE = np.array([[0, 1, 1] * 10 + [0, 1], [1, 0, 1] * 10 + [1, 0], [1, 1, 0] * 10 + [1, 1]], np.uint8)  # TS 36.212 Table 5.3.4-1
W_NORMAL = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1], [1j, 1j, 1j, 1j], [1j, -1j, 1j, -1j], [1j, 1j, -1j, -1j], [1j, -1j, -1j, 1j]])
W_EXT = np.array([[1, 1], [1, -1], [1j, 1j], [1j, -1j]])  # TS 36.211 Table 6.9.1-2


def c_init(sf):
    return (sf["sf_idx"] + 1) * (2 * sf["cell_id"] + 1) * 512 + sf["cell_id"]


# ---- the map
def _regs(sf):
    """the REGs of the control symbols in the reference's order: [l, k0, [k0 .. k3], assigned] (the ordering loop of regs.c:730-755)"""
    nof_prb, vo = sf["cell_nof_prb"], sf["cell_id"] % 3
    max_ctrl = 4 if nof_prb <= 10 else 3
    n = [2, 2 if sf["cell_nof_ports"] == 4 else 3, 3, 3 if sf["cp_nsymb"] == 7 else 2][:max_ctrl]
    regs, j, i, prb, jmax = [], [0] * 4, 0, 0, 0
    while len(regs) < nof_prb * sum(n):
        if n[i] == 3 or (n[i] == 2 and jmax != 1):
            if n[i] == 2:
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
    return regs


def _pcfich_regs(sf, regs):
    nof_prb = sf["cell_nof_prb"]
    k_hat = 6 * (sf["cell_id"] % (2 * nof_prb))
    out = []
    for i in range(4):
        k = (k_hat + (i * nof_prb // 2) * 6) % (nof_prb * 12)
        r = next(r for r in regs if r[0] == 0 and r[1] == k)  # regs_find_reg
        assert not r[3]
        r[3] = True
        out.append(r)
    return out


def pcfich_table(sf):
    """-> the 16 grid indices srsran_regs_pcfich_get reads, in its order (uint32)"""
    return np.array([k for r in _pcfich_regs(sf, _regs(sf)) for k in r[2]], np.uint32)


def phich_units(sf):
    """mapping units: ngroups_phich before the doubling of the extended prefix"""
    if sf["phich_mi"] == 0:
        return 0
    return sf["phich_mi"] * int(np.ceil(F32(PM.NG[sf["phich_resources"]] * F32(F32(sf["cell_nof_prb"]) / F32(8)))))


def phich_ngroups(sf):
    return phich_units(sf) * (2 if sf["cp_nsymb"] == 6 else 1)


def _phich_units_tables(sf):
    regs = _regs(sf)
    _pcfich_regs(sf, regs)
    per = [[r for r in regs if r[0] == l and not r[3]] for l in range(3)]
    c = [len(p) for p in per]
    ext = sf["phich_length"] == 1
    alt = ext and sf["mbsfn_or_sf1_6_tdd"]
    cid, row, out = sf["cell_id"], 12 * sf["cell_nof_prb"], []
    for mi in range(phich_units(sf)):
        idx = []
        for q in range(3):
            li = 0 if not ext else ((mi // 2 + q + 1) % 2 if alt else q)
            ni = ((cid * c[li] // c[1 if alt else 0]) + mi + q * c[li] // 3) % c[li]
            idx += [k + li * row for k in per[li][ni][2]]
        out.append(idx)
    return np.array(out, np.uint32).reshape(-1, 12)


def phich_table(sf, ngroup):
    """-> the 12 grid indices srsran_regs_phich_get reads for the group (uint32)"""
    assert ngroup < phich_ngroups(sf)
    return _phich_units_tables(sf)[ngroup // 2 if sf["cp_nsymb"] == 6 else ngroup]


# ---- the receivers, float32, one rounding per operation
def equalise(y, h, ports, noise_estimate):
    """y[rx][n], h[port][rx][n] (extracted REs) -> the n equalised symbols in the order of d; the noise estimate as it is, added when above 0"""
    if ports != 1:
        return PM.equalise(y, h, ports, noise_estimate)
    y, h = np.asarray(y, np.complex64), np.asarray(h, np.complex64)
    xr = xi = g = None
    for a in range(y.shape[0]):
        pr, pi = PM._cmul_conj(h[0][a], y[a])
        sq = PM._sq(h[0][a])
        xr, xi, g = (pr, pi, sq) if a == 0 else (xr + pr, xi + pi, g + sq)
    if F32(noise_estimate) > 0:
        g = g + F32(noise_estimate)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (xr / g + 1j * (xi / g)).astype(np.complex64)


def _dot(signs, v):
    """sum of +-v[i] in index order from 0, float32 (srsran_vec_dot_prod_fff against a row of +-1)"""
    acc = F32(0)
    for s, x in zip(signs, v):
        acc = F32(acc + x) if s > 0 else F32(acc - x)
    return acc


def _extract(grids, ce, t):
    y = np.array([np.asarray(g, np.complex64).ravel()[t] for g in grids])
    h = np.array([[np.asarray(g, np.complex64).ravel()[t] for g in row] for row in ce])
    return y, h


def pcfich_decode(sf, grids, ce, noise_estimate, table=None):
    """grids[rx], ce[port][rx] -> dict(d, data_f, corr3, cfi, corr)"""
    import oracle_api as O

    y, h = _extract(grids, ce, pcfich_table(sf) if table is None else table)
    d = equalise(y, h, sf["cell_nof_ports"], noise_estimate)
    data_f = np.empty(32, F32)
    data_f[0::2], data_f[1::2] = d.real * F32(-PM.SQRT2), d.imag * F32(-PM.SQRT2)
    c = O.sequence_bits(c_init(sf), 32).astype(bool)
    data_f[c] = -data_f[c]
    corr3 = np.array([_dot(2.0 * CFI_TABLE[k] - 1.0, data_f) for k in range(3)], F32)
    index, max_corr = 0, F32(0)
    for k in range(3):
        if corr3[k] > max_corr:
            index, max_corr = k, corr3[k]
    return dict(d=d, data_f=data_f, corr3=corr3, cfi=index + 1, corr=max_corr)


def phich_decode(sf, grids, ce, noise_estimate, ngroup, nseq, table=None):
    """-> dict(z, bits, ack_value, distance)"""
    import oracle_api as O

    ext = sf["cp_nsymb"] == 6
    assert nseq < (4 if ext else 8)
    y, h = _extract(grids, ce, phich_table(sf, ngroup) if table is None else table)
    d0 = equalise(y, h, sf["cell_nof_ports"], noise_estimate)
    d = np.array([d0[4 * (k // 2) + 2 * (ngroup % 2) + k % 2] for k in range(6)], np.complex64) if ext else d0
    c = O.sequence_bits(c_init(sf), 12).astype(bool)[:d.size]
    d = np.where(c, -d, d).astype(np.complex64)
    nsf, w = (2, W_EXT[nseq]) if ext else (4, W_NORMAL[nseq])
    z, bits = np.zeros(3, np.complex64), np.zeros(3, F32)
    for i in range(3):
        zr, zi = F32(0), F32(0)
        for j in range(nsf):
            s, wr, wi = d[nsf * i + j], F32(w[j].real), F32(w[j].imag)
            tr = F32(F32(wr * s.real) + F32(wi * s.imag))  # conj(w) d
            ti = F32(F32(wr * s.imag) - F32(wi * s.real))
            zr, zi = F32(zr + F32(tr / F32(nsf))), F32(zi + F32(ti / F32(nsf)))
        z[i] = zr + 1j * zi
        bits[i] = F32(np.float64(-F32(zr + zi)) * 0.70710678118654752440)
    ack, distance = ack_decode(bits)
    return dict(z=z, bits=bits, ack_value=ack, distance=distance)


def ack_decode(bits):
    """srsran_phich_ack_decode: max_corr starts at -9999, strict"""
    index, max_corr, distance = 0, F32(-9999), F32(0)
    for i in range(2):
        corr = F32(_dot([1.0 if i else -1.0] * 3, bits) / F32(3))
        if corr > max_corr:
            index, max_corr, distance = i, corr, corr
    return index, distance
