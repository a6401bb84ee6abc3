"""float64 restatement of the reference's downlink channel estimator, srsran_chest_dl_estimate_cfg (lib/src/phy/ch_estimation/chest_dl.c:1004) with
estimate_port, average_pilots, interpolate_pilots, estimate_noise_pilots / _pss / _empty_sc, chest_dl_rssi, chest_estimate_cfo and fill_res, and with
srsran_conv_same_cf (utils/convolution.c:181-218), srsran_interp_linear_offset and srsran_interp_linear_vector{,2} (resampling/interp.c:137-188, :258-284),
the filters of chest_common.c:62-95 and the CRS geometry of refsignal_dl.c:135-267 -- AS WRITTEN, for SRSRAN_SF_NORM subframes with the full CRS pattern.
What tests/test_chest_dl_golden.py holds to the reference's record (tests/golden/chest_dl_ref.npz) and tests/test_gpu_chest_dl.py holds the device to.

Quirks kept: estimate_noise_pilots returns the LAST symbol's power only (sum_power is assigned, not accumulated); get_rsrp walks ports with an antenna
counter; conv_same's virtual elements are (2 + M/2 - i) x[1] - (1 + M/2 - i) x[0] in front and (2 + i - M/2) x[N-1] - (1 + i - M/2) x[N-2] behind; the AVERAGE
path interpolates with offset cell.id % 3 for every port and, with no filter, reads the first 4 nof_prb raw estimates as one row; ports 2 and 3 extrapolate
the symbols behind their second CRS symbol from the FIRST one; time interpolation is a chain of additions; a filter of length 0 (automatic Gauss taps from a
noise estimate of 0) gives a ce of zeros.  The library computes ce whether or not the caller wants it, so the PSS / EMPTY noise estimates do not depend on
that (the reference skips them with a NULL ce).

The values that the reference forms in float32 from its sums (cargf, dB) are formed here in float32 from the float64 sums."""
import numpy as np

F32 = np.float32
ALG_AVERAGE, ALG_INTERPOLATE, ALG_WIENER = 0, 1, 2
NOISE_REFS, NOISE_PSS, NOISE_EMPTY = 0, 1, 2
FILTER_GAUSS, FILTER_TRIANGLE, FILTER_NONE = 0, 1, 2  # srsran_chest_filter_t, chest_common.h:30-34
MAX_TAPS = 9


def nof_symbols(port):
    return 4 if port < 2 else 2


def cs_v(port, l):
    if port == 0:
        return 0 if l % 2 == 0 else 3
    if port == 1:
        return 3 if l % 2 == 0 else 0
    if port == 2:
        return 0 if l == 0 else 3
    return 3 if l == 0 else 0


def fidx(cell_id, l, port):
    return (cs_v(port, l) + cell_id % 6) % 6


def nsymbol(l, cp_nsymb, port):
    if port < 2:
        return (l // 2 + 1) * cp_nsymb - 3 if l % 2 else (l // 2) * cp_nsymb
    return 1 + l * cp_nsymb


def symbol_sz(nof_prb):
    for prb, n in ((6, 128), (15, 256), (25, 384), (50, 768), (75, 1024), (110, 1536)):
        if nof_prb <= prb:
            return n
    raise ValueError(nof_prb)


def taps(filter_type, coef, noise):
    """the smoothing filter as chest_dl.c:702-718 sets it: float32 taps (None: no smoothing; an empty array: filter_len 0)"""
    if filter_type == FILTER_NONE:
        return None
    if filter_type == FILTER_TRIANGLE:
        w = F32(coef[0])
        return np.array([w, F32(1) - F32(2) * w, w], F32)
    order, std = (4, F32(noise) * F32(200.0)) if coef[0] <= 0 else (int(np.uint32(coef[0])), F32(coef[1]))
    n = order + 1
    center = (n - 1) // 2
    with np.errstate(all="ignore"):
        f = np.exp(-np.power(np.arange(n, dtype=np.float64) - center, 2) / (2.0 * float(std) ** 2)).astype(F32)
        norm = F32(np.sum(f.astype(np.float64)))
        if not np.isfinite(norm) or norm == 0 or abs(norm) < np.finfo(F32).tiny:
            return np.zeros(0, F32)
        return (f * (F32(1.0) / norm)).astype(F32)


def conv_same(x, f):
    """srsran_conv_same_cf, convolution.c:181-218"""
    M, N = len(f), len(x)
    f = np.asarray(f, np.float64)
    h = M // 2
    first = np.array([(2 + h - i) * x[1] - (1 + h - i) * x[0] if i < h else x[i - h] for i in range(M + h)], np.complex128)
    last = np.array([(2 + i - h) * x[N - 1] - (1 + i - h) * x[N - 2] if i >= M - 1 else x[N - M + i + 1] for i in range(M + h)], np.complex128)
    out = np.zeros(N, np.complex128)
    j = 0
    for i in range(N):
        if i < h:
            out[i] = np.dot(first[i:i + M], f)
        elif i < N - h:
            out[i] = np.dot(x[i - h:i - h + M], f)
        else:
            out[i] = np.dot(last[j:j + M], f)
            j += 1
    return out


def interp_offset(x, M, off_st, off_end):
    """srsran_interp_linear_offset, interp.c:258-284"""
    L = len(x)
    out = np.zeros(off_st + (L - 1) * M + off_end, np.complex128)
    for j in range(off_st):
        out[off_st - j - 1] = x[0] - (j + 1) * (x[1] - x[0]) / M
    d = (x[1:] - x[:-1]) * (1.0 / M)
    for j in range(M):
        out[off_st + j:off_st + (L - 1) * M:M] = x[:-1] + d * j
    diff = x[L - 1] - x[L - 2]
    for j in range(off_end):
        out[(L - 1) * M + j + off_st] = x[L - 1] + j * diff / M
    return out


def time_schedule(cp_nsymb, port):
    """the calls of interpolate_pilots (chest_dl.c:524-553) as (in0, in1, start, between, d, M): `between` and the M - 1 rows behind it are
    start + k (in1 - in0) / d, k = 1 .. M, each row the one before plus the step"""
    if cp_nsymb == 7:
        if port < 2:
            return [(0, 4, 0, 1, 4, 3), (4, 7, 4, 5, 3, 2), (7, 11, 7, 8, 4, 3), (7, 11, 11, 12, 4, 2)]
        return [(8, 1, 1, 0, 7, 1), (1, 8, 1, 2, 7, 6), (1, 8, 1, 9, 7, 5)]
    if port < 2:
        return [(0, 3, 0, 1, 3, 2), (3, 6, 3, 4, 3, 2), (6, 9, 6, 7, 3, 2), (6, 9, 9, 10, 3, 2)]
    return [(7, 1, 1, 0, 6, 1), (1, 7, 1, 2, 6, 5), (1, 7, 1, 8, 6, 4)]


def noise_pilots(pe, cell_id, port):
    """estimate_noise_pilots, chest_dl.c:325-401; pe: [nsymbols, nref]"""
    nsym, nref = pe.shape
    rows = [None] + [pe[i] for i in range(nsym)] + [None]
    rows[0] = 2.0 * rows[2] - rows[4] if nsym > 3 else rows[2].copy()
    rows[nsym + 1] = 2.0 * rows[nsym - 1] - rows[nsym - 3] if nsym > 3 else rows[nsym - 1].copy()
    sum_power, count = 0.0, 0
    for i in range(1, nsym + 1):
        offset = 0 if ((fidx(cell_id, 0, port) < 3) ^ bool(i & 1)) else 1
        t = rows[i].copy()
        for nb in (rows[i - 1], rows[i + 1]):
            t[offset:] += nb[:nref - offset]
            t[:nref + offset - 1] += nb[1 - offset:]
            if offset:
                t[0] += 2.0 * nb[0] - nb[1]
            else:
                t[nref - 1] += 2.0 * nb[nref - 2] - nb[nref - 1]
        t = rows[i] - t * (1.0 / 5.0)
        sum_power = np.mean(np.abs(t) ** 2)  # assigned, not accumulated
        count += 1
    return sum_power / count * np.sqrt(5.0)


def db(v):
    with np.errstate(all="ignore"):
        return F32(10.0) * np.log10(F32(v))


def estimate(cfg, state, grids, pilots, pss=None):
    """cfg: dict(nof_prb, nof_ports, id, cp_nsymb, nof_rx, sf_idx, estimator_alg, noise_alg, filter_type, filter_coef, rsrp_neighbour, cfo_estimate_enable,
    cfo_estimate_sf_mask); state: dict(noise [4, 4] by [rx][port], cfo); grids: [nof_rx, 2 cp_nsymb * 12 nof_prb]; pilots: the two rows
    csr_refs.pilots[p][sf_idx] (8 and 4 nof_prb points); pss: the 62 points.  Returns dict(ce [port][rx] grids, the per-pair arrays rsrp_pair, rssi_pair,
    rsrp_corr_pair [rx][port], the state out noise_pair and cfo_state, and what fill_res sets)."""
    prb, ports, cid, nsymb, nrx, sf_idx = (cfg[k] for k in ("nof_prb", "nof_ports", "id", "cp_nsymb", "nof_rx", "sf_idx"))
    nre = 12 * prb
    noise = np.array(state["noise"], np.float64).reshape(4, 4).copy()
    cfo = float(state["cfo"])
    rsrp, rssi, corr = np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((4, 4))
    ce = np.zeros((ports, nrx, 2 * nsymb, nre), np.complex128)
    late = sf_idx in (0, 5)
    for rx in range(nrx):
        g = np.asarray(grids[rx]).reshape(2 * nsymb, nre).astype(np.complex128)
        for port in range(ports):
            nsym = nof_symbols(port)
            recv = np.stack([g[nsymbol(l, nsymb, port), fidx(cid, l, port)::6] for l in range(nsym)])
            pe = recv * np.conj(np.asarray(pilots[port // 2]).astype(np.complex128).reshape(nsym, 2 * prb))
            if cfg["rsrp_neighbour"]:
                corr[rx, port] = float(F32(abs(pe.sum() / pe.size))) ** 2
            rsrp[rx, port] = np.mean(np.abs(recv) ** 2)
            rssi[rx, port] = sum(np.sum(np.abs(g[nsymbol(l, nsymb, port)]) ** 2) for l in range(nsym)) / nsym
            if cfg["cfo_estimate_enable"] and ((1 << sf_idx) & cfg["cfo_estimate_sf_mask"]):
                flat = pe.reshape(-1)
                s = np.sum(flat[:4 * prb] * np.conj(flat[4 * prb:8 * prb]))
                n = float(symbol_sz(prb))
                ng = float(int(np.ceil(F32(F32(144.0) * F32(n)) / F32(2048.0))))
                cfo = float(F32(-np.arctan2(F32(s.imag), F32(s.real)) * n / (nsymb * (n + ng)) / 2 / np.pi))
            if cfg["noise_alg"] == NOISE_REFS:
                noise[rx, port] = noise_pilots(pe, cid, port)
            f = taps(cfg["filter_type"], cfg["filter_coef"], noise[rx, port])
            average = cfg["estimator_alg"] == ALG_AVERAGE
            src = pe
            if f is not None:
                if average:
                    a, b = (pe[0::2].sum(axis=0), pe[1::2].sum(axis=0))
                    if fidx(cid, 0, port) >= 3:
                        a, b = b, a
                    row = np.stack([a, b], axis=1).reshape(-1) * (2.0 / nsym)
                    src = (conv_same(row, f) if len(f) else np.zeros_like(row))[None, :]
                else:
                    src = np.stack([conv_same(r, f) if len(f) else np.zeros_like(r) for r in pe])
            c = ce[port, rx]
            if average:
                c[:] = interp_offset(src.reshape(-1)[:4 * prb], 3, cid % 3, 3 - cid % 3)[None, :]
            else:
                for l in range(nsym):
                    c[nsymbol(l, nsymb, port)] = interp_offset(src[l], 6, fidx(cid, l, port), 6 - fidx(cid, l, port))
                for in0, in1, start, between, d, M in time_schedule(nsymb, port):
                    step = (c[in1] - c[in0]) * (1.0 / d)
                    prev = c[start].copy()
                    for k in range(M):
                        prev = prev + step
                        c[between + k] = prev
            if late and cfg["noise_alg"] == NOISE_PSS:
                k = (nsymb - 1) * nre + nre // 2 - 31
                e = c.reshape(-1)[k:k + 62] * np.asarray(pss).astype(np.complex128) - g.reshape(-1)[k:k + 62]
                noise[rx, port] = ports * np.mean(np.abs(e) ** 2) * np.sqrt(0.5)
            elif late and cfg["noise_alg"] == NOISE_EMPTY:
                flat = g.reshape(-1)
                acc = 0.0
                for sym in (nsymb - 2, nsymb - 1):
                    k = sym * nre + nre // 2 - 31
                    acc += np.mean(np.abs(flat[k - 5:k]) ** 2) + np.mean(np.abs(flat[k + 62:k + 67]) ** 2)
                noise[rx, port] = acc
    out = {"ce": ce, "rsrp_pair": rsrp, "rssi_pair": rssi, "rsrp_corr_pair": corr, "noise_pair": noise, "cfo_state": cfo}
    out.update(fill_res(prb, ports, nrx, noise, rsrp, rssi, corr, cfo))
    return out


def fill_res(prb, ports, nrx, noise, rsrp, rssi, corr, cfo):
    """fill_res and its getters, chest_dl.c:868-991, in float32 from the per-pair values"""
    noise, rsrp, rssi, corr = (np.asarray(a, np.float64).astype(F32) for a in (noise, rsrp, rssi, corr))
    with np.errstate(all="ignore"):
        n = F32(0)
        for i in range(nrx):
            n = F32(n + F32(np.sum(noise[i, :ports], dtype=F32) / F32(ports)))
        n = F32(n / F32(nrx))
        rsrp_port = lambda p: F32(np.sum(rsrp[:nrx, p], dtype=F32) / F32(nrx))  # noqa: E731
        r = max([F32(-1e9)] + [rsrp_port(i) for i in range(nrx)])  # (ports walked with the antenna counter)
        neigh = max([F32(-1e9)] + [F32(np.sum(corr[i, :ports], dtype=F32) / F32(ports)) for i in range(nrx)])
        rsrq = F32(sum(F32(F32(prb) * rsrp[i, 0] / rssi[i, 0]) for i in range(nrx)) / F32(nrx))
        rssi_all = F32(sum(F32(F32(4) * rssi[i, 0] / F32(prb) / F32(12)) for i in range(nrx)) / F32(nrx))
        o = {"noise_estimate": n, "noise_estimate_dbm": db(n) + F32(30), "snr_db": db(F32(r / n)), "rsrp": r, "rsrp_dbm": db(r) + F32(30), "rsrp_neigh": neigh,
             "rsrq": rsrq, "rsrq_db": db(rsrq), "rssi_dbm": db(rssi_all) + F32(30), "cfo": F32(cfo), "sync_error": F32(0)}
        z = lambda: np.zeros((4, 4), F32)  # noqa: E731
        o["rsrp_port_dbm"], o["snr_ant_port_db"], o["rsrp_ant_port_dbm"], o["rsrq_ant_port_db"] = np.zeros(4, F32), z(), z(), z()
        for p in range(ports):
            o["rsrp_port_dbm"][p] = db(rsrp_port(p)) + F32(30)
            for a in range(nrx):
                o["snr_ant_port_db"][a, p] = db(F32(rsrp[a, p] / noise[a, p]))
                o["rsrp_ant_port_dbm"][a, p] = db(rsrp[a, p]) + F32(30)
                o["rsrq_ant_port_db"][a, p] = db(F32(F32(prb) * rsrp[a, p] / rssi[a, p]))
    return o


RES_SCALARS = ["noise_estimate", "noise_estimate_dbm", "snr_db", "rsrp", "rsrp_dbm", "rsrp_neigh", "rsrq", "rsrq_db", "rssi_dbm", "cfo", "sync_error"]
RES_ARRAYS = ["rsrp_port_dbm", "snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db"]
PAIR_ARRAYS = ["rsrp_pair", "rssi_pair", "rsrp_corr_pair", "noise_pair"]


# ---- the record (tests/golden/chest_dl_ref.npz, tools/gen_golden_chest_dl.py) and the distances the tests and the generator measure


def unpack(out, st_out):
    """the wrapper's floats by name"""
    d = {k: out[i] for i, k in enumerate(RES_SCALARS)}
    d["rsrp_port_dbm"] = out[11:15]
    for i, k in enumerate(["snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db", "rsrp_pair", "rssi_pair", "rsrp_corr_pair"]):
        d[k] = out[15 + 16 * i:31 + 16 * i].reshape(4, 4)
    d["noise_pair"], d["cfo_state"] = st_out[:16].reshape(4, 4), st_out[16]
    return d


POWER = ["noise_estimate", "rsrp", "rsrp_neigh", "rsrq", "rsrp_pair", "rssi_pair", "rsrp_corr_pair", "noise_pair"]
DB = ["noise_estimate_dbm", "snr_db", "rsrp_dbm", "rsrq_db", "rssi_dbm", "rsrp_port_dbm", "snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db"]


def named(m):
    return {k: m[k] for k in RES_SCALARS + RES_ARRAYS + PAIR_ARRAYS + ["cfo_state"]}


def scalar_distance(got, want):
    """(worst relative distance of the power-like values -- dB values as the power ratio they stand for --, |cfo| distance in Hz, every non-finite value and
    every exact zero where the other side has the same: bool)"""
    worst, same = 0.0, True
    for k in POWER + DB:
        a, b = np.atleast_1d(np.asarray(got[k], np.float64)).reshape(-1), np.atleast_1d(np.asarray(want[k], np.float64)).reshape(-1)
        special = ~np.isfinite(a) | ~np.isfinite(b) | (a == 0) | (b == 0)
        same = same and bool(np.all((a[special] == b[special]) | (np.isnan(a[special]) & np.isnan(b[special]))))
        a, b = a[~special], b[~special]
        if a.size:
            d = np.abs(a - b) * (np.log(10.0) / 10.0) if k in DB else np.abs(a - b) / np.abs(b)
            worst = max(worst, float(d.max()))
    cfo = max(abs(float(got["cfo"]) - float(want["cfo"])), abs(float(got["cfo_state"]) - float(want["cfo_state"])))
    return worst, cfo, same and float(got["sync_error"]) == float(want["sync_error"])


def grid_distance(ce, model_ce):
    top = np.max(np.abs(model_ce))
    return float(np.max(np.abs(ce.astype(np.complex128) - model_ce)) / (top if top > 0 else 1.0))


def case_of(d, i):
    """(cfg, state, grids, pilots, pss) of recorded case i"""
    prb, ports, rx, cp, alg, ft, noise, sf, cid, cfo_en, neigh, _ = [int(v) for v in d["cases"][i]]
    cfg = dict(nof_prb=prb, nof_ports=ports, id=cid, cp_nsymb=cp, nof_rx=rx, sf_idx=sf, estimator_alg=alg, noise_alg=noise, filter_type=ft,
               filter_coef=d["filter_coef"][i], rsrp_neighbour=neigh, cfo_estimate_enable=cfo_en, cfo_estimate_sf_mask=0x3FF if sf != 7 else 0x37F)
    st = d["state_%d" % i]
    return cfg, {"noise": st[:16].reshape(4, 4), "cfo": st[16]}, list(d["grids_%d" % i]), [d["pilots0_%d" % i], d["pilots1_%d" % i]], d["pss_%d" % i]


def recorded_ce(d, i):
    """the reference's ce grids of case i, [port][rx][symbol][sub-carrier] (AVERAGE: row 0 was recorded, with the flag that every row equals it)"""
    cfg = case_of(d, i)[0]
    ce = d["ce_%d" % i]
    if cfg["estimator_alg"] == ALG_AVERAGE:
        assert d["flags_%d" % i][1]
        ce = np.repeat(ce[:, :, None, :], 2 * cfg["cp_nsymb"], axis=2)
    return ce
