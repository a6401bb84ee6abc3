"""float64 restatement of the reference's PUSCH channel estimator, srsran_chest_ul_estimate_pusch (lib/src/phy/ch_estimation/chest_ul.c:199-404 with
chest_common.c:51-107, utils/convolution.c:181-218, utils/vector_simd.c:1741-1784 and refsignal_ul.c:209-224), the pattern of csi_model.py: what
tests/test_chest_ul_golden.py holds to the reference's record (tests/golden/chest_ul_ref.npz) and tests/test_gpu_chest_ul.py holds the device to.

With n = 12 L_prb and L(slot) = (slot + 1) cp_nsymb - 4, per slot: rx = symbol L(slot) of the grid at sub-carriers 12 n_prb[slot] + k; ls = rx conj(r);
sm = the 3-tap filter over ls with srsran_conv_same_cf's end rule (the virtual neighbour in front of element 0 is 3 ls[1] - 2 ls[0], the one behind the last
3 ls[n-1] - 2 ls[n-2]), or ls itself with filter_len 0; the slot's row goes to the grant's columns of every symbol of the slot.  The values that the
reference forms in float32 from its sums -- arg(), the rounding of ta_us, the dB conversions -- are formed here in float32 from the float64 sums, so that
ta_us and the NAN / -inf cases compare exactly."""
import numpy as np

F32 = np.float32


def ref_symbol(slot, cp_nsymb):
    return (slot + 1) * cp_nsymb - 4


def rows(grid, r, nof_prb, cp_nsymb, n_prb, L_prb, filt):
    """(rx [2, n] complex128, ls [2, n], sm [2, n]); grid: [2 cp_nsymb * 12 nof_prb] complex64, r: [2 n], filt: None or the three taps"""
    n = 12 * L_prb
    g = np.asarray(grid).reshape(2 * cp_nsymb, 12 * nof_prb)
    rx = np.stack([g[ref_symbol(s, cp_nsymb), 12 * n_prb[s]:12 * n_prb[s] + n] for s in range(2)]).astype(np.complex128)
    ls = rx * np.conj(np.asarray(r).reshape(2, n).astype(np.complex128))
    if filt is None:
        return rx, ls, ls.copy()
    f = np.asarray(filt, F32).astype(np.float64)
    ext = np.concatenate([3 * ls[:, 1:2] - 2 * ls[:, 0:1], ls, 3 * ls[:, -1:] - 2 * ls[:, -2:-1]], axis=1)
    sm = f[0] * ext[:, :-2] + f[1] * ext[:, 1:-1] + f[2] * ext[:, 2:]
    return rx, ls, sm


def sums(rx, ls, sm):
    """the five reductions: (noise power per slot, mean |rx|^2, CFO phasor, time-alignment phasor per slot)"""
    noise = np.mean(np.abs(sm - ls) ** 2, axis=1)
    power = np.mean(np.abs(rx) ** 2)
    cfo = np.sum(ls[0] * np.conj(ls[1]))
    ta = np.sum(ls[:, 1:] * np.conj(ls[:, :-1]), axis=1)
    return noise, power, cfo, ta


def ta_unrounded(ta):
    """mean over the slots of -arg / 2 pi, in micro-seconds (float64: the generator's distance to a rounding boundary)"""
    return float(np.mean(-np.angle(ta) / (2 * np.pi)) / 15e3 * 1e6)


def measurements(noise, power, cfo, ta, filt, meas_ta_en):
    """dict of the six float32 outputs (chest_ul.c:300-326, :211-219, :358-367)"""
    out = {}
    out["cfo_hz"] = F32(F32(np.angle(cfo)) / (F32(2.0) * F32(np.pi) * F32(0.0005)))
    ta_err = F32(0)
    if meas_ta_en:
        for s in range(2):
            ta_err = F32(ta_err + F32(F32(-float(F32(np.angle(ta[s]))) * (1.0 / np.pi) * 0.5) / F32(2)))
    if ta_err != 0 and np.isfinite(ta_err) and abs(ta_err) >= np.finfo(F32).tiny:
        t = F32(F32(ta_err / F32(15e3)) * F32(1e6))
        out["ta_us"] = F32(np.float32(np.floor(abs(t * F32(10.0)) + F32(0.5)) * np.sign(t)) / F32(10.0))  # roundf: halves away from zero
    else:
        out["ta_us"] = F32(0)
    if filt is None:
        ne = F32(0)
    else:
        w = F32(np.asarray(filt, F32)[0])
        a = F32(7.419 * float(w) * float(w) + 0.1117 * float(w) - 0.005387)
        ne = F32(float(np.mean(noise)) / (float(a) * 0.8))
    out["noise_estimate"] = ne
    with np.errstate(divide="ignore", invalid="ignore"):
        normal = np.isfinite(ne) and abs(ne) >= np.finfo(F32).tiny
        out["snr"] = F32(power / float(ne)) if normal else F32(np.nan)
        out["snr_db"] = F32(10.0) * np.log10(out["snr"], dtype=F32)
        out["noise_estimate_dbm"] = F32(F32(10.0) * np.log10(ne, dtype=F32) + F32(30.0))
    return out


def db_values(noise_estimate, snr):
    """the two logarithmic outputs from given float32 linear values, as the host forms them"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(F32(10.0) * np.log10(F32(noise_estimate), dtype=F32) + F32(30.0)), F32(F32(10.0) * np.log10(F32(snr), dtype=F32))


def estimate(grid, r, nof_prb, cp_nsymb, n_prb, L_prb, filt, meas_ta_en, ce=None):
    """(sm rows [2, n] complex128, measurements, ce grid): ce (a flat complex64 grid, or None for zeros) gets the rows in the grant's columns of every symbol
    of each slot and is otherwise untouched"""
    rx, ls, sm = rows(grid, r, nof_prb, cp_nsymb, n_prb, L_prb, filt)
    m = measurements(*sums(rx, ls, sm), filt, meas_ta_en)
    n = 12 * L_prb
    out = (np.zeros(2 * cp_nsymb * 12 * nof_prb, np.complex64) if ce is None else np.array(ce, np.complex64)).reshape(2 * cp_nsymb, 12 * nof_prb)
    for l in range(2 * cp_nsymb):
        s = l // cp_nsymb
        out[l, 12 * n_prb[s]:12 * n_prb[s] + n] = sm[s].astype(np.complex64)
    return sm, m, out.reshape(-1)
