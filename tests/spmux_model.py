"""What the spatial-multiplexing / CDD tests share (test_spmux_golden.py on the CPU, test_gpu_spmux.py on the device): the cases the library takes, a
well-conditioned 2x2 channel, the float64 model of the receive and transmit stages in closed form, the bound scale S of every output, and a float32
emulation of the library's fixed operation order (numpy rounds every float32 operation by itself, as the kernels do) from which the constant of the
bound is taken.  No device and no library is needed here."""
import numpy as np

TXSCHEME_SPATIALMUX, TXSCHEME_CDD = 2, 3
ZF, MMSE = 0, 1
EPS = 2.0 ** -24

# (tx_scheme, nof_layers, codebook_idx): everything that is taken
CASES = [(TXSCHEME_CDD, 2, 0), (TXSCHEME_SPATIALMUX, 2, 0), (TXSCHEME_SPATIALMUX, 2, 1), (TXSCHEME_SPATIALMUX, 2, 2),
         (TXSCHEME_SPATIALMUX, 1, 0), (TXSCHEME_SPATIALMUX, 1, 1), (TXSCHEME_SPATIALMUX, 1, 2), (TXSCHEME_SPATIALMUX, 1, 3)]
DECODERS = [(ZF, 0.0), (MMSE, 0.0), (MMSE, 0.05)]
SCALINGS = [1.0, 0.7]

# The constant c of the bound |x - x64| <= c 2^-24 S per component (S: below).  The worst factor of the float32 emulation of the fixed operation order
# against the float64 model over the shapes, cases, decoders and scalings of test_gpu_spmux.py's first test (test_spmux_golden.py measures it on the CPU
# and prints it) was 5.4 (ZF), 9.0 (MMSE) and 4.1 (one layer); c is five times that.  On the MI355X the kernels reach 0.19 ... 0.21 of c in every case
# (profiles/spmux_gputests.log): the emulation's factors, as they must, since test_spmux_golden.py holds the header's source to the emulation bit for bit.  The MMSE chain is the longest (H^H H, its determinant,
# its inverse times H^H, then times y: the conditioning of the channel enters twice), hence its larger constant.
C_BOUND = {"zf": 27.0, "mmse": 45.0, "mrc": 21.0}


def kind_of(layers, dec):
    return "mrc" if layers == 1 else ("mmse" if dec == MMSE else "zf")


def cn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def channel(rng, n):
    """h[port][rx][n]: (port == rx ? 1 : 0.3 e^{j theta}) + 0.1 CN(0,1), theta uniform: every effective channel has a condition number below about 2.5"""
    theta = rng.uniform(0, 2 * np.pi, (2, 2, n))
    base = np.where(np.eye(2, dtype=bool)[:, :, None], 1.0, 0.3 * np.exp(1j * theta))
    return np.ascontiguousarray((base + 0.1 * cn(rng, (2, 2, n))).astype(np.complex64))


def precoder(scheme, layers, cb, n):
    """W[n][port][layer] without its normalisation (TS 36.211 6.3.4.2: tables 6.3.4.2.3-1, 6.3.4.2.2-1 with U D(i))"""
    if layers == 1:
        col = {0: [1, 1], 1: [1, -1], 2: [1, 1j], 3: [1, -1j]}[cb]
        return np.broadcast_to(np.array(col, np.complex128).reshape(1, 2, 1), (n, 2, 1))
    if scheme == TXSCHEME_CDD:
        w = np.empty((n, 2, 2), np.complex128)
        w[0::2] = [[1, 1], [1, -1]]
        w[1::2] = [[1, 1], [-1, 1]]
        return w
    m = {0: [[1, 0], [0, 1]], 1: [[1, 1], [1, -1]], 2: [[1, 1], [1j, -1j]]}[cb]
    return np.broadcast_to(np.array(m, np.complex128), (n, 2, 2))


def norm_of(scheme, layers, cb, scaling):
    s = float(np.float32(scaling))
    return (2.0 if layers == 2 and (scheme == TXSCHEME_CDD or cb > 0) else np.sqrt(2.0)) / s


def model64(y, h, scheme, layers, cb, dec, noise, scaling):
    """the receive stage in float64: x[layer][n], csi[layer][n] (NaN where the reference's scalar body writes nothing), S[layer][n] = norm sum_j |G_kj| |y_j|, the sum
    of the magnitudes of the terms that form x_k = norm sum_j G_kj y_j, G the equaliser matrix"""
    n = y.shape[1]
    H = np.transpose(h.astype(np.complex128), (2, 1, 0)) @ precoder(scheme, layers, cb, n)  # [n][rx][layer]
    Y = y.astype(np.complex128).T[:, :, None]
    nrm = norm_of(scheme, layers, cb, scaling)
    Hh = np.conj(np.transpose(H, (0, 2, 1)))
    if layers == 1:
        g = (np.abs(H) ** 2).sum((1, 2))
        G = Hh / g[:, None, None]
        csi = (g / nrm / np.sqrt(2.0))[None, :]
    elif dec == ZF:
        G = np.linalg.inv(H)
        csi = np.ones((2, n))
        if scheme == TXSCHEME_SPATIALMUX:
            csi[1] = np.nan  # precoding.c:1330-1331 writes csi[i] twice
    else:
        A = Hh @ H + float(np.float32(noise)) * np.eye(2)
        Ai = np.linalg.inv(A)
        G = np.linalg.solve(A, Hh)
        csi = np.stack([1.0 / (nrm * Ai[:, 0, 0].real), 1.0 / (nrm * Ai[:, 1, 1].real)])
    x = nrm * (G @ Y)[:, :, 0].T
    S = nrm * (np.abs(G) @ np.abs(Y))[:, :, 0].T
    return x, csi, S


def precode64(x, scheme, layers, cb, scaling):
    """the transmit stage in float64: y[port][n] = W x times the normalisation (1 / sqrt 2 for one layer and the identity, 1 / 2 else) and the scaling"""
    n = x.shape[1]
    s = float(np.float32(scaling)) * (0.5 if layers == 2 and (scheme == TXSCHEME_CDD or cb > 0) else np.sqrt(0.5))
    return s * (precoder(scheme, layers, cb, n) @ x[:layers].astype(np.complex128).T[:, :, None])[:, :, 0].T


# ---- float32 emulation of the library's operation order (modem_arith.h: mimo_equalise), complex numbers as (re, im) pairs of float32 arrays

def _c(z):
    return np.ascontiguousarray(z.real.astype(np.float32)), np.ascontiguousarray(z.imag.astype(np.float32))


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _conj(a):
    return a[0], -a[1]


def _neg(a):
    return -a[0], -a[1]


def _scale(a, s):
    return a[0] * s, a[1] * s


def _column(a, b, kind):
    if kind == 0:
        return _add(a, b)
    if kind == 1:
        return _sub(a, b)
    if kind == 2:
        return a[0] - b[1], a[1] + b[0]
    return a[0] + b[1], a[1] - b[0]


def _eq32(y0, y1, a0, b0, a1, b1, layers, pre, mmse, norm, noise):
    if layers == 1:
        h0, h1 = _column(a0, b0, pre), _column(a1, b1, pre)
        g = h0[0] * h0[0] + h0[1] * h0[1] + h1[0] * h1[0] + h1[1] * h1[1]
        x = _scale(_add(_mul(_conj(h0), y0), _mul(_conj(h1), y1)), norm / g)
        return [x], [g / norm * np.float32(np.sqrt(0.5))]
    if pre == 0:
        h00, h01, h10, h11 = a0, b0, a1, b1
    else:
        k0, k1 = {1: (0, 1), 2: (2, 3), 3: (1, 0)}[pre]
        h00, h01, h10, h11 = _column(a0, b0, k0), _column(a0, b0, k1), _column(a1, b1, k0), _column(a1, b1, k1)
    if not mmse:
        det = _sub(_mul(h00, h11), _mul(h01, h10))
        q = norm / (det[0] * det[0] + det[1] * det[1])
        d = _scale(_conj(det), q)
        x0 = _mul(_sub(_mul(h11, y0), _mul(h01, y1)), d)
        x1 = _mul(_add(_mul(_neg(h10), y0), _mul(h00, y1)), d)
        one = np.ones_like(x0[0])
        return [x0, x1], [one, one]
    c00, c01, c10, c11 = _conj(h00), _conj(h01), _conj(h10), _conj(h11)
    a00 = _add(_mul(c00, h00), _mul(c10, h10))
    a01 = _add(_mul(c00, h01), _mul(c10, h11))
    a10 = _add(_mul(c01, h00), _mul(c11, h10))
    a11 = _add(_mul(c01, h01), _mul(c11, h11))
    a00 = (a00[0] + noise, a00[1])
    a11 = (a11[0] + noise, a11[1])
    det = _sub(_mul(a00, a11), _mul(a01, a10))
    dn = det[0] * det[0] + det[1] * det[1]
    nr = _scale((det[0] / dn, -det[1] / dn), norm)
    b00, b01, b10, b11 = _mul(a11, nr), _mul(_neg(a01), nr), _mul(_neg(a10), nr), _mul(a00, nr)
    w00, w01 = _add(_mul(b00, c00), _mul(b01, c01)), _add(_mul(b00, c10), _mul(b01, c11))
    w10, w11 = _add(_mul(b10, c00), _mul(b11, c01)), _add(_mul(b10, c10), _mul(b11, c11))
    x0 = _add(_mul(y0, w00), _mul(y1, w01))
    x1 = _add(_mul(y0, w10), _mul(y1, w11))
    return [x0, x1], [np.float32(1) / b00[0], np.float32(1) / b11[0]]


def emulate32(y, h, scheme, layers, cb, dec, noise, scaling):
    """the library's float32 evaluation on the CPU: x[layer][n] complex64, csi[layer][n] float32 (the rows it writes: as model64)"""
    n = y.shape[1]
    s = np.float32(scaling)
    norm = (np.float32(2.0) if layers == 2 and (scheme == TXSCHEME_CDD or cb > 0) else np.float32(np.sqrt(2.0))) / s
    x = np.zeros((layers, n), np.complex64)
    csi = np.full((layers, n), np.nan, np.float32)
    for par in (0, 1):
        sl = slice(par, None, 2)
        if layers == 1:
            pre = cb
        elif scheme == TXSCHEME_CDD:
            pre = 1 if par == 0 else 3
        else:
            pre = cb
        xs, cs = _eq32(_c(y[0][sl]), _c(y[1][sl]), _c(h[0][0][sl]), _c(h[1][0][sl]), _c(h[0][1][sl]), _c(h[1][1][sl]), layers, pre, dec == MMSE, norm, np.float32(noise))
        for k in range(layers):
            x[k][sl] = xs[k][0] + 1j * xs[k][1]
            csi[k][sl] = cs[k]
    if layers == 2 and dec == ZF and scheme == TXSCHEME_SPATIALMUX:
        csi[1] = np.nan
    return x, csi


def precode32(x, scheme, layers, cb, scaling):
    """the transmit stage as the reference's float32 expressions state it: (x0 +- x1) * factor, a multiplication by +-j as a swap and a sign"""
    s = np.float32(scaling)
    x0 = x[0].astype(np.complex64)
    if layers == 1:
        f = np.float32(np.float64(s) * np.sqrt(0.5))
        y0 = (x0.real * f + 1j * (x0.imag * f)).astype(np.complex64)
        y1 = {0: y0, 1: -y0, 2: (-y0.imag + 1j * y0.real).astype(np.complex64), 3: (y0.imag - 1j * y0.real).astype(np.complex64)}[cb]
        return np.stack([y0, y1])
    x1 = x[1].astype(np.complex64)
    if scheme == TXSCHEME_SPATIALMUX and cb == 0:
        f = np.float32(np.float64(s) * np.sqrt(0.5))
        return np.stack([x0.real * f + 1j * (x0.imag * f), x1.real * f + 1j * (x1.imag * f)]).astype(np.complex64)
    f = s / np.float32(2.0)
    su, di = x0 + x1, x0 - x1
    y0 = su.real * f + 1j * (su.imag * f)
    if scheme == TXSCHEME_SPATIALMUX and cb == 2:
        y1 = (-di.imag) * f + 1j * (di.real * f)
    else:
        y1 = di.real * f + 1j * (di.imag * f)
        if scheme == TXSCHEME_CDD:
            y1[1::2] = -y1[1::2]
    return np.stack([y0, y1]).astype(np.complex64)


def worst_factor(x, want, S):
    """max over the components of |x - want| / (2^-24 S)"""
    er, ei = np.abs(x.real - want.real), np.abs(x.imag - want.imag)
    return max(float((er / S).max()), float((ei / S).max())) / EPS
