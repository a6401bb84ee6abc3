"""The PRACH occasions at the stream counts D = N_ifft_ul / 128 the record tests/golden/prach_ref.npz does not hold (it runs D = 1, 2, 3 and 16): one handle
configuration per size, three occasions each -- freq_offset 0, the first one whose 839 wanted bins wrap past N_ifft_prach in transform order, and
nof_prb - 6 -- of two preambles of different roots (0 and -6 dB, different delays) plus noise, all seeded and made by tests/prach_model.py alone
(preamble()).  tests/test_prach_sizes.py asserts the generator's margins on the model for them, tools/gen_golden_prach.py --check-sizes holds the model to
the reference on them, tests/test_gpu_prach_sizes.py holds the device to the model."""
import functools

import numpy as np

import prach_model as M

# (nof_prb, standard symbol size) -> D
SIZES = [(25, True), (50, False), (50, True), (75, False), (75, True), (100, False)]
D_OF = {(25, True): 4, (50, False): 6, (50, True): 8, (75, False): 8, (75, True): 12, (100, False): 12}
FIRST_WRAP = {25: 7, 50: 20, 75: 32, 100: 45}
PHASE_FORM = (50, True)  # the size whose handle has freq_domain_offset_calc = 1
# per occasion: two (root, window, delay in samples per D, gain in dB)
TX = [[(0, 2, 30, 0.0), (3, 5, 90, -6.0)], [(1, 0, 110, 0.0), (2, 6, 17, -6.0)], [(3, 1, 64, 0.0), (0, 4, 141, -6.0)]]
NOISE = 0.05


def name(size):
    return "%dprb_%s_D%d" % (size[0], "standard" if size[1] else "default", D_OF[size])


def cfg_of(size):
    """zero_corr_zone 12 (N_cs 119: seven windows a root), four roots searched"""
    return dict(zip(M.CFG_FIELDS, (size[0], 0, 100 + 37 * SIZES.index(size), 12, 4, 0, int(size == PHASE_FORM))))


def freq_offsets(size):
    return [0, FIRST_WRAP[size[0]], size[0] - 6]


@functools.lru_cache(maxsize=None)
def occasions(size):
    """[(freq_offset, signal complex64 [N_ifft_prach], sent indices)] -- computed once, never changed"""
    cfg, n_ul = cfg_of(size), M.symbol_sz(size[0], size[1])
    p = M.plan(cfg, n_ul)
    assert p["N_ifft_prach"] == 1536 * D_OF[size] and p["n_wins"] == 7 and p["num_ra_preambles"] == 4
    rng = np.random.default_rng(8390 + SIZES.index(size))
    out = []
    for fo, tx in zip(freq_offsets(size), TX):
        n = p["N_ifft_prach"]
        sig, rms = np.zeros(n, np.complex128), None
        for root, win, delay, gain in tx:
            x = M.preamble(p, size[0], fo, p["root_u"][root], win * p["N_cs"], delay * D_OF[size])
            rms = rms or float(np.sqrt(np.mean(np.abs(x) ** 2)))
            sig += x * 10.0 ** (gain / 20.0)
        sig += NOISE * rms / np.sqrt(2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        sig = sig.astype(np.complex64)
        sig.setflags(write=False)
        out.append((fo, sig, sorted(root * p["n_wins"] + win for root, win, _, _ in tx)))
    return out


def wraps(p, nof_prb, freq_offset):
    """the wanted bins pass the end of the transform: (begin + N / 2) mod N + 839 > N"""
    n = p["N_ifft_prach"]
    return (M.begin_of(p, nof_prb, freq_offset) + n // 2) % n + M.N_ZC > n
