"""The edge groups of the throughput turbo kernel's main passes (int16, fixed iterations: turbo_kernels.hip, tdec_win_unit with 16-step
check-points), bit for bit against the oracle.

Both main passes go over the 8-step blocks of a sub-block in groups of four, and a group takes either the whole-block body (straight-line
steps) or the general one (tests/test_gpu_turbo_wholeblock.py).  The groups at the ends of a pass take the whole-block body too where
their blocks are whole: a normalisation that the end of the sub-block takes out of the schedule is masked there, not branched around.
With nblk blocks per sub-block (steps = K / sub-blocks, nblk = ceil(steps / 8)):

    forward pass    groups start at b = 0 mod 4 and are whole-block while b + wl <= nblk, wl = 4 where steps is a multiple of 32, else 5;
                    masked: the normalisation behind step 0, and in the last group of a sub-block of whole groups the first one of the
                    even block's walk and of the odd block's re-derivation, which start from the sub-block's end
    backward pass   groups have their top block at b = 3 mod 4, from (nblk - 1) | 3 down, and are whole-block for 3 <= b <= nblk - 5 (the
                    groups above hold the four blocks from the beta buffer); in the bottom group the requests run off the array's start,
                    the normalisation behind step 0 is masked and block 0 files a check-point nobody reads in slot 0

The sizes are chosen by which edge groups change body:

    K     sub-blocks  steps  nblk         forward whole / general   backward whole / general
    416   8           52     7   ragged   1 / 1                     0 / 2     smallest: only blocks 0 ... 3 change body
    816   16          51     7   ragged   1 / 1                     0 / 2     the same on the 16-sub-block kernel
    512   8           64     8            2 / 0                     1 / 1     every forward group whole-block; bottom backward group, nblk - 5 = 3
    1024  16          64     8            2 / 0                     1 / 1     the same on the 16-sub-block kernel
    768   8           96     12           3 / 0                     2 / 1     first, interior and last group in one loop
    1536  16          96     12           3 / 0                     2 / 1
    1984  16          124    16  ragged   3 / 1                     3 / 1     nblk a multiple of 4 but the last block ragged: the last group stays general
    2304  16          144    18           4 / 1                     3 / 2     whole blocks, group count not a multiple of 4
    6144  16          384    48           12 / 0                    11 / 1    the benchmark's size

nit 1, 2, 3, 8, one block and 11, at -1 dB and 3 dB, through the product entry point (want_llr=False: sign bits) and the debug one
(want_llr=True: int16 rows, decision LLRs compared as well).  At -1 dB and nit = 8 the oracle itself must get at least 1 and at most 10 of
the 11 blocks wrong; that is asserted on the oracle alone, before anything runs on the GPU.

Saturation: inputs of nothing but +-32767 drive every state metric to the bounds of int16, where the masked normalisation (subtract
o[0] & mask) and the plain one could differ if the helper were wrong."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

NITS = (1, 2, 3, 8)
SNRS = (-1.0, 3.0)
N_CB = 11
SIZES_8 = (416, 512, 768)  # 8 sub-blocks: tdec_win_kernel<4, Ar16, false, 16>
SIZES_16 = (816, 1024, 1536, 1984, 2304)  # 16 sub-blocks: tdec_win_kernel<8, Ar16, false, 16>


def _groups(K):
    """(nblk, forward whole-block / general groups, backward whole-block / general groups): the kernel's loop bounds, restated"""
    nb = 16 if K > 800 else 8
    steps = K // nb
    nblk = (steps + 7) // 8
    wl = 5 if steps % 32 else 4
    fw = 0
    while 4 * fw + wl <= nblk:
        fw += 1
    tops = range((nblk - 1) | 3, -1, -4)
    bw = sum(1 for b in tops if b <= nblk - 5)
    return nblk, fw, (nblk + 3) // 4 - fw, bw, len(tops) - bw


def test_sizes_cover_the_edge_groups():
    """Not a check of the kernel: _groups() restates its loop bounds, and this holds the docstring's table to that restatement"""
    table = {416: (7, 1, 1, 0, 2), 816: (7, 1, 1, 0, 2), 512: (8, 2, 0, 1, 1), 1024: (8, 2, 0, 1, 1), 768: (12, 3, 0, 2, 1),
             1536: (12, 3, 0, 2, 1), 1984: (16, 3, 1, 3, 1), 2304: (18, 4, 1, 3, 2), 6144: (48, 12, 0, 11, 1)}
    assert set(table) == set(SIZES_8 + SIZES_16 + (6144,))
    for K, want in table.items():
        assert _groups(K) == want, (K, _groups(K), want)


@pytest.fixture(autouse=True)
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0


@functools.lru_cache(maxsize=None)
def _llrs(K, snr):
    msgs, llr = O.turbo_llrs(K, N_CB, snr, seed=K * 3 + int(snr))
    llr.setflags(write=False)
    return msgs, llr


@functools.lru_cache(maxsize=None)
def _ref(K, snr, nit):
    """the oracle's hard bits and decision LLRs: made once per case"""
    bits, dl = O.turbo_decode(_llrs(K, snr)[1], nit, K, want_llr=True)
    bits.setflags(write=False)
    dl.setflags(write=False)
    return bits, dl


def _precondition(K):
    msgs = _llrs(K, -1.0)[0]
    wrong = int(np.any(np.unpackbits(_ref(K, -1.0, 8)[0], axis=1)[:, :K] != msgs, axis=1).sum())
    assert 1 <= wrong <= N_CB - 1, "K=%d: the oracle gets %d of %d blocks wrong at -1 dB, the case compares only one kind" % (K, wrong, N_CB)


def _compare(dec, K, snr, nit, n_cb):
    llr = _llrs(K, snr)[1]
    ref, ref_dl = _ref(K, snr, nit)
    what = "K=%d nit=%d snr=%g n_cb=%d" % (K, nit, snr, n_cb)
    out = dec.decode(llr[:n_cb], nit, 0, want_llr=False)
    bad = np.any(out != ref[:n_cb], axis=1).sum()
    assert bad == 0, "%s, sign rows: %d code blocks differ" % (what, bad)
    out, dl = dec.decode(llr[:n_cb], nit, 0, want_llr=True)
    bad = np.any(out != ref[:n_cb], axis=1).sum()
    assert bad == 0, "%s, int16 rows: %d code blocks differ" % (what, bad)
    assert np.array_equal(dl, ref_dl[:n_cb]), "%s: decision LLRs differ" % what


def _all_cases(K):
    import srslte_amd as S
    from srslte_amd import capi

    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    for snr in SNRS:
        for nit in NITS:
            for n_cb in (1, N_CB):
                _compare(dec, K, snr, nit, n_cb)
    dec.free()


@pytest.mark.parametrize("K", SIZES_8 + SIZES_16)
def test_edge_groups(hiplib, K):
    _all_cases(K)


def test_edge_groups_largest_size(hiplib):
    """K = 6144, the benchmark's size: every forward group and all backward groups but the top one take the whole-block body"""
    _all_cases(6144)


def test_edge_groups_resumed_run(hiplib):
    """0...3 followed by 3...8 equals the oracle at 8 (K = 1024: both forward groups and the bottom backward group are whole-block): the
    second launch starts with decoder 2, from the arrays the first one left"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 1024
    _precondition(K)
    llr = _llrs(K, -1.0)[1]
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    out, dl = dec.decode(llr, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, _ref(K, -1.0, 3)[0]) and np.array_equal(dl, _ref(K, -1.0, 3)[1])
    out, dl = dec.decode(llr, 8, 0, want_llr=True, n_begin=3)
    bad = np.any(out != _ref(K, -1.0, 8)[0], axis=1).sum()
    assert bad == 0, "K=%d: %d code blocks differ after 0...3 + 3...8" % (K, bad)
    assert np.array_equal(dl, _ref(K, -1.0, 8)[1]), "K=%d: decision LLRs differ after 0...3 + 3...8" % K
    dec.free()


@pytest.mark.parametrize("K", (512, 1024))
def test_edge_groups_saturated_input(hiplib, K):
    """three code blocks of nothing but +-32767 with seeded signs, nit 8: every metric sits at a bound of int16 when it is normalised"""
    import srslte_amd as S
    from srslte_amd import capi

    rng = np.random.default_rng(K + 1)
    llr = ((2 * rng.integers(0, 2, (3, 3 * K + 12)) - 1) * 32767).astype(np.int16)
    ref, ref_dl = O.turbo_decode(llr, 8, K, want_llr=True)
    dec = S.TdecBatch(K, 3, capi.TDEC_AUTO)
    out = dec.decode(llr, 8, 0, want_llr=False)
    assert np.array_equal(out, ref), "K=%d, saturated input, sign rows: hard bits differ" % K
    out, dl = dec.decode(llr, 8, 0, want_llr=True)
    assert np.array_equal(out, ref), "K=%d, saturated input, int16 rows: hard bits differ" % K
    assert np.array_equal(dl, ref_dl), "K=%d, saturated input: decision LLRs differ" % K
    dec.free()
