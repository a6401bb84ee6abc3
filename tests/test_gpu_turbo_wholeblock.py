"""The two bodies of the throughput turbo kernel's main passes (int16, fixed iterations: turbo_kernels.hip, tdec_win_unit with 16-step
check-points), bit for bit against the oracle.

Both main passes of a half iteration go over the 8-step blocks in groups of four.  A group whose blocks are all whole, interior ones takes
the whole-block body (straight-line steps, the block's length, its neighbours and its normalisation schedule fixed at compile time); every
other group takes the general body.  The bodies are separate loops: general group(s), the whole-block loop, general group(s).  With nblk
blocks per sub-block (steps = K / sub-blocks, nblk = ceil(steps / 8)):

    backward pass   groups have their top block at b = 3 mod 4, from (nblk - 1) | 3 down; whole-block: 7 <= b <= nblk - 5
    forward pass    groups start at b = 0 mod 4;                                       whole-block: 4 <= b, b + 5 <= nblk

What can go wrong is the hand-over between the loops (which operand set holds which block, the check-point and the requests in flight),
so the sizes are chosen by the number of whole-block groups of each pass and by whether the last block is ragged:

    K     sub-blocks  steps  nblk          whole-block groups, backward / forward
    576   8           72     9             0 / 1
    800   8           100    13  ragged    1 / 2     (the largest size with 8 sub-blocks)
    2048  16          128    16            2 / 2
    2112  16          132    17  ragged    2 / 3
    2304  16          144    18            2 / 3
    2560  16          160    20            3 / 3
    2624  16          164    21  ragged    3 / 4
    3072  16          192    24            4 / 4
    6144  16          384    48            10 / 10   (the benchmark's size)

(tests/test_gpu_turbo_prefetch.py holds 7 to 14 blocks: no whole-block group or one.)

nit 1, 2, 3, 8 (decoder 1 without a-priori, decoder 2, decoder 1 with the fused subtraction, the benchmark's count), one block and 11
(the second wave has dead lane groups), at -1 dB and 3 dB, through the product entry point (want_llr=False: the last half iteration files
sign bits) and through the debug one (want_llr=True: it files int16 rows, and the decision LLRs are compared as well).  At -1 dB and
nit = 8 the oracle itself must get at least one of the 11 blocks wrong and at least one right, so that failing and converged blocks are
both compared; that is asserted on the oracle alone, before anything runs on the GPU.

The 8-bit and the early-stop kernels have one body: they are not run here."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

NITS = (1, 2, 3, 8)
SNRS = (-1.0, 3.0)
N_CB = 11
SIZES_16 = (2048, 2112, 2304, 2560, 2624, 3072)  # 16 sub-blocks: tdec_win_kernel<8, Ar16, false, 16>
SIZES_8 = (576, 800)  # 8 sub-blocks: tdec_win_kernel<4, Ar16, false, 16>


def _groups(K):
    """(nblk, whole-block groups of the backward pass, of the forward pass): the kernel's loop bounds, restated"""
    nb = 16 if K > 800 else 8
    nblk = (K // nb + 7) // 8
    back = sum(1 for b in range((nblk - 1) | 3, -1, -4) if 7 <= b <= nblk - 5)
    fwd = sum(1 for b in range(0, nblk, 4) if b >= 4 and b + 5 <= nblk)
    return nblk, back, fwd


def test_sizes_cover_the_group_counts():
    """Not a check of the kernel: _groups() restates its loop bounds and the sub-block mapping, and this only holds the table of the docstring to
    that restatement -- every count 0, 1, 2 and more in both passes, whole and ragged last blocks.  If the kernel's bounds change, the table and
    the sizes have to be chosen again by hand; the GPU cases below compare with the oracle whatever the bounds are."""
    table = {576: (9, 0, 1), 800: (13, 1, 2), 2048: (16, 2, 2), 2112: (17, 2, 3), 2304: (18, 2, 3), 2560: (20, 3, 3), 2624: (21, 3, 4),
             3072: (24, 4, 4), 6144: (48, 10, 10)}
    for K, want in table.items():
        assert _groups(K) == want, (K, _groups(K), want)
    assert {g[1] for g in table.values()} >= {0, 1, 2, 3} and {g[2] for g in table.values()} >= {1, 2, 3}
    assert _groups(816)[1:] == (0, 0)  # (7 blocks, tests/test_gpu_turbo_prefetch.py: no whole-block group in either pass)


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


@pytest.mark.parametrize("K", SIZES_16 + SIZES_8)
def test_wholeblock_both_bodies(hiplib, K):
    import srslte_amd as S
    from srslte_amd import capi

    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    for snr in SNRS:
        for nit in NITS:
            for n_cb in (1, N_CB):
                _compare(dec, K, snr, nit, n_cb)
    dec.free()


def test_wholeblock_largest_size(hiplib):
    """K = 6144, the benchmark's size: 48 blocks per sub-block, ten whole-block groups between one general group on either side in both passes"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 6144
    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    for snr in SNRS:
        for nit in NITS:
            for n_cb in (1, N_CB):
                _compare(dec, K, snr, nit, n_cb)
    dec.free()


def test_wholeblock_resumed_run(hiplib):
    """0...3 followed by 3...8 equals the oracle at 8 (K = 2112: 17 blocks, the last one ragged, two and three whole-block groups): the second launch
    starts with decoder 2, from the arrays the first one's whole-block and general bodies left"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 2112
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
