"""The throughput turbo kernel with its operand sets rotating over four blocks in both main passes (int16, fixed iterations:
turbo_kernels.hip, tdec_win_unit with 16-step check-points), bit for bit against the oracle.

Both main passes of a half iteration go over the 8-step blocks four at a time, each of the four on its own operand set; block b lives in set
b mod 4.  The backward pass starts at the multiple of four above the last block and ends with block 0 in the set the forward pass starts from;
the forward pass runs past the last block to the next multiple of four, with blocks of no steps.  So what can go wrong depends on the block
count modulo four and on whether the last block is whole.  The sizes cover every count from 7 to 14, whole and ragged last blocks
(steps = K / sub-blocks, nblk = ceil(steps / 8)):

    K     sub-blocks  steps  nblk          K     sub-blocks  steps  nblk
    816   16          51     7   ragged    408   8           51     7   ragged
    960   16          60     8   ragged    512   8           64     8
    1152  16          72     9             576   8           72     9
    1216  16          76     10  ragged    624   8           78     10  ragged
    1344  16          84     11  ragged    688   8           86     11  ragged
    1536  16          96     12            752   8           94     12  ragged
    1600  16          100    13  ragged    800   8           100    13  ragged
    1728  16          108    14  ragged
    6144  16          384    48            (the benchmark's size)

Through the product entry point (want_llr=False: the last half iteration files sign bits), nit 1, 2, 3, 8 (decoder 1 without a-priori,
decoder 2, decoder 1 with the fused subtraction, the benchmark's count), one block and 11 (the second wave has dead lane groups), at
-1 dB and 3 dB.  At -1 dB and nit = 8 the oracle itself must get at least one of the 11 blocks wrong and at least one right, so that
failing and converged blocks are both compared; that is asserted on the oracle alone, before anything runs on the GPU.

The 8-bit and the early-stop kernels keep their backward pass (three sets, copied): they are not run here."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

NITS = (1, 2, 3, 8)
SNRS = (-1.0, 3.0)
N_CB = 11
SIZES_16 = (816, 960, 1152, 1216, 1344, 1536, 1600, 1728)  # 16 sub-blocks: tdec_win_kernel<8, Ar16, false, 16>
SIZES_8 = (408, 512, 576, 624, 688, 752, 800)  # 8 sub-blocks: tdec_win_kernel<4, Ar16, false, 16>


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
    """the oracle's hard bits: made once per case"""
    r = O.turbo_decode(_llrs(K, snr)[1], nit, K)
    r.setflags(write=False)
    return r


def _precondition(K):
    msgs = _llrs(K, -1.0)[0]
    wrong = int(np.any(np.unpackbits(_ref(K, -1.0, 8), axis=1)[:, :K] != msgs, axis=1).sum())
    assert 1 <= wrong <= N_CB - 1, "K=%d: the oracle gets %d of %d blocks wrong at -1 dB, the case compares only one kind" % (K, wrong, N_CB)


@pytest.mark.parametrize("K", SIZES_16 + SIZES_8)
def test_prefetch_plain_run(hiplib, K):
    import srslte_amd as S
    from srslte_amd import capi

    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    for snr in SNRS:
        llr = _llrs(K, snr)[1]
        for nit in NITS:
            ref = _ref(K, snr, nit)
            for n_cb in (1, N_CB):
                out = dec.decode(llr[:n_cb], nit, 0, want_llr=False)
                bad = np.any(out != ref[:n_cb], axis=1).sum()
                assert bad == 0, "K=%d nit=%d snr=%g n_cb=%d: %d code blocks differ" % (K, nit, snr, n_cb, bad)
    dec.free()


def test_prefetch_largest_size(hiplib):
    """K = 6144, the benchmark's size and count: 48 blocks per sub-block, twelve rounds of the four sets"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 6144
    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    out = dec.decode(_llrs(K, -1.0)[1], 8, 0, want_llr=False)
    bad = np.any(out != _ref(K, -1.0, 8), axis=1).sum()
    assert bad == 0, "K=%d: %d code blocks differ" % (K, bad)
    dec.free()


def test_prefetch_resumed_run(hiplib):
    """0...3 followed by 3...8 equals the oracle at 8 (K = 1216: 10 blocks, the last one ragged): every half iteration of either launch takes
    the forward warm-up's operands over through the beta buffer and block 0 in the first operand set"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 1216
    _precondition(K)
    llr = _llrs(K, -1.0)[1]
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    out, _ = dec.decode(llr, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, _ref(K, -1.0, 3))
    out, _ = dec.decode(llr, 8, 0, want_llr=True, n_begin=3)
    bad = np.any(out != _ref(K, -1.0, 8), axis=1).sum()
    assert bad == 0, "K=%d: %d code blocks differ after 0...3 + 3...8" % (K, bad)
    dec.free()
