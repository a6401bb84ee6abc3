"""The throughput turbo kernel with backward check-points every 16 steps (int16, fixed iterations: turbo_kernels.hip, win_ck_spacing),
bit for bit against the oracle.

The forward main pass takes 8-step blocks in pairs: the odd block of a pair re-derives its backward metrics from the stored check-point,
the even one first walks that check-point back through the odd block's operands.  The sizes are chosen for the pairing, not for the
workload (steps = K / sub-blocks, nblk = ceil(steps / 8)):

    K     sub-blocks  steps  nblk
    816   16          51     7     odd count, the last block (3 steps) alone in its pair
    896   16          56     7     odd count, whole blocks
    1024  16          64     8     even count, whole blocks
    1008  16          63     8     the second block of the last pair has 7 steps
    1056  16          66     9     the last block (2 steps) alone in its pair
    1152  16          72     9     odd count, whole blocks
    408   8           51     7     4 lanes per code block
    512   8           64     8     4 lanes per code block
    576   8           72     9     4 lanes per code block
    5824  16          364    46    even count, the last block has 4 steps

Through the product entry point (want_llr=False: the last half iteration files sign bits), nit 1, 2, 3, 8 (decoder 1 without a-priori,
decoder 2, decoder 1 with the fused subtraction, the benchmark's count), one block and 11 (the second wave has dead lane groups), at
-1 dB and 3 dB.  At -1 dB and nit = 8 the oracle itself must get at least one of the 11 blocks wrong and at least one right, so that
failing and converged blocks are both compared; that is asserted on the oracle alone, before anything runs on the GPU."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

NITS = (1, 2, 3, 8)
SNRS = (-1.0, 3.0)
N_CB = 11
SIZES = (816, 896, 1024, 1008, 1056, 1152, 408, 512, 576, 5824)


@pytest.fixture(autouse=True)
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0


@functools.lru_cache(maxsize=None)
def _case(K, snr):
    """LLRs of N_CB blocks, the oracle's hard bits for every nit and the number of blocks the oracle gets wrong at nit = 8: made once"""
    msgs, llr = O.turbo_llrs(K, N_CB, snr, seed=K * 3 + int(snr))
    refs = {nit: O.turbo_decode(llr, nit, K) for nit in NITS}
    wrong = int(np.any(np.unpackbits(refs[8], axis=1)[:, :K] != msgs, axis=1).sum())
    llr.setflags(write=False)
    for r in refs.values():
        r.setflags(write=False)
    return llr, refs, wrong


def _precondition(K):
    wrong = _case(K, -1.0)[2]
    assert 1 <= wrong <= N_CB - 1, "K=%d: the oracle gets %d of %d blocks wrong at -1 dB, the case compares only one kind" % (K, wrong, N_CB)


@pytest.mark.parametrize("K", SIZES)
def test_ck_spacing_plain_run(hiplib, K):
    import srslte_amd as S
    from srslte_amd import capi

    _precondition(K)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    for snr in SNRS:
        llr, refs, _ = _case(K, snr)
        for nit in NITS:
            for n_cb in (1, N_CB):
                out = dec.decode(llr[:n_cb], nit, 0, want_llr=False)
                bad = np.any(out != refs[nit][:n_cb], axis=1).sum()
                assert bad == 0, "K=%d nit=%d snr=%g n_cb=%d: %d code blocks differ" % (K, nit, snr, n_cb, bad)
    dec.free()


@pytest.mark.parametrize("K", [1008, 6144])
def test_ck_spacing_resumed_run(hiplib, K):
    """0...3 followed by 3...8 equals the oracle at 8: every half iteration hands the forward warm-up's operands over through the beta buffer
    and keeps block 0 in the prefetch registers, and the pair walk starts from there"""
    import srslte_amd as S
    from srslte_amd import capi

    _precondition(K)
    llr, refs, _ = _case(K, -1.0)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO)
    out, _ = dec.decode(llr, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, refs[3])
    out, _ = dec.decode(llr, 8, 0, want_llr=True, n_begin=3)
    bad = np.any(out != refs[8], axis=1).sum()
    assert bad == 0, "K=%d: %d code blocks differ after 0...3 + 3...8" % (K, bad)
    dec.free()
