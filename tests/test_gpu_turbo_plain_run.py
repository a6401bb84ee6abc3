"""The product entry points of the batch turbo decoder (srsran_hip_tdec_batch_run / _run_8bit) on the throughput kernel, bit for bit
against the oracle.

A launch through them completes its run, so its last half iteration files one sign bit per value for the hard decision and no
a-priori array (WinParams::final_run, turbo_kernels.hip); the other turbo tests go through the debug entry point (want_llr), which
keeps the int16 rows.  Failing blocks must match too (-1 dB), for every parity of the last half iteration:
  nit 1: decoder 1 without a-priori, 2: decoder 2, 3: decoder 1 with the fused subtraction, 8: the benchmark's case
and for a lone block as well as 11 blocks (16-bit: the second wave has 3 live and 5 dead lane groups)."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

NITS = (1, 2, 3, 8)
SNRS = (-1.0, 3.0)
N_CB = 11


@pytest.fixture(autouse=True)
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0


@functools.lru_cache(maxsize=None)
def _case(K, snr, sb_layout, in8):
    """LLRs of N_CB blocks and the oracle's hard bits for every nit, made once"""
    import srslte_amd as S

    if in8:
        _, llr = O.turbo_llrs_8bit(K, N_CB, snr, seed=K * 3 + int(snr))
        nb = S.lib().srsran_tdec_autoimp_get_subblocks_8bit(K)
    else:
        _, llr = O.turbo_llrs(K, N_CB, snr, seed=K * 3 + int(snr))
        nb = 16 if (K % 16 == 0 and K > 800) else 8
    src = np.stack([O.natural_to_sb_layout(llr[i], K, nb) for i in range(N_CB)]) if sb_layout else llr
    dec = O.turbo_decode_8bit if in8 else O.turbo_decode
    refs = {nit: dec(src, nit, K, O.ORC_TDEC_AUTO, sb_layout) for nit in NITS}
    src.setflags(write=False)
    for r in refs.values():
        r.setflags(write=False)
    return src, refs


def _check(K, sb_layout=0, in8=False):
    import srslte_amd as S
    from srslte_amd import capi

    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO, llr8=in8)
    for snr in SNRS:
        src, refs = _case(K, snr, sb_layout, in8)
        for nit in NITS:
            for n_cb in (1, N_CB):
                out = dec.decode(src[:n_cb], nit, sb_layout, want_llr=False)
                bad = np.any(out != refs[nit][:n_cb], axis=1).sum()
                assert bad == 0, "K=%d nit=%d snr=%g n_cb=%d: %d code blocks differ" % (K, nit, snr, n_cb, bad)
    dec.free()


@pytest.mark.parametrize("K", [6144, 5824, 816, 1008, 408, 504])
def test_plain_run_16bit(hiplib, K):
    """6144: aligned warm-up, 48 blocks; 5824: sub-blocks of 364 steps, the warm-up starts mid-block and the last block has 4 steps;
    816: the smallest size with 16 sub-blocks, 7 blocks; 1008: ragged 63-step sub-blocks; 408, 504: 8 sub-blocks, 4 lanes per block"""
    _check(K)


def test_plain_run_16bit_subblock_layout(hiplib):
    _check(5824, sb_layout=1)


@pytest.mark.parametrize("K", [6144, 2048])
def test_plain_run_8bit(hiplib, K):
    """6144: 32 sub-blocks, 2048: 16 sub-blocks"""
    _check(K, in8=True)


@pytest.mark.parametrize("K,in8", [(6144, False), (1008, False), (2048, True)])
def test_state_after_a_final_launch(hiplib, K, in8):
    """a plain launch keeps no state to resume from: a ranged call with n_begin > 0 right after it is refused; one from n_begin = 0 on the
    same object equals the oracle; and a run that is not final keeps its state: 0...3 followed by 3...8 equals the oracle at 8"""
    import srslte_amd as S
    from srslte_amd import capi

    src, refs = _case(K, -1.0, 0, in8)
    dec = S.TdecBatch(K, N_CB, capi.TDEC_AUTO, llr8=in8)
    assert np.array_equal(dec.decode(src, 8, 0, want_llr=False), refs[8])
    with pytest.raises(RuntimeError, match=r"\(%d\).*resume" % capi.SRSRAN_ERROR_INVALID_INPUTS):
        dec.decode(src, 8, 0, want_llr=True, n_begin=3)
    out, _ = dec.decode(src, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, refs[3])
    out, _ = dec.decode(src, 8, 0, want_llr=True, n_begin=3)
    assert np.array_equal(out, refs[8])
    assert np.array_equal(dec.decode(src, 2, 0, want_llr=False), refs[2])
    dec.free()
