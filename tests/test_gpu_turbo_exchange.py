"""The exchange-table entries of the window decoders (turbo_layout.h: xch_pack and its decode helpers), bit for bit against the oracle.

One dword per (trellis step, destination lane of the code block) tells the forward pass where a step's two outputs go: the destination row
and, for each of the lane's two destination sub-blocks, the lane and half that hold the source.  The host builds the tables, every window
kernel decodes them through the same helpers.  What a wrong field width or a wrong decode breaks shows at the edges of the fields and in
the modes that read the entry differently:

  field widths   8 sub-blocks at K = 6144: the largest row index (767), 4 lanes per code block
                 32 sub-blocks (8-bit) at K = 2112, the smallest size that takes them, and at K = 6144: 16 lanes, 4-bit lane indices
  directions     nit = 1, 2, 3, 4: decoder 1 without a-priori values (de-interleaving table), decoder 2 (interleaving table), decoder 1 with the
                 fused subtraction, and an even count, whose decision source is the exchanged output of decoder 2; and nit = 8, the
                 benchmark's count (below: no block of these sizes converges in four half iterations at -1 dB)
  store modes    with decision LLRs (int16 rows filed in the last half iteration) and through the product entry (sign bits), and a run
                 resumed at half iteration 2 after a launch that was not the final one
  lane mappings  K = 408 (8 sub-blocks) and K = 816 (16 sub-blocks), the smallest sizes of each, both with a ragged last block, on the
                 throughput kernel and once on the latency kernel, which decodes the same table

1 and 9 code blocks (9: the second wave of 8-lane code blocks has dead lane groups), the first five at -1 dB, the other four at 3 dB.  At
-1 dB and the largest count of the case (8) the oracle itself must get at least one block wrong and at least one right, so that failing and
converged blocks are both compared: asserted on the oracle alone before anything runs on the GPU.  The seeds are those for which it does
(of seeds 1 ... 12, five blocks each).  The 8-bit decoders cannot meet that: at -1 dB their oracle converges on NO block of K = 2112 or
6144, at any of the seeds 1 ... 12, LLR scales 8 ... 24 and up to 12 half iterations, and on every block at 3 dB.  For them the assertion is
what can hold: every kind is in the batch -- at least one of the -1 dB blocks wrong, at least one of the 3 dB blocks right.

There is no host-only check of the encoding: the suite has no stand-alone path that compiles device headers, so these cases are it."""
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

N_CB = 9
N_LOW = 5  # blocks at -1 dB; the others at 3 dB
NITS = (1, 2, 3, 4, 8)
# (K, 8-bit) -> seed for which the oracle meets the precondition below
SEEDS = {(6144, False): 1, (408, False): 1, (816, False): 2, (2112, True): 1, (6144, True): 1}


@pytest.fixture
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0


@pytest.fixture
def latency_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"1") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0


@functools.lru_cache(maxsize=None)
def _llrs(K, is8):
    gen = O.turbo_llrs_8bit if is8 else O.turbo_llrs
    seed = SEEDS[(K, is8)]
    m0, l0 = gen(K, N_LOW, -1.0, seed=seed)
    m1, l1 = gen(K, N_CB - N_LOW, 3.0, seed=seed + 1000)
    msgs, llr = np.concatenate([m0, m1]), np.concatenate([l0, l1])
    llr.setflags(write=False)
    return msgs, llr


@functools.lru_cache(maxsize=None)
def _ref(K, is8, impl, nit):
    """the oracle's hard bits and decision LLRs: made once per case"""
    dec = O.turbo_decode_8bit if is8 else O.turbo_decode
    out, dl = dec(_llrs(K, is8)[1], nit, K, impl, 0, want_llr=True)
    out.setflags(write=False)
    dl.setflags(write=False)
    return out, dl


def _precondition(K, is8, impl):
    msgs = _llrs(K, is8)[0]
    bad = np.any(np.unpackbits(_ref(K, is8, impl, max(NITS))[0], axis=1)[:, :K] != msgs, axis=1)
    wrong = int(bad[:N_LOW].sum())
    if is8:
        right = int((~bad[N_LOW:]).sum())
        assert wrong >= 1 and right >= 1, "K=%d: %d blocks wrong at -1 dB, %d right at 3 dB: the case compares only one kind" % (K, wrong, right)
    else:
        assert 1 <= wrong <= N_LOW - 1, "K=%d: the oracle gets %d of the %d blocks at -1 dB wrong, the case compares only one kind" % (K, wrong, N_LOW)


def _run(K, is8, impl_g, impl_o, nits=NITS):
    import srslte_amd as S

    _precondition(K, is8, impl_o)
    llr = _llrs(K, is8)[1]
    dec = S.TdecBatch(K, N_CB, impl_g, llr8=is8)
    for nit in nits:
        ref, ref_llr = _ref(K, is8, impl_o, nit)
        for n_cb in (1, N_CB):
            out, out_llr = dec.decode(llr[:n_cb], nit, 0, want_llr=True)
            assert np.array_equal(out, ref[:n_cb]), "K=%d nit=%d n_cb=%d: %d code blocks differ" % (K, nit, n_cb, np.any(out != ref[:n_cb], axis=1).sum())
            assert np.array_equal(out_llr, ref_llr[:n_cb]), "K=%d nit=%d n_cb=%d: decision LLRs differ" % (K, nit, n_cb)
            out = dec.decode(llr[:n_cb], nit, 0, want_llr=False)
            assert np.array_equal(out, ref[:n_cb]), "K=%d nit=%d n_cb=%d: %d code blocks differ (product entry)" % (
                K, nit, n_cb, np.any(out != ref[:n_cb], axis=1).sum())
    # 0...2, not the final launch, then 2...4
    ref, ref_llr = _ref(K, is8, impl_o, 4)
    out, _ = dec.decode(llr, 2, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, _ref(K, is8, impl_o, 2)[0])
    out, out_llr = dec.decode(llr, 4, 0, want_llr=True, n_begin=2)
    assert np.array_equal(out, ref), "K=%d: %d code blocks differ after 0...2 + 2...4" % (K, np.any(out != ref, axis=1).sum())
    assert np.array_equal(out_llr, ref_llr), "K=%d: decision LLRs differ after 0...2 + 2...4" % K
    dec.free()


def test_largest_row_index(hiplib, throughput_kernel):
    """8 sub-blocks, chosen explicitly, at K = 6144: rows up to 767, the widest the row field has to hold; code blocks of 4 lanes"""
    from srslte_amd import capi

    _run(6144, False, capi.TDEC_SSE_WINDOW, O.ORC_TDEC_SSE_WINDOW)


@pytest.mark.parametrize("K", [2112, 6144])
def test_sixteen_lanes_per_code_block(hiplib, throughput_kernel, K):
    """32 sub-blocks (8-bit): lane indices up to 15, the widest the lane fields have to hold; 8-bit row storage"""
    import srslte_amd as S
    from srslte_amd import capi

    assert S.lib().srsran_tdec_autoimp_get_subblocks_8bit(K) == 32
    _run(K, True, capi.TDEC_AUTO, O.ORC_TDEC_AUTO)


@pytest.mark.parametrize("K", [408, 816])
def test_smallest_windows(hiplib, throughput_kernel, K):
    """the smallest size of each lane mapping of the 16-bit decoders: 51 steps per sub-block, seven blocks, the last one ragged"""
    import srslte_amd as S
    from srslte_amd import capi

    assert S.lib().srsran_tdec_autoimp_get_subblocks(K) == (8 if K == 408 else 16)
    _run(K, False, capi.TDEC_AUTO, O.ORC_TDEC_AUTO)


@pytest.mark.parametrize("K", [408, 816])
def test_smallest_windows_latency_kernel(hiplib, latency_kernel, K):
    """the latency kernel decodes the same table (its source lanes are eight apart)"""
    from srslte_amd import capi

    _run(K, False, capi.TDEC_AUTO, O.ORC_TDEC_AUTO)
