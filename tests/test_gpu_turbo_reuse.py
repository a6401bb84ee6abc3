"""The two copies of the backward main pass's whole-block loop in the throughput turbo kernel (int16, fixed iterations: turbo_kernels.hip,
tdec_win_unit with 16-step check-points), bit for bit against the oracle.

The loop over the whole-block groups of the backward main pass is emitted twice, one copy behind the other: the first requests its
operands non-temporally, the second with the default cache policy, so that the forward main pass finds the lowest blocks on the die.
WinParams::reuse_blocks (SRSRAN_HIP_TDEC_REUSE_BLOCKS, clamped to the block count nblk) says where the first copy hands over: a group whose
top block is b (b = 3 mod 4, 3 <= b <= nblk - 5) requests blocks b - 3 ... b - 6 and runs in the first copy while b >= reuse_blocks + 6, or
for every b when reuse_blocks is 0.  A cache policy changes no value, so every setting must give the oracle's result; what can go wrong is
the control flow of the second copy: its bounds, the three requests in flight that one copy hands to the other and the last one to the
forward pass, the check-point slots, the bottom group's masked normalisation.

Sizes by the number of whole-block groups (the groups above them take the general body in either case), and what each setting makes of them
(non-temporal copy / default copy, in trips):

    K            nblk  whole groups   0      1      4      8      12     64
    512, 1024    8     1              1/0    0/1    0/1    0/1    0/1    0/1
    768, 1536    12    2              2/0    1/1    0/2    0/2    0/2    0/2
    2304         18    3              3/0    2/1    1/2    0/3    0/3    0/3
    6144         48    11             11/0   10/1   9/2    8/3    7/4    0/11

8 sub-blocks per code block at K <= 800, 16 above.  Inputs and oracle results are those of tests/test_gpu_turbo_edges.py (made once, shared):
nit 1, 2, 3, 8 at -1 dB and 3 dB, 11 blocks, the product entry point (sign bits) and the debug one (int16 rows, decision LLRs compared too).
At -1 dB and nit = 8 the oracle alone must get at least 1 and at most 10 of the 11 blocks wrong: asserted before anything runs on the GPU."""
import numpy as np
import pytest

import oracle_api as O
import test_gpu_turbo_edges as E

pytestmark = pytest.mark.gpu

KNOB = b"SRSRAN_HIP_TDEC_REUSE_BLOCKS"
SPLITS = (0, 1, 4, 8, 12, 64)
SIZES = (512, 1024, 768, 1536, 2304)


def _trips(K, split):
    """(trips of the non-temporal copy, trips of the default-policy copy): the kernel's loop bounds, restated"""
    nb = 16 if K > 800 else 8
    nblk = (K // nb + 7) // 8
    split = min(split, nblk)
    tops = [b for b in range((nblk - 1) | 3, 2, -4) if b <= nblk - 5]
    first = [b for b in tops if b >= (split + 6 if split else 3)]
    return len(first), len(tops) - len(first)


def test_splits_cover_both_copies():
    """Not a check of the kernel: _trips() restates its loop bounds, and this holds the docstring's table to that restatement"""
    table = {512: "1/0 0/1 0/1 0/1 0/1 0/1", 1024: "1/0 0/1 0/1 0/1 0/1 0/1", 768: "2/0 1/1 0/2 0/2 0/2 0/2", 1536: "2/0 1/1 0/2 0/2 0/2 0/2",
             2304: "3/0 2/1 1/2 0/3 0/3 0/3", 6144: "11/0 10/1 9/2 8/3 7/4 0/11"}
    assert set(table) == set(SIZES + (6144,))
    for K, want in table.items():
        assert " ".join("%d/%d" % _trips(K, s) for s in SPLITS) == want, K
    seen = {_trips(K, s) for K in table for s in SPLITS}
    # no trip of either copy, one of each, and the hand-over in mid-pass with more than one trip on either side
    assert {(1, 0), (0, 1), (1, 1), (2, 1), (1, 2)} <= seen


@pytest.fixture(autouse=True)
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0
    assert hiplib.srsran_hip_dev_knob(KNOB, None) == 0


def _set_split(hiplib, split):
    assert hiplib.srsran_hip_dev_knob(KNOB, b"%d" % split) == 0


def _cases(hiplib, K, splits, snrs, nits):
    import srslte_amd as S
    from srslte_amd import capi

    E._precondition(K)
    dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
    for split in splits:
        _set_split(hiplib, split)
        for snr in snrs:
            llr = E._llrs(K, snr)[1]
            for nit in nits:
                ref, ref_dl = E._ref(K, snr, nit)
                what = "K=%d split=%d nit=%d snr=%g" % (K, split, nit, snr)
                out = dec.decode(llr, nit, 0, want_llr=False)
                bad = np.any(out != ref, axis=1).sum()
                assert bad == 0, "%s, sign rows: %d code blocks differ" % (what, bad)
                out, dl = dec.decode(llr, nit, 0, want_llr=True)
                bad = np.any(out != ref, axis=1).sum()
                assert bad == 0, "%s, int16 rows: %d code blocks differ" % (what, bad)
                assert np.array_equal(dl, ref_dl), "%s: decision LLRs differ" % what
    dec.free()


@pytest.mark.parametrize("K", SIZES)
def test_reuse_split(hiplib, K):
    _cases(hiplib, K, SPLITS, E.SNRS, E.NITS)


def test_reuse_split_largest_size(hiplib):
    """K = 6144, the benchmark's size: every setting hands over at another group, the last one before the first whole-block group"""
    _cases(hiplib, 6144, SPLITS, E.SNRS, E.NITS)


def test_reuse_split_unset_is_the_product_default(hiplib):
    """no setting at all: the split the product runs with"""
    assert hiplib.srsran_hip_dev_knob(KNOB, None) == 0
    import srslte_amd as S
    from srslte_amd import capi

    for K in (1536, 6144):
        dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
        out = dec.decode(E._llrs(K, -1.0)[1], 8, 0, want_llr=False)
        assert np.array_equal(out, E._ref(K, -1.0, 8)[0]), K
        dec.free()


@pytest.mark.parametrize("split", (1, 4))
def test_reuse_split_resumed_run(hiplib, split):
    """0...3 followed by 3...8 equals the oracle at 8 (K = 1536: one trip of each copy at split 1, two of the second at 4): the second
    launch starts with decoder 2, from the arrays the first one left"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 1536
    E._precondition(K)
    _set_split(hiplib, split)
    llr = E._llrs(K, -1.0)[1]
    dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
    out, dl = dec.decode(llr, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, E._ref(K, -1.0, 3)[0]) and np.array_equal(dl, E._ref(K, -1.0, 3)[1])
    out, dl = dec.decode(llr, 8, 0, want_llr=True, n_begin=3)
    bad = np.any(out != E._ref(K, -1.0, 8)[0], axis=1).sum()
    assert bad == 0, "K=%d split=%d: %d code blocks differ after 0...3 + 3...8" % (K, split, bad)
    assert np.array_equal(dl, E._ref(K, -1.0, 8)[1]), "K=%d split=%d: decision LLRs differ after 0...3 + 3...8" % (K, split)
    dec.free()


def test_reuse_split_saturated_input(hiplib):
    """three code blocks of nothing but +-32767 with seeded signs, nit 8, K = 1024 with the split at 4: the bottom group's masked normalisation
    in the default-policy copy, every metric at a bound of int16"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 1024
    _set_split(hiplib, 4)
    rng = np.random.default_rng(K + 1)
    llr = ((2 * rng.integers(0, 2, (3, 3 * K + 12)) - 1) * 32767).astype(np.int16)
    ref, ref_dl = O.turbo_decode(llr, 8, K, want_llr=True)
    dec = S.TdecBatch(K, 3, capi.TDEC_AUTO)
    out = dec.decode(llr, 8, 0, want_llr=False)
    assert np.array_equal(out, ref), "saturated input, sign rows: hard bits differ"
    out, dl = dec.decode(llr, 8, 0, want_llr=True)
    assert np.array_equal(out, ref), "saturated input, int16 rows: hard bits differ"
    assert np.array_equal(dl, ref_dl), "saturated input: decision LLRs differ"
    dec.free()
