"""The turn from the backward to the forward main pass in the throughput turbo kernel (int16, fixed iterations: turbo_kernels.hip, tdec_win_unit
with 16-step check-points), bit for bit against the oracle.

The backward main pass ends on block 0 and the forward main pass starts there.  Where the backward pass's bottom group (blocks 3 ... 0) is a
whole-block one -- nblk >= 8 blocks per sub-block -- it is straight-line code behind the whole-block loops, which stop at blocks 7 ... 4: block 3
requests block 0, block 2 keeps its check-point in registers, blocks 1 and 0 have no steps, and nothing is requested for blocks that are not
there.  The forward pass then starts from the raw operands of blocks 0, 1 and 2 where the backward pass left them and from that check-point: it
loads neither slot 2 of the check-point array nor blocks 1 and 2 again, and slots 0 and 2 are never written.  Sub-blocks of 7 blocks or fewer
run their bottom group in the general loop and turn as before.

What can go wrong: which set holds which block when the passes meet (block b lives in set b mod 4), the hand-over of the check-point, the
bounds of the two loop copies and the way into the straight-line group from either of them or from the general loop, the normalisation
schedule at the bottom, and the three forms the operands take (no a-priori array, exchanged rows, three arrays).

Sizes are the smallest at which each way through the turn is taken, on both kernels (steps = K / sub-blocks, nblk = ceil(steps / 8); trips of
the general loop / of the two whole-block loop copies together / the straight-line bottom group):

    K     sub-blocks  steps  nblk          general  whole-block  bottom group
    408   8           51     7   ragged    2        0            general loop: the turn as it was
    816   16          51     7   ragged    2        0            general loop
    512   8           64     8             1        0            straight-line
    960   16          60     8   ragged    1        0            straight-line, entered from the general loop
    1024  16          64     8             1        0            straight-line
    576   8           72     9             2        0            straight-line
    1152  16          72     9             2        0            straight-line
    624   8           78     10  ragged    2        0            straight-line
    1216  16          76     10  ragged    2        0            straight-line
    688   8           86     11  ragged    2        0            straight-line
    1344  16          84     11  ragged    2        0            straight-line
    752   8           94     12  ragged    1        1            straight-line, entered from a whole-block loop
    1536  16          96     12            1        1            straight-line
    6144  16          384    48            1        10           the benchmark's size

Per size: nit 1, 2, 3, 8 (no a-priori array; decoder 2, exchanged rows in q.x; decoder 1 with three arrays; the benchmark's count), one block
and 11 (dead lane groups), at -1 dB and 3 dB, through the product entry point (want_llr=False: sign rows) and the debug one (want_llr=True:
int16 rows, decision LLRs compared too).  Inputs and oracle results are those of tests/test_gpu_turbo_edges.py and
tests/test_gpu_turbo_prefetch.py (same seeds; made once, shared with the former).  At -1 dB and nit = 8 the oracle alone must get at least 1
and at most 10 of the 11 blocks wrong: asserted before anything runs on the GPU.

SRSRAN_HIP_TDEC_REUSE_BLOCKS = 0, 4 and unset at K = 1536 and 6144: the straight-line group is entered from the non-temporal copy of the
whole-block loop, from the default-policy copy, or (the sizes with no whole-block trip, above) straight from the general loop."""
import numpy as np
import pytest

import oracle_api as O
import test_gpu_turbo_edges as E

pytestmark = pytest.mark.gpu

KNOB = b"SRSRAN_HIP_TDEC_REUSE_BLOCKS"
PRODUCT_SPLIT = 20  # turbo::kReuseBlocks, what an unset knob means
SIZES_8 = (408, 512, 576, 624, 688, 752)  # 8 sub-blocks: tdec_win_kernel<4, Ar16, false, 16>
SIZES_16 = (816, 960, 1024, 1152, 1216, 1344, 1536)  # 16 sub-blocks: tdec_win_kernel<8, Ar16, false, 16>


def _turn(K, split=PRODUCT_SPLIT):
    """(nblk, trips of the general loop, of the non-temporal copy, of the default-policy copy, straight-line bottom group): the kernel's
    loop bounds, restated"""
    nb = 16 if K > 800 else 8
    nblk = (K // nb + 7) // 8
    top = nblk - 5
    b = (nblk - 1) | 3
    general = stream = reuse = 0
    while b > top:
        general, b = general + 1, b - 4
    split = min(split, nblk)
    while b >= (split + 6 if split else 7):
        stream, b = stream + 1, b - 4
    while b >= 7:
        reuse, b = reuse + 1, b - 4
    assert b in (3, -1)
    assert (b == 3) == (nblk >= 8)
    return nblk, general, stream, reuse, b == 3


def test_sizes_cover_the_turn():
    """Not a check of the kernel: _turn() restates its loop bounds, and this holds the docstring's table to that restatement"""
    table = {408: (7, 2, 0, False), 816: (7, 2, 0, False), 512: (8, 1, 0, True), 960: (8, 1, 0, True), 1024: (8, 1, 0, True),
             576: (9, 2, 0, True), 1152: (9, 2, 0, True), 624: (10, 2, 0, True), 1216: (10, 2, 0, True), 688: (11, 2, 0, True),
             1344: (11, 2, 0, True), 752: (12, 1, 1, True), 1536: (12, 1, 1, True), 6144: (48, 1, 10, True)}
    assert set(table) == set(SIZES_8 + SIZES_16 + (6144,))
    for K, want in table.items():
        nblk, general, stream, reuse, straight = _turn(K)
        assert (nblk, general, stream + reuse, straight) == want, (K, _turn(K), want)
    # the way into the straight-line group: from the non-temporal copy, from the default-policy copy, with both having run
    assert _turn(1536, 0)[2:4] == (1, 0) and _turn(1536, 4)[2:4] == (0, 1) and _turn(1536)[2:4] == (0, 1)
    assert _turn(6144, 0)[2:4] == (10, 0) and _turn(6144, 4)[2:4] == (9, 1) and _turn(6144)[2:4] == (5, 5)


@pytest.fixture(autouse=True)
def throughput_kernel(hiplib):
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", b"0") == 0
    yield
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TDEC_LAT", None) == 0
    assert hiplib.srsran_hip_dev_knob(KNOB, None) == 0


def _all_cases(K):
    import srslte_amd as S
    from srslte_amd import capi

    E._precondition(K)
    dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
    for snr in E.SNRS:
        for nit in E.NITS:
            for n_cb in (1, E.N_CB):
                E._compare(dec, K, snr, nit, n_cb)
    dec.free()


@pytest.mark.parametrize("K", SIZES_8 + SIZES_16)
def test_turn(hiplib, K):
    _all_cases(K)


def test_turn_largest_size(hiplib):
    """K = 6144, the benchmark's size: ten trips of the whole-block loops, then the straight-line group"""
    _all_cases(6144)


@pytest.mark.parametrize("K", (1536, 6144))
@pytest.mark.parametrize("split", (0, 4, None))
def test_turn_from_either_loop_copy(hiplib, K, split):
    """the straight-line group behind the non-temporal copy (0), behind the default-policy copy (4) and with the product's split (unset)"""
    import srslte_amd as S
    from srslte_amd import capi

    E._precondition(K)
    assert hiplib.srsran_hip_dev_knob(KNOB, None if split is None else b"%d" % split) == 0
    dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
    for snr in E.SNRS:
        for nit in E.NITS:
            E._compare(dec, K, snr, nit, E.N_CB)
    dec.free()


def test_turn_resumed_run(hiplib):
    """0...3 followed by 3...8 equals the oracle at 8 (K = 1024: the straight-line group entered from the general loop): the second launch starts
    with decoder 2, from the arrays the first one left; nothing of a turn lives longer than its half iteration"""
    import srslte_amd as S
    from srslte_amd import capi

    K = 1024
    E._precondition(K)
    llr = E._llrs(K, -1.0)[1]
    dec = S.TdecBatch(K, E.N_CB, capi.TDEC_AUTO)
    out, dl = dec.decode(llr, 3, 0, want_llr=True, n_begin=0)
    assert np.array_equal(out, E._ref(K, -1.0, 3)[0]) and np.array_equal(dl, E._ref(K, -1.0, 3)[1])
    out, dl = dec.decode(llr, 8, 0, want_llr=True, n_begin=3)
    bad = np.any(out != E._ref(K, -1.0, 8)[0], axis=1).sum()
    assert bad == 0, "K=%d: %d code blocks differ after 0...3 + 3...8" % (K, bad)
    assert np.array_equal(dl, E._ref(K, -1.0, 8)[1]), "K=%d: decision LLRs differ after 0...3 + 3...8" % K
    dec.free()


@pytest.mark.parametrize("K", (512, 1024))
def test_turn_saturated_input(hiplib, K):
    """three code blocks of nothing but +-32767 with seeded signs, nit 8: the check-point that stays in registers and the metrics of blocks 3 and 2
    sit at the bounds of int16"""
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
