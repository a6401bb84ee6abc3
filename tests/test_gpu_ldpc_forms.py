"""The LDPC kernel forms that large batches take, held to the oracle bit for bit through the C ABI.

Batches of at most 256 code words are routed to one word per workgroup with its check-to-variable messages in LDS (ldpc_host.cpp:
ldpc_batch_run), so the comparisons of tests/test_gpu_ldpc.py (3 to 24 words) all run that form.  Here the other forms are selected at
small batch sizes with the library's run-time knobs (srsran_hip_dev_knob), and every case asserts through
srsran_hip_ldpc_batch_last_launch that the form it is there for is the one that ran:

    A  packed kernel, messages in global slabs, several words per workgroup, fixed iterations     SRSRAN_HIP_LDPC_C2V_LDS=0
    B  its CRC early-stop form, srsran_hip_ldpc_batch_run_crc and _run_crc_map                    SRSRAN_HIP_LDPC_C2V_LDS=0
    C  plain kernel (float, int16, flooded, odd Z, early stop, per-iteration messages) with a workgroup that decodes several
       shares in a row over its own stale soft words and slab                                      LDPC_SLOTS=2
    D  256 against 257 words, and the benchmark's shape, with no knob set

A and B run twice, on the default grid and with LDPC_SLOTS=2 (fewer workgroups than shares).  Inputs are never noise-free and never the
same word twice: the per-word SNR cycles through values on both sides of the threshold and the clip alternates between 63 and 127.  Every
condition on the input (some words decode and some do not, the iteration counts of an early-stop batch differ inside every workgroup) is
asserted on the oracle alone before anything runs on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu

SNRS = (4.0, 1.5, 0.0, -4.0)  # dB, per word in turn (the recipe of test_gpu_ldpc.py::test_batch_crc_early_stop)
LDPC_KNOBS = (b"SRSRAN_HIP_LDPC_C2V_LDS", b"LDPC_SLOTS", b"LDPC_PACKED", b"LDPC_PCPB")
CRC24B, CRC16 = (0x1800063, 24), (0x11021, 16)


@pytest.fixture
def knob(hiplib):
    """knob(name, value) sets a development knob; every LDPC knob is put back to "unset" afterwards, pass or fail"""
    def set_knob(name, value):
        assert name in LDPC_KNOBS
        assert hiplib.srsran_hip_dev_knob(name, None if value is None else str(value).encode()) == 0

    yield set_knob
    rcs = [hiplib.srsran_hip_dev_knob(name, None) for name in LDPC_KNOBS]
    assert rcs == [0] * len(LDPC_KNOBS)


def _form(dec):
    """what the object's last launch was routed to"""
    import srslte_amd as S
    from srslte_amd import capi

    out = (C.c_int32 * 6)()
    capi.check(S.lib().srsran_hip_ldpc_batch_last_launch(dec._h, C.byref(out)), "ldpc_batch_last_launch")
    f = dict(zip(("packed", "lds", "es", "cpb", "workgroups", "n_cw"), [int(v) for v in out]))
    f["groups"] = -(-f["n_cw"] // f["cpb"])  # shares of cpb words the launch hands out
    return f


def _dims(bg, Z):
    g = O.ldpc_graph(bg, Z)
    return g.bgK, g.bgN, g.bgK * Z, g.bgN * Z


def _short(bg, Z):
    """a rate-matched length that is no multiple of Z and leaves out most rows: fewer edges, hence a slab stride below the allocation's"""
    return (_dims(bg, Z)[0] + 9) * Z + 3


# ---------------------------------------------------------------------------------------------------------------- inputs, made once
@functools.lru_cache(maxsize=None)
def _words(bg, Z, n_cw, crc=None):
    """n_cw different noisy code words: word i at SNRS[i % 4], clipped to 63 or 127 in turn every four words, so that the clip is not tied to the
    SNR.  Drawn with O.ldpc_llrs; with crc = (generator, order) the messages have to end in their checksum, and the same channel is restated here
    around the oracle's encoder.  Returns (messages, int8 LLRs), read-only."""
    g = O.ldpc_graph(bg, Z)
    _, _, liftK, liftN = _dims(bg, Z)
    msgs = np.zeros((n_cw, liftK), np.uint8)
    llrs = np.zeros((n_cw, liftN - 2 * Z), np.int8)
    if not crc:
        for s, snr in enumerate(SNRS):
            for k, clip in enumerate((63, 127)):
                idx = [i for i in range(n_cw) if i % 4 == s and (i // 4) % 2 == k]
                if idx:
                    msgs[idx], llrs[idx] = O.ldpc_llrs(bg, Z, len(idx), snr, seed=1000 * Z + 100 * bg + 2 * s + k, clip=clip)
    else:
        poly, order = crc
        rng = np.random.default_rng([bg, Z, n_cw, order])
        msgs[:] = rng.integers(0, 2, (n_cw, liftK))
        for i in range(n_cw):
            cs = O.orc().orc_crc_bits(poly, order, O.P(msgs[i]), liftK - order)
            msgs[i, liftK - order:] = [(cs >> (order - 1 - j)) & 1 for j in range(order)]
            cw = np.zeros(liftN - 2 * Z, np.uint8)
            assert O.orc().orc_ldpc_encode(C.byref(g), O.P(msgs[i]), O.P(cw)) == 0
            sigma = 10 ** (-SNRS[i % 4] / 20)
            clip = 127 if (i // 4) % 2 else 63
            y = (1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.size)
            llrs[i] = np.clip(np.round(y * 8.0 / sigma ** 2), -clip, clip).astype(np.int8)
    assert len({r.tobytes() for r in llrs}) == n_cw  # never the same word twice
    msgs.setflags(write=False)
    llrs.setflags(write=False)
    return msgs, llrs


def _decode_c(bg, Z, llrs, sf, nit, rm, crc=None, want_soft=False):
    """orc_ldpc_decode_c per word: (messages, return values[, a-posteriori soft bits])"""
    g = O.ldpc_graph(bg, Z)
    _, _, liftK, liftN = _dims(bg, Z)
    llrs = np.ascontiguousarray(llrs, np.int8)
    n = llrs.shape[0]
    out, soft, rets = np.zeros((n, liftK), np.uint8), np.zeros((n, liftN), np.int8), []
    poly, order = crc if crc else (0, 0)
    for i in range(n):
        rets.append(O.orc().orc_ldpc_decode_c(C.byref(g), sf, nit, O.P(llrs[i]), O.P(out[i]), rm, poly, order, O.P(soft[i]) if want_soft else None))
    out.setflags(write=False)
    soft.setflags(write=False)
    return (out, rets, soft) if want_soft else (out, rets)


@functools.lru_cache(maxsize=None)
def _ref_fixed(bg, Z, n_cw, sf, nit, rm, crc=None):
    """the oracle's messages for _words() at a fixed number of iterations, after the check that the input proves something: at least one
    word decodes to its message and at least one does not"""
    msgs, llrs = _words(bg, Z, n_cw, crc)
    ref, rets = _decode_c(bg, Z, llrs, sf, nit, rm)
    assert rets == [nit] * n_cw
    good = int((ref == msgs).all(axis=1).sum())
    assert 0 < good < n_cw, "BG%d Z=%d rm=%d: %d of %d words decode on the oracle" % (bg + 1, Z, rm, good, n_cw)
    return ref


@functools.lru_cache(maxsize=None)
def _ref_crc(bg, Z, n_cw, nit, rm, crc):
    """the oracle's iteration counts and messages with CRC early stop"""
    _, llrs = _words(bg, Z, n_cw, crc)
    ref, rets = _decode_c(bg, Z, llrs, 0.8, nit, rm, crc)
    return ref, tuple(rets)


def _short_es(bg, Z):
    """the shortened length of the early-stop cases (that of test_gpu_ldpc.py::test_batch_crc_early_stop): at _short() the large lifting sizes
    of BG1 decode too few of these words within eight iterations"""
    return (_dims(bg, Z)[0] + 12) * Z


def _assert_counts_mixed(rets, cpb, distinct=3):
    """the batch holds at least three distinct iteration counts, 0 (never matched) and one above 1 among them, and every workgroup's share of
    several words holds words that stop at different iterations (share g is words g * cpb ... of the batch, whoever takes it).
    distinct=2 for the shortened length, where the words of a large lifting size that decode at all do so at the same iteration."""
    assert len(set(rets)) >= distinct and 0 in rets and max(rets) > 1, sorted(set(rets))
    for g0 in range(0, len(rets), cpb):
        share = rets[g0:g0 + cpb]
        assert len(share) == 1 or len(set(share)) >= 2, (g0, share)


# ------------------------------------------------------------------------------ A: packed kernel, global slabs, fixed iterations
# (bg, Z, n_cw, scaling factor, iterations): what each row is there for is in the comment; the words per workgroup are the library's choice
# (choose_cpb) and are asserted as a property, not as a number
ROWS_A = [
    (1, 8, 150, 0.8, 6),    # many words per workgroup, two full shares and a partial one
    (0, 10, 120, 0.8, 5),   # words x Z / 2 lanes one short of a wave: an idle lane behind the last word
    (0, 36, 45, 0.75, 7),   # a few idle lanes; the other scaling factor
    (1, 104, 23, 0.8, 8),   # most of a wave idle
    (0, 128, 18, 0.8, 6),   # words in whole waves
    (1, 208, 11, 0.75, 6),  # two words
    (0, 320, 14, 0.8, 8),   # lifting sizes above 128 choose by SIMD balance
    (0, 352, 13, 0.8, 7),
    (1, 256, 9, 0.8, 6),    # Z / 2 lanes are whole waves: one word per workgroup
    (0, 384, 9, 0.8, 8),
]
ONE_WORD_ROWS = {(1, 256), (0, 384)}


def _run_packed_global(S, knob, bg, Z, llrs, sf, nit, rm, slots):
    knob(b"SRSRAN_HIP_LDPC_C2V_LDS", 0)
    if slots:
        knob(b"LDPC_SLOTS", slots)
    dec = S.LdpcBatch(bg, Z, sf, nit, llrs.shape[0])
    out = dec.decode(llrs, rm)
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["n_cw"]) == (1, 0, 0, llrs.shape[0]), f
    if (bg, Z) in ONE_WORD_ROWS:
        assert f["cpb"] == 1, f
    else:
        assert f["cpb"] > 1 and f["n_cw"] % f["cpb"] != 0, f  # several words per workgroup, the last share partial
    assert f["groups"] >= 3, f
    if slots:
        assert f["workgroups"] == slots < f["groups"], f  # a workgroup decodes several shares in a row
    else:
        assert 1 <= f["workgroups"] <= f["groups"], f
    return out


@pytest.mark.parametrize("slots", [None, 2], ids=["default grid", "2 workgroups"])
@pytest.mark.parametrize("short", [False, True], ids=["full", "shortened"])
@pytest.mark.parametrize("bg,Z,n_cw,sf,nit", ROWS_A, ids=["BG%d-Z%d" % (r[0] + 1, r[1]) for r in ROWS_A])
def test_packed_global_slabs(hiplib, knob, bg, Z, n_cw, sf, nit, short, slots):
    import srslte_amd as S

    rm = _short(bg, Z) if short else _dims(bg, Z)[3] - 2 * Z
    ref = _ref_fixed(bg, Z, n_cw, sf, nit, rm)
    out = _run_packed_global(S, knob, bg, Z, _words(bg, Z, n_cw)[1], sf, nit, rm, slots)
    bad = np.flatnonzero(np.any(ref != out, axis=1))
    assert bad.size == 0, "BG%d Z=%d rm=%d: words %s differ" % (bg + 1, Z, rm, bad.tolist())


@functools.lru_cache(maxsize=None)
def _extreme(bg, Z):
    """the input of test_gpu_ldpc.py::test_extreme_and_full_range_inputs (nothing but the values around the decoder's special cases; the whole
    int8 range; weak LLRs salted with -128) plus one word, so that the last share of a workgroup is partial"""
    rng = np.random.default_rng(5 + Z)
    n = _dims(bg, Z)[3] - 2 * Z
    llrs = np.stack([rng.choice(np.array([-128, -127, -64, -63, 63, 64, 127, 0], np.int8), n) for _ in range(4)] +
                    [rng.integers(-128, 128, n).astype(np.int8) for _ in range(4)] +
                    [np.where(rng.random(n) < 0.1, -128, rng.integers(-30, 31, n)).astype(np.int8) for _ in range(5)])
    llrs.setflags(write=False)
    return llrs, {nit: _decode_c(bg, Z, llrs, 0.8, nit, n)[0] for nit in (1, 3, 10)}


@pytest.mark.parametrize("slots", [None, 2], ids=["default grid", "2 workgroups"])
@pytest.mark.parametrize("bg,Z", [(0, 320), (1, 104)])
def test_packed_global_slabs_extreme_inputs(hiplib, knob, bg, Z, slots):
    import srslte_amd as S

    llrs, want = _extreme(bg, Z)
    for nit in (1, 3, 10):
        got = _run_packed_global(S, knob, bg, Z, llrs, 0.8, nit, llrs.shape[1], slots)
        assert np.array_equal(got, want[nit]), (bg, Z, nit, np.flatnonzero(np.any(got != want[nit], axis=1)).tolist())


# ------------------------------------------------------------------------------ B: the packed kernel's early-stop form
# (bg, Z, n_cw, generators): several words per workgroup (the CRC fold across words) except Z = 320, which early stop keeps at one word
ROWS_B = [
    (1, 8, 150, (CRC16,)),  # liftK = 80: too short for a 24-bit checksum to leave much of a message
    (0, 36, 45, (CRC24B, CRC16)),
    (1, 104, 23, (CRC24B, CRC16)),
    (0, 128, 18, (CRC24B, CRC16)),
    (0, 320, 14, (CRC24B, CRC16)),
]
CASES_B = [(bg, Z, n_cw, crc) for bg, Z, n_cw, crcs in ROWS_B for crc in crcs]
NIT_B = 8


def _run_crc(S, dec, llrs, liftK, rm, crc, use_map):
    """srsran_hip_ldpc_batch_run_crc, or _run_crc_map with code word i in row map[i] of arrays of 2 n_cw rows: (iteration counts, messages by
    code word); with the map, the rows outside it must keep what they held"""
    from srslte_amd import capi

    lib = S.lib()
    n_cw, L = llrs.shape
    d_it = S.DeviceBuffer.from_numpy(np.full(n_cw, -1, np.int32))
    if not use_map:
        d_llr, d_msg = S.DeviceBuffer.from_numpy(llrs), S.DeviceBuffer.from_numpy(np.full((n_cw, liftK), 0xA5, np.uint8))
        capi.check(lib.srsran_hip_ldpc_batch_run_crc(dec._h, d_llr.ptr, L, d_msg.ptr, liftK, n_cw, rm, crc[0], crc[1], d_it.ptr, None), "run_crc")
        capi.check(lib.srsran_hip_stream_sync(None), "sync")
        return d_it.to_numpy(np.int32, (n_cw,)), d_msg.to_numpy(np.uint8, (n_cw, liftK))
    rng = np.random.default_rng(n_cw)
    cw_map = rng.permutation(2 * n_cw)[:n_cw].astype(np.uint32)
    assert np.any(np.diff(cw_map.astype(np.int64)) < 0) and np.any(np.diff(cw_map.astype(np.int64)) > 0)  # not monotonic
    rows = rng.integers(-128, 128, (2 * n_cw, L)).astype(np.int8)  # rows outside the map hold noise: decoding one of them would show
    rows[cw_map] = llrs
    d_llr, d_msg = S.DeviceBuffer.from_numpy(rows), S.DeviceBuffer.from_numpy(np.full((2 * n_cw, liftK), 0xA5, np.uint8))
    d_map = S.DeviceBuffer.from_numpy(cw_map)
    capi.check(lib.srsran_hip_ldpc_batch_run_crc_map(dec._h, d_llr.ptr, L, d_msg.ptr, liftK, d_map.ptr, n_cw, rm, crc[0], crc[1], d_it.ptr, None),
               "run_crc_map")
    capi.check(lib.srsran_hip_stream_sync(None), "sync")
    msg = d_msg.to_numpy(np.uint8, (2 * n_cw, liftK))
    rest = np.setdiff1d(np.arange(2 * n_cw), cw_map)
    assert np.all(msg[rest] == 0xA5), "rows outside the map were written: %s" % rest[np.any(msg[rest] != 0xA5, axis=1)].tolist()
    return d_it.to_numpy(np.int32, (n_cw,)), msg[cw_map]


def _assert_crc_equal(its, msg, ref, rets, what):
    assert its.tolist() == list(rets), (what, [(i, int(a), b) for i, (a, b) in enumerate(zip(its, rets)) if a != b])
    for i, r in enumerate(rets):
        if r > 0:
            assert np.array_equal(msg[i], ref[i]), (what, i)


@pytest.mark.parametrize("slots", [None, 2], ids=["default grid", "2 workgroups"])
@pytest.mark.parametrize("use_map", [False, True], ids=["run_crc", "run_crc_map"])
@pytest.mark.parametrize("bg,Z,n_cw,crc", CASES_B, ids=["BG%d-Z%d-CRC%d" % (c[0] + 1, c[1], c[3][1]) for c in CASES_B])
def test_packed_global_slabs_early_stop(hiplib, knob, bg, Z, n_cw, crc, use_map, slots):
    import srslte_amd as S

    _, _, liftK, liftN = _dims(bg, Z)
    _, llrs = _words(bg, Z, n_cw, crc)
    knob(b"SRSRAN_HIP_LDPC_C2V_LDS", 0)
    if slots:
        knob(b"LDPC_SLOTS", slots)
    dec = S.LdpcBatch(bg, Z, 0.8, NIT_B, n_cw)
    for rm in (liftN - 2 * Z, _short_es(bg, Z)):
        ref, rets = _ref_crc(bg, Z, n_cw, NIT_B, rm, crc)
        its, msg = _run_crc(S, dec, llrs, liftK, rm, crc, use_map)
        f = _form(dec)
        assert (f["packed"], f["lds"], f["es"], f["n_cw"]) == (1, 0, 1, n_cw), f
        if Z > 128:
            assert f["cpb"] == 1, f  # a workgroup lasts as long as its slowest word: large lifting sizes keep one word per workgroup
        else:
            assert f["cpb"] > 1 and n_cw % f["cpb"] != 0, f
        assert f["groups"] >= 3, f
        if slots:
            assert f["workgroups"] == slots < f["groups"], f
        _assert_counts_mixed(rets, f["cpb"], 3 if rm == liftN - 2 * Z else 2)  # (a condition on the input, from the oracle's counts alone)
        _assert_crc_equal(its, msg, ref, rets, (bg, Z, rm, crc[1]))


# ------------------------------------------------------------------------------ C: plain kernel, several shares per workgroup
def _assert_plain_shares(dec, n_cw, es=0):
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["n_cw"]) == (0, 0, es, n_cw), f
    assert f["workgroups"] == 2 < f["groups"], f
    return f


def _fs_llrs(bg, Z, n_cw, kind):
    """float32 / int16 LLRs from the words of _words() (test_gpu_ldpc.py::_fs_llrs: the int16 ones alternately small and large enough to
    reach the 15-bit clip)"""
    l8 = _words(bg, Z, n_cw)[1]
    rng = np.random.default_rng(Z)
    if kind == "f":
        return (l8 * rng.uniform(0.3, 0.35, l8.shape)).astype(np.float32)
    gain = np.where(np.arange(n_cw) % 2, 180, 3)[:, None]
    return (l8.astype(np.int32) * gain).clip(-32767, 32767).astype(np.int16)


@pytest.mark.parametrize("kind", ["f", "s"])
@pytest.mark.parametrize("bg,Z,n_cw", [(1, 30, 27), (0, 96, 7)])
def test_plain_shares_float_and_int16(hiplib, knob, bg, Z, n_cw, kind):
    import srslte_amd as S
    from srslte_amd import capi

    nit = 6
    llrs = _fs_llrs(bg, Z, n_cw, kind)
    msgs = _words(bg, Z, n_cw)[0]
    for rm in (_dims(bg, Z)[3] - 2 * Z, _short(bg, Z)):
        ref, ref_soft = O.ldpc_decode_fs(bg, Z, llrs, 0.8, nit, rm, want_soft=True)
        good = int((ref == msgs).all(axis=1).sum())
        assert 0 < good < n_cw, (bg, Z, rm, good)
        knob(b"LDPC_SLOTS", 2)
        dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw, capi.LDPC_F if kind == "f" else capi.LDPC_S)
        out, soft = dec.decode(llrs, rm, want_soft=True)
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm, np.flatnonzero(np.any(ref != out, axis=1)).tolist())
        assert np.array_equal(ref_soft.view(np.uint8), soft.view(np.uint8)), (bg, Z, rm)
        out = dec.decode(llrs, rm)  # the product entry point: no soft bits out
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm)


@pytest.mark.parametrize("bg,Z,n_cw", [(1, 30, 27), (0, 36, 17)])
def test_plain_shares_flooded(hiplib, knob, bg, Z, n_cw):
    import srslte_amd as S
    from srslte_amd import capi

    nit = 5  # (the flooded schedule runs twice as many)
    msgs, llrs = _words(bg, Z, n_cw)
    for rm in (_dims(bg, Z)[3] - 2 * Z, _short(bg, Z)):
        refs = [O.ldpc_decode_flood(bg, Z, llrs[i], 0.8, nit, rm) for i in range(n_cw)]
        ref, ref_soft = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
        assert [r[2] for r in refs] == [nit] * n_cw
        good = int((ref == msgs).all(axis=1).sum())
        assert 0 < good < n_cw, (bg, Z, rm, good)
        knob(b"LDPC_SLOTS", 2)
        dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw, capi.LDPC_C_FLOOD)
        out, soft = dec.decode(llrs, rm, want_soft=True)
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm, np.flatnonzero(np.any(ref != out, axis=1)).tolist())
        assert np.array_equal(ref_soft, soft), (bg, Z, rm)
        out = dec.decode(llrs, rm)
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm)


@pytest.mark.parametrize("bg,Z,n_cw", [(0, 7, 80), (1, 15, 40)])
def test_plain_shares_int8_odd_lifting_size(hiplib, knob, bg, Z, n_cw):
    """odd lifting sizes: the packed kernel cannot take them"""
    import srslte_amd as S

    nit = 6
    msgs, llrs = _words(bg, Z, n_cw)
    for rm in (_dims(bg, Z)[3] - 2 * Z, _short(bg, Z)):
        ref = _ref_fixed(bg, Z, n_cw, 0.8, nit, rm)
        ref_soft = _decode_c(bg, Z, llrs, 0.8, nit, rm, want_soft=True)[2]
        knob(b"LDPC_SLOTS", 2)
        dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
        out = dec.decode(llrs, rm)
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm, np.flatnonzero(np.any(ref != out, axis=1)).tolist())
        out, soft = dec.decode(llrs, rm, want_soft=True)
        _assert_plain_shares(dec, n_cw)
        assert np.array_equal(ref, out), (bg, Z, rm)
        assert np.array_equal(ref_soft, soft), (bg, Z, rm)


@pytest.mark.parametrize("crc", [CRC24B, CRC16], ids=["CRC24B", "CRC16"])
@pytest.mark.parametrize("bg,Z,n_cw", [(0, 7, 80), (1, 15, 40)])
def test_plain_shares_early_stop_odd_lifting_size(hiplib, knob, bg, Z, n_cw, crc):
    import srslte_amd as S

    _, _, liftK, liftN = _dims(bg, Z)
    _, llrs = _words(bg, Z, n_cw, crc)
    knob(b"LDPC_SLOTS", 2)
    dec = S.LdpcBatch(bg, Z, 0.8, NIT_B, n_cw)
    for rm in (liftN - 2 * Z, _short_es(bg, Z)):
        ref, rets = _ref_crc(bg, Z, n_cw, NIT_B, rm, crc)
        for use_map in (False, True):
            its, msg = _run_crc(S, dec, llrs, liftK, rm, crc, use_map)
            f = _assert_plain_shares(dec, n_cw, es=1)
            assert f["cpb"] > 1, f
            _assert_counts_mixed(rets, f["cpb"])
            _assert_crc_equal(its, msg, ref, rets, (bg, Z, rm, crc[1], use_map))


def test_plain_shares_iteration_messages(hiplib, knob):
    """want_iter_msgs (the one-position-per-lane kernel with the hard decisions of every iteration), BG1 Z = 384: five words on two workgroups"""
    import srslte_amd as S

    bg, Z, n_cw, nit = 0, 384, 5, 6
    _, _, liftK, liftN = _dims(bg, Z)
    _, llrs = _words(bg, Z, n_cw)
    ref = _ref_fixed(bg, Z, n_cw, 0.8, nit, liftN - 2 * Z)
    knob(b"LDPC_SLOTS", 2)
    dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
    out, per_it = dec.decode(llrs, want_iter_msgs=True)
    _assert_plain_shares(dec, n_cw)
    assert np.array_equal(ref, out)
    for k in (1, 3, 6):
        snap = ref if k == nit else _decode_c(bg, Z, llrs, 0.8, k, liftN - 2 * Z)[0]
        assert np.array_equal(np.unpackbits(per_it[:, k - 1], axis=1)[:, :liftK], snap), k


# ------------------------------------------------------------------------------ D: the threshold, no knob set
def test_threshold_256_words(hiplib):
    """256 words take the LDS form, 257 the global slabs: both against the oracle"""
    import srslte_amd as S

    bg, Z, nit = 1, 16, 8
    rm = _dims(bg, Z)[3] - 2 * Z
    _, llrs = _words(bg, Z, 257)
    ref = _ref_fixed(bg, Z, 257, 0.8, nit, rm)
    dec = S.LdpcBatch(bg, Z, 0.8, nit, 257)
    for n_cw, lds in ((256, 1), (257, 0)):
        out = dec.decode(llrs[:n_cw])
        f = _form(dec)
        assert (f["packed"], f["lds"], f["es"], f["n_cw"]) == (1, lds, 0, n_cw), f
        assert (f["cpb"] == 1) if lds else (f["cpb"] > 1), f
        bad = np.flatnonzero(np.any(ref[:n_cw] != out, axis=1))
        assert bad.size == 0, (n_cw, bad.tolist())


@pytest.mark.parametrize("short", [False, True], ids=["full", "shortened"])
def test_many_workgroups_of_many_words(hiplib, short):
    """1,100 words of BG2 Z = 8: more than eight workgroups of 64 words each, one of which takes a second share.  The cases above launch a
    handful of workgroups, and the chip hands neighbouring workgroups to different dies, whose caches do not show each other's stores while
    a kernel runs: two of them on overlapping slabs (a slab base with the wrong stride) would both see their own messages there.  Workgroups
    eight apart share a die; with 64 words per workgroup their slabs overlap when the base leaves out the words per workgroup, or is
    otherwise less than an eighth of what it should be.  (A stride that is short by less stays invisible to a comparison of results.)"""
    import srslte_amd as S

    bg, Z, n_cw, nit = 1, 8, 1100, 6
    rm = _short(bg, Z) if short else _dims(bg, Z)[3] - 2 * Z
    ref = _ref_fixed(bg, Z, n_cw, 0.8, nit, rm)
    dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
    out = dec.decode(_words(bg, Z, n_cw)[1], rm)
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["n_cw"]) == (1, 0, 0, n_cw), f
    assert f["cpb"] > 8 and 8 < f["workgroups"] < f["groups"], f
    bad = np.flatnonzero(np.any(ref != out, axis=1))
    assert bad.size == 0, bad.tolist()


BENCH_SHAPE = (0, 384, 260, 3)  # BG1 Z = 384 as bench.py's LDPC leg runs it, at a batch just over the threshold and few iterations (the oracle's time)


def test_benchmark_shape_fixed_iterations(hiplib):
    import srslte_amd as S

    bg, Z, n_cw, nit = BENCH_SHAPE
    rm = _dims(bg, Z)[3] - 2 * Z
    ref = _ref_fixed(bg, Z, n_cw, 0.8, nit, rm, CRC24B)
    dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
    out = dec.decode(_words(bg, Z, n_cw, CRC24B)[1])
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["cpb"], f["n_cw"]) == (1, 0, 0, 1, n_cw), f
    bad = np.flatnonzero(np.any(ref != out, axis=1))
    assert bad.size == 0, bad.tolist()


def test_benchmark_shape_early_stop(hiplib):
    """the same 260 words through srsran_hip_ldpc_batch_run_crc"""
    import srslte_amd as S

    bg, Z, n_cw, nit = BENCH_SHAPE
    _, _, liftK, liftN = _dims(bg, Z)
    ref, rets = _ref_crc(bg, Z, n_cw, nit, liftN - 2 * Z, CRC24B)
    assert 0 in rets and max(rets) > 1, sorted(set(rets))
    dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
    its, msg = _run_crc(S, dec, _words(bg, Z, n_cw, CRC24B)[1], liftK, liftN - 2 * Z, CRC24B, False)
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["cpb"], f["n_cw"]) == (1, 0, 1, 1, n_cw), f
    _assert_crc_equal(its, msg, ref, rets, "benchmark shape")


# ------------------------------------------------------------------------------ last: nothing stays set
def test_no_ldpc_knob_is_left_set(hiplib):
    """The library has no call that reads a knob back, so this looks at what a knob left behind would change: with none set a batch of five
    words takes the packed kernel (LDPC_PACKED=0 would not) with its messages in LDS (SRSRAN_HIP_LDPC_C2V_LDS=0 would not), one word per
    workgroup, on five workgroups (LDPC_SLOTS=2 would give two)"""
    import srslte_amd as S

    bg, Z, n_cw, nit = 1, 16, 5, 8
    dec = S.LdpcBatch(bg, Z, 0.8, nit, n_cw)
    out = dec.decode(_words(bg, Z, 257)[1][:n_cw])
    f = _form(dec)
    assert (f["packed"], f["lds"], f["es"], f["cpb"], f["workgroups"], f["n_cw"]) == (1, 1, 0, 1, n_cw, n_cw), f
    assert np.array_equal(out, _ref_fixed(bg, Z, 257, 0.8, nit, _dims(bg, Z)[3] - 2 * Z)[:n_cw])
