"""The handle objects behind srsran_hip_*_create / _free and the contexts behind the reference's own structs, on the paths no other test
takes: a handle whose job buffers GROW after its first call and are used again; the CRC lane-multiplier tables past their first capacity
(rows written before a table moves are read after it); the compatibility contexts that re-plan or re-reserve; create, use, free and create
again on one thread.  Every result against the oracle, with the tolerances of the family's own tests."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu
SB = 18600                     # SRSRAN_HIP_SOFTBUFFER_CB_SIZE
NR_SB, NR_DS = 66 * 384, 8448 // 8


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- demodulator
def _demod_case(n_jobs, seed, big=0):
    """n_jobs jobs of mixed modulation / length / alignment (int16 soft bits), the last `big` of them many tiles long: (jobs, symbols, [(offset, llr)])"""
    rng = np.random.default_rng(seed)
    jobs, syms, want = [], [], []
    s_off = l_off = 0
    for i in range(n_jobs):
        mod = int(rng.integers(0, 5)) if i < n_jobs - big else 1
        n = int(rng.choice([1, 7, 144, 1200])) if i < n_jobs - big else 70000  # 35 tiles of 2048 symbols each
        x = O.qam_symbols(mod, n, seed=seed * 100 + i, snr_db=15.0)
        sc_seed = int(rng.integers(0, 1 << 31))
        scr = (1, 1, 2, 3, 0)[i % 5]
        llr = O.demod_soft(mod, x, "s")
        if scr & 2:
            llr = (-llr.astype(np.int32)).astype(np.int16)
        if scr & 1:
            llr = O.sequence_apply(llr, sc_seed)
        pad = int(rng.choice([0, 1, 3, 8]))
        jobs.append((mod, n, s_off, l_off + pad, sc_seed, scr))
        syms.append(x)
        want.append((l_off + pad, llr))
        s_off += n
        l_off += pad + llr.size
    return jobs, np.concatenate(syms), want, l_off


def _demod_run(S, capi, h, case):
    jobs, sym, want, n_llr = case
    d_sym = S.DeviceBuffer.from_numpy(sym)
    d_llr = S.DeviceBuffer.from_numpy(np.zeros(n_llr + 64, np.int16))
    arr = (capi.HipDemodJob * len(jobs))(*[capi.HipDemodJob(*j) for j in jobs])
    capi.check(S.lib().srsran_hip_demod_run(h, d_sym.ptr, d_llr.ptr, capi.LLR_SHORT, arr, len(jobs), None), "demod_run")
    capi.check(S.lib().srsran_hip_stream_sync(None), "sync")
    got = d_llr.to_numpy(np.int16, (n_llr + 64,))
    for (off, llr), j in zip(want, jobs):
        assert _same(got[off:off + llr.size], llr), j
    return got


def test_demod_job_buffers_grow_and_are_used_again(hiplib):
    """1 job, then 40 (past 1 + 1 / 2 + 16 jobs, and more than 1 + 256 tiles), then the first again"""
    import srslte_amd as S
    from srslte_amd import capi

    one, many = _demod_case(1, 1), _demod_case(40, 2, big=8)
    h = C.c_void_p()
    capi.check(hiplib.srsran_hip_demod_create(C.byref(h)), "create")
    first = _demod_run(S, capi, h, one)
    _demod_run(S, capi, h, many)
    assert np.array_equal(_demod_run(S, capi, h, one), first)
    hiplib.srsran_hip_demod_free(h)
    capi.check(hiplib.srsran_hip_demod_create(C.byref(h)), "create again")  # ... and a fresh handle on the same thread
    assert np.array_equal(_demod_run(S, capi, h, one), first)
    hiplib.srsran_hip_demod_free(h)


# ---------------------------------------------------------------------------------------------------------------- NR rate matching
NR_BG, NR_LS, NR_F, NR_MOD = 1, 7, 3, 2
NR_N, NR_K = NR_LS * 50, NR_LS * 10


def _nr_rm_case(n_cb, seed):
    rng = np.random.default_rng(seed)
    msgs = rng.integers(0, 2, (n_cb, NR_K)).astype(np.uint8)
    msgs[:, NR_K - NR_F:] = 254
    full = np.stack([O.ldpc_encode_rm(NR_BG, NR_LS, m, NR_N) for m in msgs])
    Qm = O.QM[NR_MOD]
    Es = [max(Qm, int(NR_N * (0.6 + 0.05 * (i % 9))) // Qm * Qm) for i in range(n_cb)]
    offs = np.concatenate([[0], np.cumsum(Es)]).astype(np.int64)
    tx = [O.ldpc_rm_tx(full[i], Es[i], NR_BG, NR_LS, 0, NR_MOD, NR_N) for i in range(n_cb)]
    x = rng.integers(-60, 61, int(offs[-1])).astype(np.int8)
    rx = np.stack([O.ldpc_rm_rx(x[offs[i]:offs[i + 1]], np.zeros(NR_N, np.int8), NR_F, NR_BG, NR_LS, 0, NR_MOD, NR_N)[0] for i in range(n_cb)])
    return msgs, full, Es, offs, tx, x, rx


def _nr_rm_run(S, capi, h, case):
    """encoder, transmit-side and receive-side rate matching of the case's code blocks on one handle, each against the oracle"""
    lib = S.lib()
    msgs, full, Es, offs, tx, x, rx = case
    n_cb = len(Es)
    d_msg, d_cw = S.DeviceBuffer.from_numpy(msgs), S.DeviceBuffer.from_numpy(np.zeros((n_cb, NR_N), np.uint8))
    enc = (capi.HipLdpcCb * n_cb)(*[capi.HipLdpcCb(i * NR_K, i * NR_N, NR_N) for i in range(n_cb)])
    capi.check(lib.srsran_hip_ldpc_encode_batch(h, d_msg.ptr, d_cw.ptr, enc, n_cb, NR_BG, NR_LS, None), "encode")
    d_tx = S.DeviceBuffer.from_numpy(np.zeros(int(offs[-1]), np.uint8))
    cb_tx = (capi.HipLdpcCb * n_cb)(*[capi.HipLdpcCb(i * NR_N, int(offs[i]), Es[i]) for i in range(n_cb)])
    capi.check(lib.srsran_hip_ldpc_rm_tx_batch(h, d_cw.ptr, d_tx.ptr, cb_tx, n_cb, NR_BG, NR_LS, 0, NR_MOD, NR_N, None), "rm_tx")
    d_x, d_soft = S.DeviceBuffer.from_numpy(x), S.DeviceBuffer.from_numpy(np.zeros((n_cb, NR_N), np.int8))
    cb_rx = (capi.HipLdpcCb * n_cb)(*[capi.HipLdpcCb(int(offs[i]), i * NR_N, Es[i]) for i in range(n_cb)])
    capi.check(lib.srsran_hip_ldpc_rm_rx_batch(h, capi.LLR_BYTE, d_x.ptr, d_soft.ptr, cb_rx, n_cb, NR_F, NR_BG, NR_LS, 0, NR_MOD, NR_N, None), "rm_rx")
    capi.check(lib.srsran_hip_stream_sync(None), "sync")
    got = d_cw.to_numpy(np.uint8, (n_cb, NR_N)), d_tx.to_numpy(np.uint8, (int(offs[-1]),)), d_soft.to_numpy(np.int8, (n_cb, NR_N))
    assert np.array_equal(got[0], full)
    for i in range(n_cb):
        assert np.array_equal(got[1][offs[i]:offs[i + 1]], tx[i]), i
    assert np.array_equal(got[2], rx)
    return got


def test_nr_rate_matching_job_buffer_grows_and_is_used_again(hiplib):
    """one code block, then 40 (past 1 + 1 / 2 + 16), then the first again: LDPC encoder and rate matching in both directions"""
    import srslte_amd as S
    from srslte_amd import capi

    one, many = _nr_rm_case(1, 5), _nr_rm_case(40, 6)
    h = C.c_void_p()
    capi.check(hiplib.srsran_hip_nr_sch_create(C.byref(h)), "create")
    first = _nr_rm_run(S, capi, h, one)
    _nr_rm_run(S, capi, h, many)
    again = _nr_rm_run(S, capi, h, one)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    hiplib.srsran_hip_nr_sch_free(h)
    capi.check(hiplib.srsran_hip_nr_sch_create(C.byref(h)), "create again")
    assert all(np.array_equal(a, b) for a, b in zip(first, _nr_rm_run(S, capi, h, one)))
    hiplib.srsran_hip_nr_sch_free(h)


# ---------------------------------------------------------------------------------------------------------------- LTE transport blocks
def _tb_sizes(n, first=0):
    """transport blocks of ONE code block with distinct sizes: tbs = K - 24 for the turbo block sizes K = 40, 48, ... (no filler bits, whole bytes)"""
    return [40 + 8 * i - 24 for i in range(first, first + n)]


def _lte_case(sizes, seed, esn0_db=4.0):
    """one transport block per size, QPSK, about rate 1/3: coded bits, soft bits and the oracle's decode of each"""
    rng = np.random.default_rng(seed)
    tbs_l, e_tx, e_rx, pay, ref = [], [], [], [], []
    for tbs in sizes:
        G = 3 * (tbs + 24) + 12
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        e, _ = O.tb_coded_bits(tbs, 2, G, 0, None, payload=bits, tx_order=True)
        llr, payload = O.make_tb(tbs, 2, G, 0, esn0_db, rng, payload=bits)
        soft, crc = np.zeros((1, SB), np.int16), np.zeros(1, np.uint8)
        ret, o_data, o_avg = O.sch_decode_tb(tbs, 2, 0, llr, soft, crc, 6)
        tbs_l.append((tbs, G))
        e_tx.append(e)
        e_rx.append(llr)
        pay.append(np.packbits(bits))
        ref.append((ret, o_data, o_avg, crc[0]))
    return tbs_l, e_tx, e_rx, pay, ref


def _lte_encode(S, capi, h, case):
    tbs_l, e_tx, _, pay, _ = case
    tb, off_b, off_e = [], 0, 5
    for (tbs, G) in tbs_l:
        tb.append(capi.HipTb(tbs, 2, 0, G, off_e, off_b, 0))
        off_b += tbs // 8
        off_e += G + 3
    d_data = S.DeviceBuffer.from_numpy(np.concatenate(pay))
    d_e = S.DeviceBuffer.from_numpy(np.full(off_e // 8 + 16, 0xFF, np.uint8))
    capi.check(S.lib().srsran_hip_sch_encode(h, d_data.ptr, (capi.HipTb * len(tb))(*tb), len(tb), d_e.ptr, None), "sch_encode")
    capi.check(S.lib().srsran_hip_stream_sync(None), "sync")
    got = np.unpackbits(d_e.to_numpy(np.uint8, (off_e // 8 + 16,)))
    for t, e in zip(tb, e_tx):
        assert np.array_equal(got[t.e_offset:t.e_offset + e.size], e), t.tbs
    return got


def _lte_decode(S, capi, h, case, llrs=None, check_oracle=True):
    tbs_l, _, e_rx, pay, ref = case
    llrs = e_rx if llrs is None else llrs
    n = len(tbs_l)
    tb, off_e, off_d = [], 0, 0
    for i, (tbs, G) in enumerate(tbs_l):
        tb.append(capi.HipTb(tbs, 2, 0, G, off_e, off_d, i))
        off_e += llrs[i].size
        off_d += tbs // 8 + 6 + 3
    d_e = S.DeviceBuffer.from_numpy(np.concatenate(llrs))
    d_soft = S.DeviceBuffer.from_numpy(np.zeros((n, SB), np.int16))
    d_data = S.DeviceBuffer.from_numpy(np.zeros(off_d, np.uint8))
    cb_crc, res = np.zeros(n, np.uint8), (capi.HipTbResult * n)()
    capi.check(S.lib().srsran_hip_sch_decode(h, d_e.ptr, (capi.HipTb * n)(*tb), n, 6, d_soft.ptr, O.P(cb_crc), d_data.ptr, res, None), "sch_decode")
    data = d_data.to_numpy(np.uint8, (off_d,))
    for i, ((tbs, G), t) in enumerate(zip(tbs_l, tb)):
        if check_oracle:
            ret, o_data, o_avg, o_crc = ref[i]
            assert res[i].crc_ok == ret and cb_crc[i] == o_crc and abs(res[i].avg_iterations - o_avg) < 1e-6, (tbs, res[i].crc_ok, ret)
            assert np.array_equal(data[t.data_offset:t.data_offset + tbs // 8 + 6], o_data), tbs
        else:  # loop-back: clean soft bits
            assert res[i].crc_ok == 0, tbs
            assert np.array_equal(data[t.data_offset:t.data_offset + tbs // 8], pay[i]), tbs
    return data, cb_crc.copy(), [(r.crc_ok, r.avg_iterations, r.nof_cb) for r in res], d_soft.to_numpy(np.int16, (n, SB))


def _eq(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_transport_block_scratch_grows_and_is_used_again(hiplib):
    """srsran_hip_sch_encode and srsran_hip_sch_decode: one transport block of one code block, then 40, then the first again"""
    import srslte_amd as S
    from srslte_amd import capi

    one, many = _lte_case([4584], 31), _lte_case([152, 936] * 20, 32)
    he, hd = C.c_void_p(), C.c_void_p()
    capi.check(hiplib.srsran_hip_sch_enc_create(C.byref(he)), "enc_create")
    capi.check(hiplib.srsran_hip_sch_create(C.byref(hd)), "sch_create")
    e1, d1 = _lte_encode(S, capi, he, one), _lte_decode(S, capi, hd, one)
    _lte_encode(S, capi, he, many)
    _lte_decode(S, capi, hd, many)
    assert np.array_equal(_lte_encode(S, capi, he, one), e1) and _eq(_lte_decode(S, capi, hd, one), d1)
    hiplib.srsran_hip_sch_enc_free(he)
    hiplib.srsran_hip_sch_free(hd)
    capi.check(hiplib.srsran_hip_sch_enc_create(C.byref(he)), "enc_create again")
    capi.check(hiplib.srsran_hip_sch_create(C.byref(hd)), "sch_create again")
    assert np.array_equal(_lte_encode(S, capi, he, one), e1) and _eq(_lte_decode(S, capi, hd, one), d1)
    hiplib.srsran_hip_sch_enc_free(he)
    hiplib.srsran_hip_sch_free(hd)


@pytest.mark.parametrize("route,n_first,n_all", [("one launch, rows of 256", 12, 24), ("throughput kernels, rows of 64", 24, 48)])
def test_crc_multiplier_tables_past_their_first_capacity(hiplib, route, n_first, n_all):
    """distinct transport block sizes over two calls on ONE encoder and ONE decoder handle: the first call stays below the table's first capacity
    (16 rows of 256 lane multipliers, 32 rows of 64), the second passes it with the first call's sizes among its own -- so rows written before
    the table moved are read after it.  Encoder against the oracle's coded bits; decoder as the loop-back of test_transport_block_encode."""
    import srslte_amd as S
    from srslte_amd import capi

    lat = route.startswith("one launch")
    assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TCOD_LAT", b"1" if lat else b"0") == 0
    try:
        sizes = _tb_sizes(n_all)
        case = _lte_case(sizes, 40)
        first = tuple(c[:n_first] for c in case)
        he, hd = C.c_void_p(), C.c_void_p()
        capi.check(hiplib.srsran_hip_sch_enc_create(C.byref(he)), "enc_create")
        capi.check(hiplib.srsran_hip_sch_create(C.byref(hd)), "sch_create")
        clean = [np.where(e > 0, 40, -40).astype(np.int16) for e in case[1]]  # (the coded bits the encoder was just checked against)
        _lte_encode(S, capi, he, first)
        _lte_decode(S, capi, hd, first, clean[:n_first], check_oracle=False)
        _lte_encode(S, capi, he, case)
        _lte_decode(S, capi, hd, case, clean, check_oracle=False)
        hiplib.srsran_hip_sch_enc_free(he)
        hiplib.srsran_hip_sch_free(hd)
    finally:
        assert hiplib.srsran_hip_dev_knob(b"SRSRAN_HIP_TCOD_LAT", None) == 0


# ---------------------------------------------------------------------------------------------------------------- NR transport blocks
def _nr_tb_case(sizes, seed, sigma=3.0):
    """one transport block per (tbs, R): encoded by the oracle, soft bits, and the oracle's decode on cleared buffers"""
    rng = np.random.default_rng(seed)
    out = []
    for tbs, R in sizes:
        mod, Nl = 2, 1
        G = int(tbs / R) // 4 * 4 + 48
        cfg = O.sch_nr_tb_info(tbs, R, mod, G, Nl, NR_SB)  # (Nref = the largest code word: no limited buffer)
        payload = rng.integers(0, 256, tbs // 8).astype(np.uint8)
        e = O.sch_nr_encode_tb(cfg, 0, payload)
        llr = np.clip(np.round(9.0 * (1.0 - 2.0 * e) + sigma * rng.standard_normal(e.size)), -63, 63).astype(np.int8)
        soft, crc, data = np.zeros((cfg.C, NR_SB), np.int8), np.zeros(cfg.C, np.uint8), np.zeros((cfg.C, NR_DS), np.uint8)
        pay, ok, avg = O.sch_nr_decode_tb(cfg, 0, 0.8, 6, llr, soft, crc, data)
        out.append(dict(tbs=tbs, R=R, mod=mod, G=G, C=cfg.C, L_tb=cfg.L_tb, llr=llr, payload=payload, ref=(pay, ok, avg, crc)))
    return out


def _nr_tb_decode(S, capi, h, case, max_cb):
    tb, off_e, off_p, first = [], 0, 0, 0
    for c in case:
        tb.append(capi.HipNrTb(c["R"], c["tbs"], c["mod"], 0, 1, c["G"], NR_SB, off_e, off_p, first, 0))
        off_e += c["llr"].size
        off_p += c["tbs"] // 8
        first += c["C"]
    assert first <= max_cb
    n = len(case)
    d_llr = S.DeviceBuffer.from_numpy(np.concatenate([c["llr"] for c in case]))
    d_soft = S.DeviceBuffer.from_numpy(np.zeros((max_cb, NR_SB), np.int8))
    d_data = S.DeviceBuffer.from_numpy(np.zeros((max_cb, NR_DS), np.uint8))
    d_pay = S.DeviceBuffer.from_numpy(np.zeros(off_p, np.uint8))
    cb_crc, res = np.zeros(max_cb, np.uint8), (capi.HipNrTbResult * n)()
    capi.check(S.lib().srsran_hip_sch_nr_decode(h, d_llr.ptr, (capi.HipNrTb * n)(*tb), n, d_soft.ptr, NR_SB, cb_crc.ctypes.data, d_data.ptr, NR_DS, d_pay.ptr,
                                                res, None), "sch_nr_decode")
    pay = d_pay.to_numpy(np.uint8, (off_p,))
    for i, (c, t) in enumerate(zip(case, tb)):
        o_pay, ok, avg, crc = c["ref"]
        assert np.array_equal(cb_crc[t.first_cb:t.first_cb + c["C"]], crc), (i, c["tbs"])
        assert (res[i].crc_ok, res[i].all_decoded, res[i].nof_cb) == (ok, int(crc.all()), c["C"]) and abs(res[i].avg_iter - avg) < 1e-6, (i, c["tbs"])
        if crc.all():
            assert np.array_equal(pay[t.payload_offset:t.payload_offset + c["tbs"] // 8], o_pay), (i, c["tbs"])
    return pay, cb_crc.copy(), [(r.crc_ok, r.all_decoded, r.avg_iter, r.nof_cb) for r in res]


def test_nr_transport_block_buffers_grow_and_are_used_again(hiplib):
    """srsran_hip_sch_nr_decode: one transport block of one code block, then 40, then the first again"""
    import srslte_amd as S
    from srslte_amd import capi

    one, many = _nr_tb_case([(1056, 0.5)], 51), _nr_tb_case([(256 + 64 * (i % 5), 0.4) for i in range(40)], 52)
    assert one[0]["C"] == 1 and all(c["C"] == 1 for c in many)
    h = C.c_void_p()
    capi.check(hiplib.srsran_hip_sch_nr_create(C.byref(h), 0.8, 6, 48), "create")
    first = _nr_tb_decode(S, capi, h, one, 48)
    _nr_tb_decode(S, capi, h, many, 48)
    again = _nr_tb_decode(S, capi, h, one, 48)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    hiplib.srsran_hip_sch_nr_free(h)
    capi.check(hiplib.srsran_hip_sch_nr_create(C.byref(h), 0.8, 6, 48), "create again")
    again = _nr_tb_decode(S, capi, h, one, 48)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    hiplib.srsran_hip_sch_nr_free(h)


def test_nr_crc_multiplier_table_past_its_first_capacity(hiplib):
    """17 distinct (chunk of the transport-block CRC, CRC order) pairs on one handle, 16 rows being the table's first capacity: the chunk is
    ceil(bytes / 256) (nrsch::tb_finish_chunk), the order 16 up to 3824 bits and 24 above.  Ten pairs in a first call, all of them in a second."""
    import srslte_amd as S
    from srslte_amd import capi

    def tbs_of(chunk):  # a size of TS 38.214 5.1.3.2's form above 3824 bits, 8 C m - 24 (whole bytes in every code block), with that CRC chunk
        Cn = -(-(8 * (256 * chunk - 8) + 24) // 8424)
        return 8 * Cn * ((256 * chunk - 5) // Cn) - 24

    sizes = [(1984, 0.5), (2400, 0.5)] + [(tbs_of(c), 0.6) for c in range(2, 17)]
    case = _nr_tb_case(sizes, 53, sigma=1.0)
    pairs = {((c["tbs"] // 8 + 255) // 256, c["L_tb"]) for c in case}
    assert len(pairs) == 17 and {p[1] for p in pairs} == {16, 24}
    max_cb = sum(c["C"] for c in case)
    h = C.c_void_p()
    capi.check(hiplib.srsran_hip_sch_nr_create(C.byref(h), 0.8, 6, max_cb), "create")
    _nr_tb_decode(S, capi, h, case[:10], max_cb)
    _, _, res = _nr_tb_decode(S, capi, h, case, max_cb)
    assert all(r[0] == 1 for r in res)  # every transport CRC was computed with the right row, and passed
    hiplib.srsran_hip_sch_nr_free(h)


# ---------------------------------------------------------------------------------------------------------------- contexts that re-plan
def _dft_oracle(x, n):
    y = np.zeros(n, np.complex64)
    O.orc().orc_dft_c(O.P(np.ascontiguousarray(x, np.complex64)), O.P(y), n, 0, 0, 0, 0)
    return y


def test_dft_replan_across_the_four_step_limit(hiplib):
    """srsran_dft_plan_c at a four-step length, then srsran_dft_replan to a single-kernel length, to another four-step length (its work
    arrays and both twiddle tables are allocated anew), and to the small length again -- each against the oracle with test_gpu_dft's
    tolerances (1e-4 of the output RMS up to 4096 points, 2e-4 above); then a fresh plan after srsran_dft_plan_free"""
    from srslte_amd import capi

    rng = np.random.default_rng(9)
    xs = {n: (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for n in (9728, 600, 8192)}

    def run(plan, n):
        y = np.zeros(n, np.complex64)
        hiplib.srsran_dft_run_c(C.byref(plan), O.P(xs[n]), O.P(y))
        if n <= 4096:
            ref = _dft_oracle(xs[n], n)
            assert float(np.abs(y - ref).max()) / max(1.0, float(np.sqrt(np.mean(np.abs(ref) ** 2)))) < 1e-4, n
        else:
            ref = np.fft.fft(xs[n].astype(np.complex128))
            assert np.abs(y - ref).max() < 2e-4 * max(1.0, np.sqrt(np.mean(np.abs(ref) ** 2))), n
        return y

    plan = capi.DftPlan()
    assert hiplib.srsran_dft_plan_c(C.byref(plan), 9728, 0) == 0
    big = run(plan, 9728)
    assert hiplib.srsran_dft_replan(C.byref(plan), 600) == 0 and plan.size == 600
    small = run(plan, 600)
    assert hiplib.srsran_dft_replan(C.byref(plan), 8192) == 0
    run(plan, 8192)
    assert hiplib.srsran_dft_replan(C.byref(plan), 600) == 0
    assert np.array_equal(run(plan, 600), small)
    assert hiplib.srsran_dft_replan(C.byref(plan), 9728) == 0
    assert np.array_equal(run(plan, 9728), big)
    hiplib.srsran_dft_plan_free(C.byref(plan))
    assert hiplib.srsran_dft_plan_c(C.byref(plan), 600, 0) == 0
    assert np.array_equal(run(plan, 600), small)
    hiplib.srsran_dft_plan_free(C.byref(plan))


def test_ofdm_handle_at_6_25_and_6_prb(hiplib):
    """one srsran_ofdm_t: set to 6 PRB, 25 PRB (its device object is rebuilt and its staging grows) and 6 PRB again, a subframe each,
    against the oracle with test_gpu_ofdm's tolerance; then a fresh handle after srsran_ofdm_rx_free"""
    from srslte_amd import capi

    lib = hiplib
    rng = np.random.default_rng(4)
    tin, rout = np.zeros(15 * 384, np.complex64), np.zeros(14 * 300, np.complex64)
    xs = {prb: ((rng.standard_normal(15 * n) + 1j * rng.standard_normal(15 * n)) * 0.7).astype(np.complex64) for prb, n in ((6, 128), (25, 384))}

    def run(q, prb):
        assert lib.srsran_ofdm_rx_set_prb(C.byref(q), capi.CP_NORM, prb) == 0
        x = xs[prb]
        assert q.sf_sz == x.size and q.nof_re == 12 * prb
        tin[:x.size] = x
        lib.srsran_ofdm_rx_sf(C.byref(q))
        got, ref = rout[:14 * 12 * prb].copy(), O.ofdm_rx(O.ofdm_cfg(prb), x[None])[0]
        assert float(np.abs(got - ref).max()) / max(1.0, float(np.sqrt(np.mean(np.abs(ref) ** 2)))) < 1e-4, prb
        return got

    q = capi.Ofdm()
    assert lib.srsran_ofdm_rx_init(C.byref(q), capi.CP_NORM, tin.ctypes.data, rout.ctypes.data, 25) == 0
    first = run(q, 6)
    run(q, 25)
    assert np.array_equal(run(q, 6), first)
    lib.srsran_ofdm_rx_free(C.byref(q))
    q = capi.Ofdm()
    assert lib.srsran_ofdm_rx_init(C.byref(q), capi.CP_NORM, tin.ctypes.data, rout.ctypes.data, 25) == 0
    assert np.array_equal(run(q, 6), first)
    lib.srsran_ofdm_rx_free(C.byref(q))


def test_pss_resize_to_a_larger_frame_and_back(hiplib):
    """srsran_pss_resize to half the frame, to the full frame and back: the search of a capture at each size against the oracle, with the
    tolerances of test_gpu_sync (equal peak position, peak value within 1e-4, PSR within 1e-3); then a fresh object after srsran_pss_free"""
    from srslte_amd import capi
    from test_gpu_sync import _capture

    lib = hiplib
    rng = np.random.default_rng(12)
    N, prb = 128, 6
    caps = {frame: _capture(7, prb, N, frame, delay, 0.05, rng) for frame, delay in ((4800, 1500), (9600, 3000))}

    def find(q, frame):
        psr = C.c_float()
        pk, pv, opsr = O.pss_find(caps[frame], N, 1)[:3]
        assert lib.srsran_pss_find_pss(C.byref(q), O.P(caps[frame]), C.byref(psr)) == pk
        assert abs(psr.value - opsr) <= 1e-3 * opsr and abs(q.peak_value - pv) <= 1e-4 * pv
        return pk, psr.value, q.peak_value

    def resize(q, frame):  # (as in the reference, srsran_pss_resize forgets N_id_2 and the averaging weight: pss.c:237-241)
        assert lib.srsran_pss_resize(C.byref(q), frame, N, 0) == 0 and q.frame_size == frame
        assert lib.srsran_pss_set_N_id_2(C.byref(q), 1) == 0
        lib.srsran_pss_set_ema_alpha(C.byref(q), 1.0)

    q = capi.Pss()
    assert lib.srsran_pss_init_fft(C.byref(q), 9600, N) == 0
    resize(q, 4800)
    first = find(q, 4800)
    resize(q, 9600)
    find(q, 9600)
    resize(q, 4800)
    assert find(q, 4800) == first
    lib.srsran_pss_free(C.byref(q))
    q = capi.Pss()
    assert lib.srsran_pss_init_fft(C.byref(q), 9600, N) == 0
    resize(q, 4800)
    assert find(q, 4800) == first
    lib.srsran_pss_free(C.byref(q))


# ---------------------------------------------------------------------------------------------------------------- create, use, free, create again
def test_create_use_free_and_create_again(hiplib):
    """handle types the tests above do not free and re-create: the turbo, LDPC and OFDM batch objects, the cell search and the turbo encoder
    behind srsran_tcod_t -- one small call each, equal to the oracle, and equal again after free and create"""
    import srslte_amd as S
    from srslte_amd import capi

    lib = hiplib
    rng = np.random.default_rng(77)
    _, t_llr = O.turbo_llrs(512, 3, 1.0, seed=7)
    t_ref = O.turbo_decode(t_llr, 4, 512)
    _, l_llr = O.ldpc_llrs(1, 16, 2, 2.0, seed=3)
    l_ref, _ = O.ldpc_decode(1, 16, l_llr, 0.8, 10)
    ocfg = O.ofdm_cfg(6, 0, 0, 1)
    sf_sz = O.ofdm_geometry(ocfg)[2]
    o_x = (rng.standard_normal((1, sf_sz)) + 1j * rng.standard_normal((1, sf_sz))).astype(np.complex64) * 0.7
    o_ref = O.ofdm_rx(ocfg, o_x)
    c_bits = rng.integers(0, 2, 512).astype(np.uint8)
    c_ref = np.zeros(3 * 512 + 12, np.uint8)
    assert O.orc().orc_tcod_encode(O.P(c_bits), O.P(c_ref), 512) == 0
    from test_gpu_sync import _capture, _run_batch

    cap = _capture(151, 6, 128, 9600, 2000, 0.05, rng)[None]
    pk = O.pss_find(cap[0], 128, 151 % 3)[0]
    seen = []
    for _ in range(2):
        b = S.TdecBatch(512, 3, capi.TDEC_AUTO)
        t = b.decode(t_llr, 4)
        b.free()
        b = S.LdpcBatch(1, 16, 0.8, 10, 2)
        ld = b.decode(l_llr)
        b.free()
        b = S.OfdmBatch(6, False, 0, normalize=True)
        of = b.process(o_x)
        b.free()
        h, cells = _run_batch(S, cap, 9600, 128, 1)
        cs = [(c.peak_pos, c.peak_value, c.psr, c.N_id_1) for c in cells]
        lib.srsran_hip_cellsearch_free(h)
        q = capi.Tcod()
        assert lib.srsran_tcod_init(C.byref(q), 6144) == 0
        enc = np.zeros(3 * 512 + 12, np.uint8)
        assert lib.srsran_tcod_encode(C.byref(q), O.P(c_bits), O.P(enc), 512) == 0
        lib.srsran_tcod_free(C.byref(q))
        assert np.array_equal(t, t_ref) and np.array_equal(ld, l_ref) and np.abs(of - o_ref).max() < 1e-4 and np.array_equal(enc, c_ref)
        assert cs[151 % 3][0] == pk and cs[151 % 3][3] == 151 // 3
        seen.append((t, ld, of, enc, cs))
    for a, b in zip(seen[0][:4], seen[1][:4]):
        assert np.array_equal(a, b)
    assert seen[0][4] == seen[1][4]


def test_contexts_behind_the_reference_structs_create_use_free_and_init_again(hiplib):
    """the contexts behind srsran_tdec_t, srsran_ldpc_decoder_t, srsran_sss_t and srsran_ldpc_rm_t / srsran_ldpc_encoder_t: init, one small call
    against the oracle as the family's own tests make it, free, init again on the same thread, the same call with the same result"""
    from srslte_amd import capi
    from test_gpu_sync import _capture

    lib = hiplib
    rng = np.random.default_rng(78)
    K, nit = 512, 4
    _, t_llr = O.turbo_llrs(K, 1, 0.5, 9)
    t_ref = O.turbo_decode(t_llr, nit, K)[0]
    bg, Z, F, mod = 1, 16, 4, 2
    N, Kl = 50 * Z, 10 * Z
    _, l_llr = O.ldpc_llrs(bg, Z, 1, 2.0, seed=4)
    l_llr = np.ascontiguousarray(l_llr[0, :N])
    l_ref, l_ret = O.ldpc_decode(bg, Z, l_llr[None], 0.8, 9, None)
    cid = 3 * 55 + 2
    xx = _capture(cid, 6, 128, 9600, 2000, 0.05, rng, sf5=True)
    pos = 2000 + 960 - 2 * (128 + 9) + 9
    sym = xx[pos:pos + 128].copy()
    s_ref = O.sss_detect(sym, 128, cid % 3, 1)
    msg = rng.integers(0, 2, Kl).astype(np.uint8)
    msg[Kl - F:] = 254
    cw_ref = O.ldpc_encode_rm(bg, Z, msg, N)
    E = N * 3 // 4 // O.QM[mod] * O.QM[mod]
    tx_ref = O.ldpc_rm_tx(cw_ref, E, bg, Z, 0, mod, N)
    x = rng.integers(-60, 61, E).astype(np.int8)
    rx_ref, rx_ret = O.ldpc_rm_rx(x, np.zeros(N, np.int8), F, bg, Z, 0, mod, N)
    seen = []
    for _ in range(2):
        h = capi.Tdec()
        assert lib.srsran_tdec_init(C.byref(h), 6144) == 0
        lib.srsran_tdec_force_not_sb(C.byref(h))
        t_in, t_out = t_llr[0].copy(), np.zeros(K // 8, np.uint8)
        assert lib.srsran_tdec_run_all(C.byref(h), O.P(t_in), O.P(t_out), nit, K) == 0
        lib.srsran_tdec_free(C.byref(h))
        assert np.array_equal(t_out, t_ref)
        q = capi.LdpcDecoder()
        args = capi.LdpcDecoderArgs(capi.LDPC_C, bg, Z, 0.8, 9)
        assert lib.srsran_ldpc_decoder_init(C.byref(q), C.byref(args)) == 0
        l_out = np.zeros(Kl, np.uint8)
        ret = lib.srsran_ldpc_decoder_decode_c(C.byref(q), O.P(l_llr), O.P(l_out), N)
        lib.srsran_ldpc_decoder_free(C.byref(q))
        assert ret == l_ret[0] and np.array_equal(l_out, l_ref[0])
        s = capi.Sss()
        assert lib.srsran_sss_init(C.byref(s), 128) == 0 and lib.srsran_sss_set_N_id_2(C.byref(s), cid % 3) == 0
        m0, m1, v0, v1 = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float()
        assert lib.srsran_sss_m0m1_partial(C.byref(s), O.P(sym), 1, None, C.byref(m0), C.byref(v0), C.byref(m1), C.byref(v1)) == 0
        nid = lib.srsran_sss_N_id_1(C.byref(s), m0.value, m1.value, v0.value + v1.value)
        lib.srsran_sss_free(C.byref(s))
        assert (m0.value, m1.value, nid) == (s_ref[0], s_ref[1], s_ref[4]) and nid == cid // 3 and abs(v0.value - s_ref[2]) <= 1e-3 * s_ref[2]
        enc, tx, rxc = capi.LdpcEncoder(), capi.LdpcRm(), capi.LdpcRm()
        assert lib.srsran_ldpc_encoder_init(C.byref(enc), 0, bg, Z) == 0
        assert lib.srsran_ldpc_rm_tx_init(C.byref(tx)) == 0 and lib.srsran_ldpc_rm_rx_init_c(C.byref(rxc)) == 0
        cw, e_out, soft = np.full(N, 7, np.uint8), np.zeros(E, np.uint8), np.zeros(N, np.int8)
        assert lib.srsran_ldpc_encoder_encode_rm(C.byref(enc), O.P(msg), O.P(cw), msg.size, N) == 0
        assert lib.srsran_ldpc_rm_tx(C.byref(tx), O.P(cw), O.P(e_out), E, bg, Z, 0, mod, N) == 0
        r = lib.srsran_ldpc_rm_rx_c(C.byref(rxc), O.P(x), O.P(soft), E, F, bg, Z, 0, mod, N)
        lib.srsran_ldpc_encoder_free(C.byref(enc))
        lib.srsran_ldpc_rm_tx_free(C.byref(tx))
        lib.srsran_ldpc_rm_rx_free_c(C.byref(rxc))
        assert np.array_equal(cw, cw_ref) and np.array_equal(e_out, tx_ref) and np.array_equal(soft, rx_ref) and r == rx_ret
        seen.append((t_out, l_out, (m0.value, m1.value, v0.value, v1.value), cw, e_out, soft))
    for a, b in zip(seen[0], seen[1]):
        assert np.array_equal(a, b)
