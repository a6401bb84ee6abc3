// warmup_host.cpp -- warm start (srsran_hip_warmup, include/srsran_amd/phy_chan_abi.h).
//
// The first grant of a process used to cost 20-28 ms (profiles/r03_ref_programs.json: pdsch_test -X 1): the device code of every kernel on the path is
// loaded at its first launch, the thread's staging contexts create their stream, pinned and device images, decoder and encoder objects, transform plans,
// and every (block size, redundancy version) brings its rate-matching table.  The reference does that kind of work in srsran_sch_init (sch.c:159-197:
// allocation, srsran_tdec_init, srsran_rm_turbo_gentables) -- so does the library: srsran_rm_turbo_gentables() builds every rate-matching table in
// one allocation and warms ONE worker's contexts; srsran_hip_warmup(n) makes that n.  A warm context is made by running real calls -- the largest
// grant of a 100-PRB cell, a one-block grant and a scalar-decoder grant, receive and transmit side, 16- and 8-bit soft bits, one CSI-weighted grant of each
// width, one 2-port transmit-diversity grant and one two-codeword spatial-multiplexing grant each way, one PDSCH grant from the subframe grids with and without the channel estimator in front, one PUSCH
// transmit grant with control information, one small PDCCH candidate call -- on a short-lived
// thread whose contexts go back to the pools (hip_common.h: StagePool) when it ends.
#include "stage.h"
#include "turbo_device.h"
#include "srsran_amd/phy_chan_abi.h"
#include "srsran_amd/phy_conv_abi.h"
#include "srsran_amd/phy_nr_chan_abi.h"

#include <algorithm>
#include <condition_variable>
#include <thread>
#include <vector>

using namespace phyhip;

namespace {

struct HostSoftbuffers {
  std::vector<std::vector<int16_t>> rows;
  std::vector<std::vector<uint8_t>> keep, txrows;
  std::vector<int16_t*>             rp;
  std::vector<uint8_t*>             kp, tp;
  std::vector<uint8_t>              flags; // bool-sized
  srsran_softbuffer_rx_t            rx;
  srsran_softbuffer_tx_t            tx;
  explicit HostSoftbuffers(uint32_t n) : rows(n), keep(n), txrows(n), rp(n), kp(n), tp(n), flags(n, 0)
  {
    for (uint32_t i = 0; i < n; i++) {
      rows[i].assign(SRSRAN_HIP_SOFTBUFFER_CB_SIZE, 0);
      keep[i].assign(SRSRAN_HIP_SOFTBUFFER_CB_SIZE / 8, 0);
      txrows[i].assign(SRSRAN_HIP_SOFTBUFFER_CB_SIZE, 0);
      rp[i] = rows[i].data();
      kp[i] = keep[i].data();
      tp[i] = txrows[i].data();
    }
    rx = {n, SRSRAN_HIP_SOFTBUFFER_CB_SIZE, rp.data(), kp.data(), reinterpret_cast<bool*>(flags.data()), false};
    tx = {n, SRSRAN_HIP_SOFTBUFFER_CB_SIZE, tp.data()};
  }
  void reset()
  {
    for (auto& r : rows) {
      std::fill(r.begin(), r.end(), 0);
    }
    std::fill(flags.begin(), flags.end(), 0);
  }
};

void warm_one_worker()
{
  const uint32_t nof_prb = 100, L_prb = 100, nsymb = 12;
  // transport block sizes without filler bits: C blocks of K = 6144 carry C (6144 - 24) - 24 payload bits (C > 1), one block K - 24
  const struct {
    uint32_t tbs, mod, L;
  } grants[] = {{13 * 6120 - 24, SRSRAN_MOD_64QAM, L_prb}, {6144 - 24, SRSRAN_MOD_16QAM, 12}, {40 - 24, SRSRAN_MOD_QPSK, 1}};
  HostSoftbuffers      sb(13);
  std::vector<cf_t>    grid((size_t)14 * 12 * nof_prb, cf_t(0.5f, -0.5f)), ce((size_t)14 * 12 * nof_prb, cf_t(1.f, 0.f)), sym((size_t)nsymb * 12 * L_prb), qsym((size_t)nsymb * 12 * 12);
  std::vector<uint8_t> data(13 * 768 + 64, 0x5a), qbits((size_t)nsymb * 12 * L_prb * 6 / 8 + 8);
  for (uint32_t llr8 = 0; llr8 < 2; llr8++) {
    for (const auto& gr : grants) {
      const uint32_t        nof_re = nsymb * 12 * gr.L;
      srsran_hip_grant_tb_t tb     = {gr.mod, gr.tbs, 0, nof_re, 12345u, 1, llr8, 1};
      srsran_hip_grant_res_t res;
      // receive: PUSCH grant from the grid, PDSCH codeword with and without the equaliser
      srsran_hip_pusch_rx_t pu = {tb, nof_prb, 7, {0, 0}, gr.L, 0, 0.01f, 0};
      sb.reset();
      (void)srsran_hip_pusch_decode(&pu, grid.data(), ce.data(), &sb.rx, data.data(), &res);
      srsran_hip_pdsch_rx_t pd = {tb, 1.0f, 0.01f};
      sb.reset();
      (void)srsran_hip_pdsch_decode_dbg(&pd, grid.data(), ce.data(), &sb.rx, data.data(), &res, sym.data(), nullptr);
      // (a retransmission: the rows that came back are combined into)
      tb.rv = 2;
      pd.tb = tb;
      (void)srsran_hip_pdsch_decode(&pd, grid.data(), nullptr, &sb.rx, data.data(), &res);
      tb.rv = 0;
      if (gr.L == 12) { // one CSI-weighted grant per soft-bit width (cfg->csi_enable, srsue's default): csi_kernels.hip is loaded
        pd.tb = tb;
        sb.reset();
        (void)srsran_hip_pdsch_decode_csi(&pd, grid.data(), ce.data(), nullptr, &sb.rx, data.data(), &res);
      }
      if (!llr8) { // transmit
        srsran_hip_pdsch_tx_t tx = {tb, 1.0f};
        (void)srsran_hip_pdsch_encode_dbg(&tx, &sb.tx, data.data(), sym.data(), qbits.data());
        (void)srsran_hip_ulsch_encode(&tb, nsymb, &sb.tx, data.data(), qbits.data());
      }
    }
  }
  // one PUSCH transmit grant with control information (the one-block 16-QAM grant, 12 PRB: ACK, RI and CQI symbols), so the device code of
  // pusch_tx_kernels.hip and the forward transform plan are there before a UE worker's first uplink subframe
  {
    const uint32_t                  L = 12, nof_re = nsymb * 12 * L, Qm = 4;
    const srsran_hip_pusch_tx_t     tx  = {{SRSRAN_MOD_16QAM, 6144 - 24, 0, nof_re, 12345u, 1, 0, 1}, nof_prb, 7, {0, 0}, L, 0};
    const srsran_hip_pusch_uci_t    uci = {24, 5, 60};
    const std::vector<uint8_t>      types((24 + 5) * Qm, 1), cqi(60 * Qm, 1);
    const srsran_hip_pusch_uci_in_t in  = {types.data(), types.data() + 24 * Qm, cqi.data()};
    (void)srsran_hip_pusch_encode(&tx, &uci, &in, &sb.tx, data.data(), grid.data());
  }
  // one PDSCH grant from the subframe grids (12 PRB of the 100-PRB cell, subframe 1, one control symbol: 1800 REs; CSI-weighted), so the device code of
  // pdsch_map_kernels.hip is loaded before a UE worker's first srsran_pdsch_decode
  {
    srsran_hip_pdsch_sf_t sf = {nof_prb, 1, 1, 7, 0, 1, 1, {7, 7}, 1, {}};
    for (uint32_t n = 40; n < 52; n++) {
      sf.prb_idx[0][n] = sf.prb_idx[1][n] = 1;
    }
    const int                   nof_re = srsran_hip_pdsch_nof_re(&sf);
    const srsran_hip_pdsch_rx_t pd     = {{SRSRAN_MOD_16QAM, 6144 - 24, 0, (uint32_t)(nof_re > 0 ? nof_re : 0), 12345u, 1, 0, 1}, 1.0f, 0.01f};
    srsran_hip_grant_res_t      res;
    sb.reset();
    (void)srsran_hip_pdsch_decode_sf(&pd, &sf, grid.data(), ce.data(), &sb.rx, data.data(), &res);
    // and the same grant from the received grid alone (srsue's default estimator), so the device code of chest_dl_kernels.hip is loaded as well; `ce` serves
    // as the pilot row (8 nof_prb points of it are read)
    srsran_hip_chest_dl_t est = {};
    est.nof_prb = nof_prb;
    est.nof_ports = est.nof_rx = est.id = est.sf_idx = 1;
    est.cp_nsymb       = 7;
    est.estimator_alg  = SRSRAN_HIP_ESTIMATOR_ALG_AVERAGE;
    est.noise_alg      = SRSRAN_HIP_NOISE_ALG_REFS;
    est.filter_type    = SRSRAN_HIP_CHEST_FILTER_GAUSS;
    est.filter_coef[0] = 4.0f;
    est.filter_coef[1] = 1.0f;
    est.pilots[0]      = ce.data();
    const srsran_hip_chest_dl_state_t state = {};
    srsran_hip_chest_dl_res_t         est_out;
    sb.reset();
    (void)srsran_hip_pdsch_decode_est(&pd, &sf, &est, &state, grid.data(), &sb.rx, data.data(), &res, &est_out);
  }
  // one 2-port transmit-diversity codeword each way (the one-block 16-QAM grant above: 1728 REs on two layers), so the device code of txdiv_kernels.hip
  // is loaded before the first subframe of a 2-port cell
  {
    const uint32_t               nof_re = nsymb * 12 * 12;
    const srsran_hip_grant_tb_t  tb     = {SRSRAN_MOD_16QAM, 6144 - 24, 0, nof_re, 12345u, 1, 0, 2};
    std::vector<cf_t>            port1(nof_re);
    cf_t* const                  planes[SRSRAN_MAX_PORTS] = {sym.data(), port1.data(), nullptr, nullptr};
    cf_t* const                  est[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{ce.data(), ce.data()}, {ce.data(), ce.data()}};
    srsran_hip_pdsch_txdiv_tx_t  tx = {tb, 2, 1.0f};
    srsran_hip_pdsch_txdiv_rx_t  rx = {tb, 2, 2, 1.0f, 0};
    srsran_hip_grant_res_t       res;
    (void)srsran_hip_pdsch_encode_txdiv(&tx, &sb.tx, data.data(), planes);
    sb.reset();
    (void)srsran_hip_pdsch_decode_txdiv_dbg(&rx, planes, est, &sb.rx, data.data(), &res, qsym.data(), nullptr);
  }
  // one two-codeword spatial-multiplexing grant each way on the same planes (16-QAM + QPSK, 1728 REs, one block each), so the device code of
  // spmux_kernels.hip is loaded before the first TM3 / TM4 subframe
  {
    const uint32_t               nof_re = nsymb * 12 * 12;
    const srsran_hip_grant_tb_t  tb0    = {SRSRAN_MOD_16QAM, 6144 - 24, 0, nof_re, 12345u, 1, 0, 1};
    const srsran_hip_grant_tb_t  tb1    = {SRSRAN_MOD_QPSK, 3136 - 24, 0, nof_re, 54321u, 1, 0, 1};
    std::vector<cf_t>            port1(nof_re), est1(nof_re, cf_t(0.f, 0.5f));
    cf_t* const                  planes[SRSRAN_MAX_PORTS] = {sym.data(), port1.data(), nullptr, nullptr};
    cf_t* const                  est[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{ce.data(), est1.data()}, {est1.data(), ce.data()}};
    HostSoftbuffers              sb1(1);
    srsran_softbuffer_tx_t* const stx[2] = {&sb.tx, &sb1.tx};
    srsran_softbuffer_rx_t* const srx[2] = {&sb.rx, &sb1.rx};
    std::vector<uint8_t>         data1(3136 / 8 + 64, 0xa5);
    uint8_t* const               pay[2] = {data.data(), data1.data()};
    srsran_hip_pdsch_mimo_tx_t   tx = {{tb0, tb1}, 2, 2, SRSRAN_HIP_TXSCHEME_SPATIALMUX, 1, 1.0f};
    srsran_hip_pdsch_mimo_rx_t   rx = {{tb0, tb1}, 2, 2, SRSRAN_HIP_TXSCHEME_SPATIALMUX, 1, SRSRAN_HIP_MIMO_DECODER_MMSE, 2, 1.0f, 0.01f};
    srsran_hip_grant_res_t       res[2];
    cf_t* const                  dd[2] = {qsym.data(), nullptr};
    (void)srsran_hip_pdsch_encode_mimo(&tx, stx, pay, planes);
    sb.reset();
    (void)srsran_hip_pdsch_decode_mimo_dbg(&rx, planes, est, srx, pay, res, dd, nullptr);
  }
  // NR: one codeword through the one-call paths of phy_nr_chan_abi.h, transmit then receive -- the 8-block 256-QAM transport block of a 100 MHz
  // carrier with the reference's default decoder parameters, so a worker's first slot finds its context, decoder objects and kernels ready
  {
    const uint32_t            nr_re = 12672, nr_cb = 8, nr_N = 66 * 384;
    srsran_hip_nr_tb_t        ntb   = {0.67, 67368, SRSRAN_MOD_256QAM, 0, 1, 8 * nr_re, 0, 0, 0, 0, 0};
    std::vector<cf_t>         nsym(nr_re), nce(nr_re, cf_t(1.f, 0.f));
    std::vector<uint8_t>      npay(ntb.tbs / 8 + 8, 0x5a), nrows((size_t)nr_cb * nr_N, 0), nkeep((size_t)nr_cb * (8448 / 8), 0), nflags(nr_cb, 0);
    std::vector<int16_t*>     nrp(nr_cb);
    std::vector<uint8_t*>     nkp(nr_cb);
    for (uint32_t r = 0; r < nr_cb; r++) {
      nrp[r] = reinterpret_cast<int16_t*>(nrows.data() + (size_t)r * nr_N);
      nkp[r] = nkeep.data() + (size_t)r * (8448 / 8);
    }
    srsran_softbuffer_rx_t    nsb = {nr_cb, nr_N, nrp.data(), nkp.data(), reinterpret_cast<bool*>(nflags.data()), false};
    srsran_hip_nr_cw_tx_t     ntx = {ntb, nr_re, 12345u, 1.0f, 0};
    srsran_hip_nr_cw_rx_t     nrx = {ntb, nr_re, 12345u, 0.f, 0, 0.01f, 0};
    srsran_hip_nr_tb_result_t nres;
    (void)srsran_hip_nr_cw_encode(&ntx, npay.data(), nsym.data());
    (void)srsran_hip_nr_cw_decode(&nrx, nsym.data(), nce.data(), &nsb, npay.data(), &nres);
  }
  // two PDCCH candidates of a 6-CCE control region (conv_host.cpp), so the device code of conv_kernels.hip is loaded and the context's images exist
  // before a UE worker's first blind search
  {
    const std::vector<float>      llr(6 * 72, 1.0f);
    const srsran_hip_pdcch_cand_t cand[2] = {{0, 0, 27}, {2, 2, 43}};
    srsran_hip_pdcch_res_t        pres[2];
    (void)srsran_hip_pdcch_dci_decode_multi(llr.data(), (uint32_t)llr.size(), 2, cand, pres);
  }
}

struct WarmState { // per device
  std::mutex mu;
  uint32_t   workers = 0;
};

} // namespace

extern "C" int srsran_hip_warmup(uint32_t nof_workers)
{
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  bind_thread();
  WarmState&                  ws = device_local<WarmState>(); // of the calling thread's device
  std::lock_guard<std::mutex> lk(ws.mu);
  const int                   dev = current_device();
  if (!rm::build_all_tables() || !turbo::prebuild_tables()) {
    return SRSRAN_ERROR;
  }
  // the workers' contexts are made by threads that exist TOGETHER (a context goes back to the pool when its thread ends: one after the other they
  // would all warm the same one)
  const uint32_t have = ws.workers;
  if (have < nof_workers) {
    const uint32_t           n = nof_workers - have;
    std::mutex               mu;
    std::condition_variable  cv;
    uint32_t                 done = 0;
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n; i++) {
      th.emplace_back([&] {
        (void)srsran_hip_set_thread_device(dev);
        warm_one_worker();
        std::unique_lock<std::mutex> l(mu);
        done++;
        cv.notify_all();
        cv.wait(l, [&] { return done == n; });
      });
    }
    for (auto& t : th) {
      t.join(); // their contexts are in the pools now
    }
    ws.workers = nof_workers;
  }
  return SRSRAN_SUCCESS;
}
