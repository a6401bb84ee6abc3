// nr_chan_host.cpp -- one device call per NR codeword (include/srsran_amd/phy_nr_chan_abi.h):
//   receive   pdsch_nr_decode_codeword (lib/src/phy/phch/pdsch_nr.c:426-483, behind the single-port equaliser of :540) and pusch_nr_decode_codeword
//             without control information (pusch_nr.c:830-911): nr_front_kernel, then the transport-block loop of sch_nr_host.cpp on soft bits that
//             never leave the device
//   transmit  pdsch_nr_encode_codeword (pdsch_nr.c:304-351): srsran_hip_sch_nr_encode, then nr_mod_kernel on its bit-per-byte output
// The staging context is the transport-block one of sch_nr_host.cpp (one per worker thread).  One image layout serves the pinned host image and the
// device buffer; every region starts on a multiple of 256 bytes -- in particular every codeword's soft bits, so the front end's 16-byte stores are
// aligned whatever the lengths of the codewords in front of it (the kernel falls back to byte stores on a base that is not):
//   [soft rows | data rows | per codeword: symbols, channel estimates | per codeword: soft bits / coded bits | per codeword: payload | job lists]
// Symbols, estimates, payloads and job lists are read from the pinned image by the kernels themselves; soft rows, data rows and soft bits live in the
// device buffer.
#include "hip_common.h"
#include "joblist.h"
#include "nr_chan_device.h"
#include "nr_chest_device.h"
#include "sch_nr_internal.h"
#include "srsran_amd/phy_nr_chan_abi.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace phyhip;
using namespace phyhip::nrtb;

namespace {

#define NR_CW_REFUSE(...)                                                                                              \
  do {                                                                                                                 \
    fprintf(stderr, "[srsran_phy_hip] " __VA_ARGS__);                                                                  \
    fputc('\n', stderr);                                                                                               \
    return SRSRAN_ERROR_INVALID_INPUTS;                                                                                \
  } while (0)

// the checks both directions share; fills the transport-block parameters
int check_tb(const char* who, uint32_t i, const srsran_hip_nr_tb_t& tb, uint32_t nof_re, TbCfg* c)
{
  if (tb.mod < SRSRAN_MOD_QPSK || tb.mod > SRSRAN_MOD_256QAM) {
    NR_CW_REFUSE("%s: codeword %u: modulation %u outside QPSK .. 256-QAM", who, i, tb.mod);
  }
  if (!tb_cfg(tb, c)) {
    NR_CW_REFUSE("%s: codeword %u: invalid transport block (tbs %u, layers %u, rv 0x%x)", who, i, tb.tbs, tb.N_L, tb.rv);
  }
  if (nof_re == 0 || (uint64_t)nof_re * c->Qm != tb.nof_bits) {
    NR_CW_REFUSE("%s: codeword %u: nof_bits %u is not nof_re %u x %u", who, i, tb.nof_bits, nof_re, c->Qm);
  }
  if (tb.nof_bits > SRSRAN_HIP_SEQUENCE_MAX_LEN) {
    NR_CW_REFUSE("%s: codeword %u: %u bits exceed the sequence tables (%u)", who, i, tb.nof_bits, SRSRAN_HIP_SEQUENCE_MAX_LEN);
  }
  if (tb.nof_bits < c->C * c->Nl * c->Qm) { // sch_nr_get_E would hand a code block no bit at all
    NR_CW_REFUSE("%s: codeword %u: %u bits for %u code blocks", who, i, tb.nof_bits, c->C);
  }
  return SRSRAN_SUCCESS;
}

struct RxCw { // one codeword of a receive call
  TbCfg      c;
  uint32_t   first_cb;
  size_t     o_sym, o_ce, o_e, o_pay;
  SoftStager harq; // its soft buffer, in and out
};

// the one line of a call that failed behind its first enqueue: the step, and what that step left as the last error
int failed_at(const char* who, const char* what)
{
  fprintf(stderr, "[srsran_phy_hip] %s: %s: %s\n", who, what, get_error());
  return SRSRAN_ERROR;
}

// grids == nullptr: the codewords come as extracted REs (symbols, ce).  Else symbols and ce are not looked at: codeword i is described by grids[i] on the
// one slot grid sf_symbols, the estimator and the de-mapper (nr_chest_kernels.hip) run in front of the front end and leave its inputs in the device
// buffer; chest (may be nullptr) receives the estimator's measurements.
int nr_cw_decode(uint32_t n, const srsran_hip_nr_cw_rx_t* g, const cf_t* const* symbols, const cf_t* const* ce, srsran_softbuffer_rx_t* const* softbuffers,
                 uint8_t* const* payloads, srsran_hip_nr_tb_result_t* res, int8_t* e_out, const srsran_hip_nr_grid_t* grids = nullptr,
                 const cf_t* sf_symbols = nullptr, srsran_hip_nr_chest_res_t* chest = nullptr)
{
  const char* who = grids ? "nr_cw_decode_grid" : "nr_cw_decode";
  TraceRange  trace_("srsran_hip_nr_cw_decode");
  if (res) {
    memset(res, 0, (size_t)n * sizeof(*res)); // every result is initialised before anything is checked
  }
  if (chest) {
    memset(chest, 0, (size_t)n * sizeof(*chest));
  }
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || (!grids && !symbols) || (grids && !sf_symbols) || !softbuffers || !payloads || !res) {
    NR_CW_REFUSE("%s: NULL argument", who);
  }
  // ---- validation: nothing is enqueued and nothing of the caller's is written before every entry has passed
  std::vector<RxCw> cw(n);
  uint32_t          n_cb = 0, sb_stride = 0, data_stride = 0, n_seg_total = 0, n_prbs_total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const srsran_softbuffer_rx_t* sb = softbuffers[i];
    if ((!grids && !symbols[i]) || !sb || !payloads[i] || !sb->buffer_f || !sb->data || !sb->cb_crc) {
      NR_CW_REFUSE("%s: codeword %u: NULL symbols, soft buffer or payload", who, i);
    }
    if (grids) {
      if (const char* why = nr_map::invalid(grids[i])) {
        NR_CW_REFUSE("%s: codeword %u: %s", who, i, why);
      }
      if (grids[i].nof_prb != grids[0].nof_prb) {
        NR_CW_REFUSE("%s: codeword %u: nof_prb %u on a grid of %u", who, i, grids[i].nof_prb, grids[0].nof_prb);
      }
      const uint32_t nof_re = nr_map::nof_re(grids[i]);
      if (nof_re != g[i].nof_re) {
        NR_CW_REFUSE("%s: codeword %u: nof_re %u, the grant takes %u", who, i, g[i].nof_re, nof_re);
      }
      n_seg_total += nr_map::nof_seg(grids[i]);
      n_prbs_total += nr_map::granted_prbs(grids[i]);
    }
    TbCfg& c = cw[i].c;
    if (check_tb(who, i, g[i].tb, g[i].nof_re, &c) != SRSRAN_SUCCESS) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (sb->max_cb < c.C || sb->max_cb_size < c.N) { // sch_nr.c:556-559
      NR_CW_REFUSE("%s: codeword %u: soft buffer of %u rows x %u for %u code blocks of %u soft bits", who, i, sb->max_cb, sb->max_cb_size, c.C, c.N);
    }
    if (c.C > NrTbStage::MAX_CB - n_cb) {
      NR_CW_REFUSE("%s: codeword %u: more than %u code blocks in one call", who, i, NrTbStage::MAX_CB);
    }
    for (uint32_t r = 0; r < c.C; r++) {
      if (!sb->buffer_f[r] || !sb->data[r]) {
        NR_CW_REFUSE("%s: codeword %u: soft-buffer provided NULL buffer for cb_idx=%u", who, i, r); // sch_nr.c:571-574
      }
    }
    cw[i].first_cb = n_cb;
    n_cb += c.C;
    sb_stride   = std::max(sb_stride, (uint32_t)al256(c.N));
    data_stride = std::max(data_stride, (uint32_t)al256((c.Kr + 7) / 8));
  }
  NrTbStage& s = tb_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  // ---- layout
  const size_t o_soft = 0, o_data = al256(o_soft + (size_t)n_cb * sb_stride);
  size_t       o      = al256(o_data + (size_t)n_cb * data_stride);
  uint32_t     n_tiles = 0;
  const size_t o_in    = o;
  for (uint32_t i = 0; i < n; i++) {
    cw[i].o_sym = o;
    o           = al256(o + (size_t)g[i].nof_re * sizeof(cf_t));
    cw[i].o_ce  = o;
    if (grids || (ce && ce[i])) {
      o = al256(o + (size_t)g[i].nof_re * sizeof(cf_t));
    }
    n_tiles += modem::tiles_of(g[i].tb.mod, g[i].nof_re);
  }
  const size_t o_e = o;
  for (uint32_t i = 0; i < n; i++) {
    cw[i].o_e = o;
    o         = al256(o + g[i].tb.nof_bits);
  }
  const size_t e_bytes = o - o_e, o_pay = o;
  for (uint32_t i = 0; i < n; i++) {
    cw[i].o_pay = o;
    o           = al256(o + cw[i].c.A / 8 + 8);
  }
  const size_t        pay_bytes = o - o_pay;
  const JobListLayout jl        = job_list_layout(o, (size_t)n * sizeof(nrchan::FrontJob), n_tiles);
  o                             = jl.end;
  // grid calls: [grid | tables | granted PRBs | estimator jobs | de-mapper jobs] staged in the pinned image and uploaded in one copy, the records in the pinned
  // image (the estimator writes them there), the noise estimates in the device buffer
  const uint32_t grid_points = grids ? nr_map::NSYMB * 12 * grids[0].nof_prb : 0;
  const size_t   o_grid = al256(o), o_tab = al256(o_grid + (size_t)grid_points * sizeof(cf_t)), o_prbs = al256(o_tab + (size_t)n_seg_total * sizeof(nr_map::Seg));
  const size_t   o_ej = al256(o_prbs + (size_t)n_prbs_total * sizeof(uint16_t)), o_dj = al256(o_ej + (size_t)n * sizeof(nr_chest::EstJob));
  const size_t   o_rec = al256(o_dj + (size_t)n * sizeof(nr_chest::DemapJob)), o_noise = al256(o_rec + (size_t)n * sizeof(nr_chest::Record));
  if (grids) {
    o = al256(o_noise + (size_t)n * sizeof(float));
  }
  if (o - o_in > 0xffffffffull) {
    NR_CW_REFUSE("%s: %zu bytes of symbols and soft bits in one call", who, o - o_in);
  }
  if (!s.grow(o)) {
    return call::failed(who, "staging allocation failed");
  }
  JobList<nrchan::FrontJob> jobs(s.pin, jl.o_jobs, jl.o_tj);
  nrchan::FrontParams       fp;
  const uint32_t *          mp_x1 = nullptr, *mp_x2 = nullptr;
  {
    modem::Params mp;
    if (!modem::params_for(mp, modem::LLR_I8)) {
      return call::failed(who, get_error());
    }
    fp.in       = grids ? reinterpret_cast<const float2*>(s.dev + o_in) : reinterpret_cast<const float2*>(s.pin + o_in);
    fp.noise_dev = grids ? reinterpret_cast<const float*>(s.dev + o_noise) : nullptr;
    mp_x1 = mp.x1_bits, mp_x2 = mp.x2_cols;
    fp.out      = reinterpret_cast<int8_t*>(s.dev + o_e);
    fp.jobs     = jobs.jobs;
    fp.tile_job = jobs.tile_job;
    fp.n_tiles  = n_tiles;
    fp.x1_bits = mp.x1_bits, fp.x2_cols = mp.x2_cols, fp.k = mp.k;
  }
  uint8_t                         flags[NrTbStage::MAX_CB];
  std::vector<srsran_hip_nr_tb_t> tbs(n);
  nr_chest::Record*               rec = reinterpret_cast<nr_chest::Record*>(s.pin + o_rec);
  // Everything the call enqueues in front of its host wait (the last transport-block pass takes it).  nullptr, or the step that failed, its text the last
  // error: nothing more is enqueued then, and the ONE exit below waits for what was.
  auto enqueue = [&]() -> const char* {
    // ---- staging: symbols, estimates, job lists; rows and stored blocks of retransmissions
    for (uint32_t i = 0; i < n; i++) {
      RxCw&        w  = cw[i];
      const size_t nb = (size_t)g[i].nof_re * sizeof(cf_t);
      const bool   eq = grids || (ce && ce[i]);
      if (!grids) {
        memcpy(s.pin + w.o_sym, symbols[i], nb);
        if (eq) {
          memcpy(s.pin + w.o_ce, ce[i], nb);
        }
      }
      const uint32_t nt = modem::tiles_of(g[i].tb.mod, g[i].nof_re);
      jobs.jobs[i] = nrchan::FrontJob{g[i].tb.mod, g[i].nof_re, (uint32_t)((w.o_sym - o_in) / sizeof(cf_t)), eq ? (uint32_t)((w.o_ce - o_in) / sizeof(cf_t)) : NR_CHAN_NO_CE,
                                      (uint32_t)(w.o_e - o_e), g[i].seed, jobs.append(i, nt), nt, g[i].noise_estimate, g[i].noise_estimate > 0.f ? 1u : 0u};
      const hipError_t e = w.harq.stage_in(s, softbuffers[i], w.c, w.first_cb, o_soft, sb_stride, o_data, data_stride,
                                           (g[i].tb.rv & SRSRAN_HIP_NR_TB_NEW_DATA) != 0, flags); // (codeword 0: the call's first enqueue on s.st)
      if (e != hipSuccess) {
        set_error("%s", hipGetErrorString(e));
        return "soft buffer";
      }
      tbs[i]                = g[i].tb;
      tbs[i].rv             = (g[i].tb.rv & 3u) | (w.harq.fresh ? SRSRAN_HIP_NR_TB_NEW_DATA : 0u);
      tbs[i].e_offset       = (uint32_t)(w.o_e - o_e);
      tbs[i].payload_offset = (uint32_t)(w.o_pay - o_pay);
      tbs[i].first_cb       = w.first_cb;
    }
    // ---- one front-end launch over all codewords, one transport-block pass per (scaling factor, iterations)
    if (grids) { // the grid is staged once; every codeword has its own table and its own workgroup of the estimator
      memcpy(s.pin + o_grid, sf_symbols, (size_t)grid_points * sizeof(cf_t));
      nr_map::Seg*        tab  = reinterpret_cast<nr_map::Seg*>(s.pin + o_tab);
      uint16_t*           prbs = reinterpret_cast<uint16_t*>(s.pin + o_prbs);
      nr_chest::EstJob*   ej   = reinterpret_cast<nr_chest::EstJob*>(s.pin + o_ej);
      nr_chest::DemapJob* dj   = reinterpret_cast<nr_chest::DemapJob*>(s.pin + o_dj);
      uint32_t            t0 = 0, p0 = 0, max_seg = 0;
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t ns = nr_map::fill_table(grids[i], tab + t0);
        nr_chest::fill_job(grids[i], &ej[i], prbs + p0);
        ej[i].o_prb = p0, ej[i].o_tab = t0, ej[i].n_seg = ns, ej[i].o_ce = (uint32_t)((cw[i].o_ce - o_in) / sizeof(cf_t)), ej[i].nof_re = g[i].nof_re;
        dj[i]   = nr_chest::DemapJob{t0, ns, (uint32_t)((cw[i].o_sym - o_in) / sizeof(cf_t)), g[i].nof_re};
        max_seg = std::max(max_seg, ns);
        t0 += ns, p0 += ej[i].n_prbs;
      }
      // one upload of the grid, the tables and the jobs: every codeword's workgroups read them, the estimator's several times
      hipError_t                e      = hipMemcpyAsync(s.dev + o_grid, s.pin + o_grid, o_rec - o_grid, hipMemcpyHostToDevice, s.st);
      const float2*             d_grid = reinterpret_cast<const float2*>(s.dev + o_grid);
      const nr_map::Seg*        d_tab  = reinterpret_cast<const nr_map::Seg*>(s.dev + o_tab);
      const uint32_t            io_points = (uint32_t)((o_e - o_in) / sizeof(cf_t));
      nr_chest::DemapParams dp{d_grid, grid_points, reinterpret_cast<const nr_chest::DemapJob*>(s.dev + o_dj), n, max_seg, d_tab, n_seg_total,
                               reinterpret_cast<float2*>(s.dev + o_in), io_points};
      nr_chest::EstParams   ep{d_grid, grid_points, reinterpret_cast<const nr_chest::EstJob*>(s.dev + o_ej), reinterpret_cast<const uint16_t*>(s.dev + o_prbs), n_prbs_total,
                             d_tab, n_seg_total, reinterpret_cast<float2*>(s.dev + o_in), io_points, rec, reinterpret_cast<float*>(s.dev + o_noise), n, max_seg, mp_x1, mp_x2};
      if (e == hipSuccess) {
        e = nr_chest::launch_demap(dp, s.st);
      }
      if (e == hipSuccess) {
        e = nr_chest::launch_est(ep, s.st);
      }
      if (e != hipSuccess) {
        set_error("grid upload / nr_demap_kernel / nr_dmrs_est_kernel: %s", hipGetErrorString(e));
        return "estimator";
      }
    }
    if (const hipError_t e = nrchan::launch_front(fp, s.st); e != hipSuccess) {
      set_error("nr_front_kernel: %s", hipGetErrorString(e));
      return "front end";
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) {
      order[i] = i;
    }
    auto dec_key = [&](uint32_t i) {
      const float sc = std::isnormal(g[i].scaling_fctr) ? g[i].scaling_fctr : 0.8f; // sch_nr.c:275
      uint32_t    b;
      memcpy(&b, &sc, 4);
      return ((uint64_t)b << 32) | (g[i].max_nof_iter ? g[i].max_nof_iter : 10u);
    };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dec_key(a) < dec_key(b); });
    std::vector<srsran_hip_nr_tb_t>        gtb;
    std::vector<srsran_hip_nr_tb_result_t> gres;
    for (uint32_t i = 0; i < n;) {
      uint32_t e = i;
      gtb.clear();
      while (e < n && dec_key(order[e]) == dec_key(order[i])) {
        gtb.push_back(tbs[order[e]]);
        e++;
      }
      gres.assign(gtb.size(), srsran_hip_nr_tb_result_t{});
      const uint32_t       i0 = order[i];
      srsran_hip_sch_nr_t* h  = s.decoder(std::isnormal(g[i0].scaling_fctr) ? g[i0].scaling_fctr : 0.8f, g[i0].max_nof_iter ? g[i0].max_nof_iter : 10u);
      if (!h) {
        return "decoder object";
      }
      // the last pass carries the downloads in front of its host wait: stored code blocks, payloads, and the soft bits where they are asked for
      const TailCopy tail[3] = {{s.pin + o_data, s.dev + o_data, (size_t)n_cb * data_stride}, {s.pin + o_pay, s.dev + o_pay, pay_bytes},
                                {s.pin + o_e, s.dev + o_e, e_out ? e_bytes : 0}};
      if (sch_nr_decode(h, reinterpret_cast<const int8_t*>(s.dev + o_e), gtb.data(), (uint32_t)gtb.size(), reinterpret_cast<int8_t*>(s.dev + o_soft), sb_stride,
                        flags, s.dev + o_data, data_stride, s.dev + o_pay, gres.data(), s.st, tail, e == n ? 3 : 0) != SRSRAN_SUCCESS) {
        return "transport blocks";
      }
      for (uint32_t k = i; k < e; k++) {
        res[order[k]] = gres[k - i];
      }
      i = e;
    }
    return nullptr;
  };
  if (const char* what = enqueue()) {
    (void)call::settle(hipSuccess, s.st); // nothing of a failed call may still be in flight when the next one re-uses the images
    return failed_at(who, what);
  }
  // ---- the soft buffers' side of the results; the rows of the blocks that are still undecoded are the one enqueue behind that wait, and take one of their own
  hipError_t e         = hipSuccess;
  bool       rows_left = false;
  for (uint32_t i = 0; i < n && e == hipSuccess; i++) {
    e         = cw[i].harq.fetch(s, flags);
    rows_left = rows_left || cw[i].harq.first >= 0;
  }
  if (rows_left) {
    e = call::settle(e, s.st);
  }
  if (e != hipSuccess) {
    return call::device_failed(who, e);
  }
  for (uint32_t i = 0; i < n; i++) {
    const RxCw& w = cw[i];
    w.harq.finish(s);
    if (res[i].all_decoded) { // sch_nr.c:664-666: otherwise the payload is not touched
      memcpy(payloads[i], s.pin + w.o_pay, w.c.A / 8);
    }
    if (e_out && i == 0) {
      memcpy(e_out, s.pin + w.o_e, g[i].tb.nof_bits);
    }
    if (grids && chest) {
      nr_chest::finish(rec[i], g[i].nof_re, &chest[i]);
    }
  }
  return SRSRAN_SUCCESS;
}

int nr_cw_encode(uint32_t n, const srsran_hip_nr_cw_tx_t* g, const uint8_t* const* data, cf_t* const* symbols)
{
  static const char* who = "nr_cw_encode";
  TraceRange         trace_("srsran_hip_nr_cw_encode");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !data || !symbols) {
    NR_CW_REFUSE("%s: NULL argument", who);
  }
  std::vector<TbCfg> cfg(n);
  uint32_t           n_cb = 0, n_tiles = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!data[i] || !symbols[i]) {
      NR_CW_REFUSE("%s: codeword %u: NULL payload or symbols", who, i);
    }
    if (check_tb(who, i, g[i].tb, g[i].nof_re, &cfg[i]) != SRSRAN_SUCCESS) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (g[i].tb.rv > 3) {
      NR_CW_REFUSE("%s: codeword %u: rv %u", who, i, g[i].tb.rv);
    }
    if (cfg[i].C > NrTbStage::MAX_CB - n_cb) {
      NR_CW_REFUSE("%s: codeword %u: more than %u code blocks in one call", who, i, NrTbStage::MAX_CB);
    }
    n_cb += cfg[i].C;
    n_tiles += modem::tiles_of(g[i].tb.mod, g[i].nof_re);
  }
  NrTbStage& s = tb_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  srsran_hip_sch_nr_t* h = s.decoder(0.8f, 10); // (the transmit side has no decoder parameters: one object per thread)
  if (!h) {
    return SRSRAN_ERROR;
  }
  // layout: [payloads | coded bits (device) | symbols | job lists]
  std::vector<size_t> o_pay(n), o_e(n), o_sym(n);
  size_t              o = 0;
  for (uint32_t i = 0; i < n; i++) {
    o_pay[i] = o;
    o        = al256(o + cfg[i].A / 8 + 8);
  }
  const size_t e0 = o;
  for (uint32_t i = 0; i < n; i++) {
    o_e[i] = o;
    o      = al256(o + g[i].tb.nof_bits);
  }
  const size_t s0 = o;
  for (uint32_t i = 0; i < n; i++) {
    o_sym[i] = o;
    o        = al256(o + (size_t)g[i].nof_re * sizeof(cf_t));
  }
  const JobListLayout jl = job_list_layout(o, (size_t)n * sizeof(nrchan::ModJob), n_tiles);
  o                      = jl.end;
  if (o > 0xffffffffull) {
    NR_CW_REFUSE("%s: %zu bytes in one call", who, o);
  }
  modem::Params mp;
  const float2* tab = modem::mod_tables();
  if (!s.grow(o) || !modem::params_for(mp, modem::LLR_I8) || !tab) {
    return call::failed(who, get_error());
  }
  JobList<nrchan::ModJob>         jobs(s.pin, jl.o_jobs, jl.o_tj);
  std::vector<srsran_hip_nr_tb_t> tbs(n);
  for (uint32_t i = 0; i < n; i++) {
    memcpy(s.pin + o_pay[i], data[i], cfg[i].A / 8);
    tbs[i]                = g[i].tb;
    tbs[i].e_offset       = (uint32_t)(o_e[i] - e0);
    tbs[i].payload_offset = (uint32_t)o_pay[i];
    tbs[i].first_cb       = 0;
    const uint32_t nt     = modem::tiles_of(g[i].tb.mod, g[i].nof_re);
    const float    scale  = (g[i].scaling != 0.f && !std::isnan(g[i].scaling)) ? g[i].scaling : 1.0f;
    jobs.jobs[i] = nrchan::ModJob{g[i].tb.mod, g[i].nof_re, g[i].seed, scale, (uint32_t)(o_e[i] - e0), (uint32_t)((o_sym[i] - s0) / sizeof(cf_t)), jobs.append(i, nt), nt};
  }
  nrchan::ModParams p;
  p.bits = s.dev + e0, p.out = reinterpret_cast<float2*>(s.pin + s0), p.table = tab, p.jobs = jobs.jobs, p.tile_job = jobs.tile_job, p.n_tiles = n_tiles;
  p.x1_bits = mp.x1_bits, p.x2_cols = mp.x2_cols;
  // the coding kernels read the payloads from the pinned image; the rate matcher's bits stay on the device; the modulator writes the pinned image
  const char* what = nullptr; // the step that could not be enqueued, its text the last error
  if (srsran_hip_sch_nr_encode(h, s.pin, tbs.data(), n, s.dev + e0, s.st) != SRSRAN_SUCCESS) {
    what = "transport blocks";
  } else if (const hipError_t e = nrchan::launch_mod(p, s.st); e != hipSuccess) {
    set_error("nr_mod_kernel: %s", hipGetErrorString(e));
    what = "modulator";
  }
  const hipError_t w = call::settle(hipSuccess, s.st); // the call's one host wait, whether or not everything was enqueued
  if (what || w != hipSuccess) {
    return what ? failed_at(who, what) : call::device_failed(who, w);
  }
  for (uint32_t i = 0; i < n; i++) {
    memcpy(symbols[i], s.pin + o_sym[i], (size_t)g[i].nof_re * sizeof(cf_t));
  }
  return SRSRAN_SUCCESS;
}

} // namespace

extern "C" uint32_t srsran_hip_sequence_nr_seed(uint16_t rnti, uint32_t cw_idx, uint32_t n_id)
{
  return ((uint32_t)rnti << 15) + (cw_idx << 14) + n_id; // pdsch_nr.c:297, pusch_nr.c:346
}

extern "C" int srsran_hip_nr_cw_decode_multi(uint32_t n, const srsran_hip_nr_cw_rx_t* g, const cf_t* const* symbols, const cf_t* const* ce,
                                             srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* payloads, srsran_hip_nr_tb_result_t* res)
{
  return nr_cw_decode(n, g, symbols, ce, softbuffers, payloads, res, nullptr);
}

extern "C" int srsran_hip_nr_cw_decode_dbg(const srsran_hip_nr_cw_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                           uint8_t* payload, srsran_hip_nr_tb_result_t* res, int8_t* e_out)
{
  return nr_cw_decode(1, g, &symbols, &ce, &softbuffer, &payload, res, e_out);
}

extern "C" int srsran_hip_nr_cw_decode(const srsran_hip_nr_cw_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* payload, srsran_hip_nr_tb_result_t* res)
{
  return nr_cw_decode(1, g, &symbols, &ce, &softbuffer, &payload, res, nullptr);
}

extern "C" int srsran_hip_nr_cw_decode_grid_multi(uint32_t n, const srsran_hip_nr_cw_rx_t* g, const srsran_hip_nr_grid_t* grids, const cf_t* sf_symbols,
                                                  srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* payloads, srsran_hip_nr_tb_result_t* res,
                                                  srsran_hip_nr_chest_res_t* chest)
{
  if (n && !grids) {
    if (res) {
      memset(res, 0, (size_t)n * sizeof(*res));
    }
    if (chest) {
      memset(chest, 0, (size_t)n * sizeof(*chest));
    }
    fprintf(stderr, "[srsran_phy_hip] nr_cw_decode_grid: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return nr_cw_decode(n, g, nullptr, nullptr, softbuffers, payloads, res, nullptr, grids, sf_symbols, chest);
}

extern "C" int srsran_hip_nr_cw_decode_grid_dbg(const srsran_hip_nr_cw_rx_t* g, const srsran_hip_nr_grid_t* grid, const cf_t* sf_symbols,
                                                srsran_softbuffer_rx_t* softbuffer, uint8_t* payload, srsran_hip_nr_tb_result_t* res,
                                                srsran_hip_nr_chest_res_t* chest, int8_t* e_out)
{
  if (!grid) {
    return srsran_hip_nr_cw_decode_grid_multi(1, g, nullptr, sf_symbols, &softbuffer, &payload, res, chest);
  }
  return nr_cw_decode(1, g, nullptr, nullptr, &softbuffer, &payload, res, e_out, grid, sf_symbols, chest);
}

extern "C" int srsran_hip_nr_cw_decode_grid(const srsran_hip_nr_cw_rx_t* g, const srsran_hip_nr_grid_t* grid, const cf_t* sf_symbols,
                                            srsran_softbuffer_rx_t* softbuffer, uint8_t* payload, srsran_hip_nr_tb_result_t* res,
                                            srsran_hip_nr_chest_res_t* chest)
{
  return srsran_hip_nr_cw_decode_grid_dbg(g, grid, sf_symbols, softbuffer, payload, res, chest, nullptr);
}

extern "C" int srsran_hip_nr_cw_encode_multi(uint32_t n, const srsran_hip_nr_cw_tx_t* g, const uint8_t* const* data, cf_t* const* symbols)
{
  return nr_cw_encode(n, g, data, symbols);
}

extern "C" int srsran_hip_nr_cw_encode(const srsran_hip_nr_cw_tx_t* g, const uint8_t* data, cf_t* symbols)
{
  return nr_cw_encode(1, g, &data, &symbols);
}
