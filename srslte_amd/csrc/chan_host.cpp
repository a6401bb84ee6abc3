// chan_host.cpp -- one device call per grant (include/srsran_amd/phy_chan_abi.h): the stages between the resource grid and the transport
// block of srsran_pusch_decode (pusch.c:358-478), srsran_pdsch_decode / _encode (pdsch.c:662-760, 949-1015) and srsran_ulsch_encode
// (sch.c:1194) chained on the calling thread's transport-block stream, nothing but the inputs and the results crossing the bus.
#include "chan_device.h"
#include "chan_internal.h"
#include "chest_dl_device.h"
#include "chest_ul_device.h"
#include "csi_device.h"
#include "modem_device.h"
#include "pdsch_map_device.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace phyhip;
using namespace phyhip::chan;

ChanStage* phyhip::chan::stage_for(const char* who)
{
  static thread_local StageRef<ChanStage> r;
  if (!device_available()) {
    call::no_device(who);
    return nullptr;
  }
  bind_thread();
  return &r.get();
}

bool phyhip::chan::segment(srsran_cbsegm_t* seg, uint32_t tbs)
{
  if (srsran_cbsegm(seg, tbs) != SRSRAN_SUCCESS) {
    fprintf(stderr, "Error computing segmentation for TBS=%d\n", tbs); // sch.c:637-640, 1133-1136, 1224-1228
    return false;
  }
  return true;
}

bool phyhip::chan::tb_valid(const srsran_hip_grant_tb_t& tb, const char* who)
{
  if (tb.mod > SRSRAN_MOD_256QAM || tb.nl > 2 || tb.nof_re == 0 || tb.tbs == 0 || (tb.tbs & 7u) || tb.rv > 3 ||
      (uint64_t)tb.nof_re * qm_of(tb.mod) > SRSRAN_HIP_SEQUENCE_MAX_LEN) {
    refuse("%s: invalid grant (mod %u, %u REs, tbs %u, rv %u)", who, tb.mod, tb.nof_re, tb.tbs, tb.rv);
    return false;
  }
  return true;
}

bool phyhip::chan::enqueue_csi_weight(hipStream_t st, const CsiCodeword* cw, uint32_t n_cw, uint32_t nof_re, bool llr8)
{
  csi::WeightParams p = {};
  for (uint32_t k = 0; k < n_cw && k < 2; k++) {
    p.job[k] = {cw[k].d_e, cw[k].csi, cw[k].mod, nof_re};
  }
  p.n_jobs = n_cw;
  p.tile1  = (nof_re + CSI_TILE_SYMS - 1) / CSI_TILE_SYMS;
  if (csi::launch_weight(p, llr8, st) != hipSuccess) {
    set_error("grant front end: CSI weighting launch failed");
    return false;
  }
  return true;
}

bool phyhip::chan::csi_row_valid(const float* csi, uint32_t nof_re)
{
  for (uint32_t i = 0; i < nof_re; i++) {
    if (!(csi[i] >= 0.f) || !std::isfinite(csi[i])) {
      return false;
    }
  }
  return true;
}

namespace {

// the receive front end of one grant, enqueued on `st`: [equaliser] -> [transform de-precoding] -> demodulator + descrambler (+ UL channel
// de-interleaver in its store) -> d_e.  p_sym / p_ce: the grant's REs in the pinned image; d_x / d_z: device scratch of nof_re points each; d_csi: nullptr,
// or where the equaliser files its nof_re channel-state values.  d_eqj: nullptr, or the grant's equaliser job in DEVICE memory, which the channel estimator's
// kernel ahead on the stream fills with the noise estimate (`noise` is then not looked at; nof_re is even).
bool enqueue_rx_front(hipStream_t st, const srsran_hip_grant_tb_t& tb, const uint8_t* p_sym, const uint8_t* p_ce, float scaling, float noise, uint32_t L_prb,
                      uint32_t nof_symb, uint8_t* d_x, uint8_t* d_z, srsran_hip_dft_batch_t* plan, void* d_e, float* d_csi = nullptr,
                      const modem::EqJob* d_eqj = nullptr, const modem::NoiseAvg* dev_noise = nullptr)
{
  const uint8_t* cur = p_sym;
  if (p_ce) {
    if ((d_eqj ? modem::launch_eq_jobs(p_sym, p_ce, d_x, d_eqj, 1, tb.nof_re / 2, scaling, st)
               : modem::launch_eq(p_sym, p_ce, d_x, d_csi, tb.nof_re, scaling, noise, st, dev_noise)) !=
        hipSuccess) {
      set_error("grant front end: equaliser launch failed");
      return false;
    }
    cur = d_x;
  }
  if (L_prb) {
    if (srsran_hip_dft_batch_run(plan, (const cf_t*)cur, (cf_t*)d_z, nof_symb, st) != SRSRAN_SUCCESS) {
      return false;
    }
    cur = d_z;
  }
  modem::Params p;
  if (!modem::params_for(p, tb.llr_is_8bit ? modem::LLR_I8 : modem::LLR_I16)) {
    return false;
  }
  p.in      = cur;
  p.out     = d_e;
  p.single  = modem::Job{tb.mod, tb.nof_re, 0, 0, tb.seed, 1u, 0, modem::tiles_of(tb.mod, tb.nof_re), L_prb ? 12 * L_prb : 0u, L_prb ? nof_symb : 0u};
  p.n_jobs  = 1;
  p.n_tiles = p.single.ntiles;
  if (modem::launch(p, st) != hipSuccess) {
    set_error("grant front end: demodulator launch failed");
    return false;
  }
  return true;
}

// srsran_vec_avg_power_cf over n points (a measurement: plain left-to-right float sums, not the reference's SIMD order)
float avg_power(const float* x, size_t n)
{
  double acc = 0;
  for (size_t i = 0; i < 2 * n; i++) {
    acc += (double)x[i] * x[i];
  }
  return n ? (float)(acc / (double)n) : 0.f;
}

struct PuschPlan { // one grant of a (multi-)call
  uint32_t                nof_symb = 0;
  size_t                  o_sym = 0, o_ce = 0, o_x = 0, o_z = 0; // byte offsets in the pinned (symbols, estimates) and device (equalised, de-precoded) images
  srsran_cbsegm_t         seg;
  srsran_hip_sch_head_t   head;
  srsran_hip_dft_batch_t* plan = nullptr;
  sch::FrontEnd           front;
  size_t                  o_uci = 0; // the grant's control image in the pinned image (modem_device.h: uci_image_*)
  size_t                  o_refs = 0; // with an estimator: the grant's reference rows in the pinned image (stage_refs)
};

inline bool has_uci(const srsran_hip_pusch_uci_t& u)
{
  return (u.Q_prime_ack | u.Q_prime_ri | u.Q_prime_cqi) != 0;
}

// the geometry of a PUSCH allocation (what the channel estimator reads of a grant)
inline bool alloc_valid(const srsran_hip_pusch_rx_t& x)
{
  return (x.cp_nsymb == 7 || x.cp_nsymb == 6) && x.L_prb != 0 && srsran_dft_precoding_valid_prb(x.L_prb) && x.n_prb_tilde[0] + x.L_prb <= x.cell_nof_prb &&
         x.n_prb_tilde[1] + x.L_prb <= x.cell_nof_prb;
}

// the estimator's input of one grant into the pinned image at byte `at`: the two received reference rows (srsran_refsignal_dmrs_pusch_get,
// refsignal_ul.c:209-224: symbol (slot + 1) cp_nsymb - 4 of each slot), then the grant's DMRS row -- 4 n points.  Returns the job but for its output rows.
chest_ul::Job stage_refs(uint8_t* pin, size_t at, const srsran_hip_pusch_rx_t& x, const srsran_hip_chest_ul_t& e, const cf_t* grid)
{
  const uint32_t n = 12 * x.L_prb;
  for (uint32_t slot = 0; slot < 2; slot++) {
    const size_t idx = ((size_t)((slot + 1) * x.cp_nsymb - 4) * x.cell_nof_prb + x.n_prb_tilde[slot]) * 12;
    memcpy(pin + at + (size_t)slot * n * sizeof(cf_t), grid + idx, n * sizeof(cf_t));
  }
  memcpy(pin + at + (size_t)2 * n * sizeof(cf_t), e.r, (size_t)2 * n * sizeof(cf_t));
  chest_ul::Job j = {};
  j.n          = n;
  j.o_rx       = (uint32_t)(at / sizeof(cf_t));
  j.o_r        = j.o_rx + 2 * n;
  j.filter_len = e.filter_len;
  for (uint32_t i = 0; i < e.filter_len && i < 3; i++) {
    j.filter[i] = e.filter[i];
  }
  return j;
}

} // namespace

// ------------------------------------------------------------------------------------------------ PUSCH receive

// the grants of a call.  uci == nullptr: srsran_hip_pusch_decode{,_multi}; else uci[i] / out[i] are grant i's control-information counts and outputs
// (srsran_hip_pusch_decode_uci{,_multi}) and the 16-bit grants' demodulator launch is the de-multiplexing one (modem::launch_uci).
// est != nullptr: srsran_hip_pusch_decode_est{,_multi} -- there is no ce; est[i] describes grant i's channel estimator, whose kernel runs ahead of the equaliser
// and hands it the rows and the noise estimate on the device; est_out[i] <- its measurements.  Every refusal of those calls comes before the device is
// looked for, with one line on stderr.
static int pusch_decode_grants(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* const* sf_symbols, const cf_t* const* ce,
                               srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data, srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* out,
                               const srsran_hip_chest_ul_t* est = nullptr, srsran_hip_chest_ul_res_t* est_out = nullptr)
{
  TraceRange trace_("srsran_hip_pusch_decode");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !sf_symbols || (!ce && !est) || !softbuffers || !data || !res) {
    return est ? refuse("srsran_hip_pusch_decode_est: NULL argument") : SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = est ? nullptr : stage_for("srsran_hip_pusch_decode");
  if (!sp && !est) {
    return SRSRAN_ERROR;
  }
  std::vector<PuschPlan> pl(n);
  size_t                 pin_need = 0, dev_need = 0;
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_pusch_rx_t& x = g[i];
    res[i] = {0, 0.f, NAN};
    if (!tb_valid(x.tb, "srsran_hip_pusch_decode")) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (!sf_symbols[i] || (!est && !ce[i]) || !softbuffers[i] || !data[i]) {
      return est ? refuse("srsran_hip_pusch_decode_est: grant %u: NULL argument", i) : SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (est && chest_ul::invalid(&est[i])) {
      return refuse("srsran_hip_pusch_decode_est: grant %u: %s", i, chest_ul::invalid(&est[i]));
    }
    const uint32_t nsymb = 2 * (x.cp_nsymb - 1) - (x.shortened ? 1u : 0u);
    if (!alloc_valid(x) || x.tb.nof_re != nsymb * 12 * x.L_prb || x.tb.mod < SRSRAN_MOD_QPSK || x.tb.mod > SRSRAN_MOD_64QAM) {
      return refuse("srsran_hip_pusch_decode: grant %u: allocation (%u PRB at %u / %u of %u, %u REs, mod %u) is not a PUSCH allocation", i, x.L_prb, x.n_prb_tilde[0],
                    x.n_prb_tilde[1], x.cell_nof_prb, x.tb.nof_re, x.tb.mod);
    }
    if (uci && has_uci(uci[i])) {
      const srsran_hip_pusch_uci_t& u = uci[i];
      const srsran_hip_pusch_uci_out_t* o = out ? &out[i] : nullptr;
      const char* why = nullptr;
      if (x.tb.llr_is_8bit) {
        why = "control information is taken with 16-bit soft bits only";
      } else if (u.Q_prime_ack > 4 * 12 * x.L_prb || u.Q_prime_ri > 4 * 12 * x.L_prb) {
        why = "more ACK / RI symbols than four columns hold";
      } else if ((uint64_t)u.Q_prime_ri + u.Q_prime_cqi >= x.tb.nof_re) {
        why = "RI and CQI leave no symbol for the transport block";
      } else if (!o || (u.Q_prime_ack && (!o->ack_llr || !o->ack_c || !o->ack_pos)) || (u.Q_prime_ri && (!o->ri_llr || !o->ri_c || !o->ri_pos)) ||
                 (u.Q_prime_cqi && !o->cqi_llr)) {
        why = "no output for a non-zero count";
      }
      if (why) {
        return refuse("srsran_hip_pusch_decode_uci: grant %u (Q'ack %u, Q'ri %u, Q'cqi %u, %u PRB): %s", i, u.Q_prime_ack, u.Q_prime_ri, u.Q_prime_cqi, x.L_prb, why);
      }
    }
    PuschPlan& p = pl[i];
    p.nof_symb   = nsymb;
    if (!segment(&p.seg, x.tb.tbs)) {
      return SRSRAN_ERROR;
    }
  }
  if (est) {
    sp = stage_for("srsran_hip_pusch_decode_est");
    if (!sp) {
      return SRSRAN_ERROR;
    }
  }
  ChanStage& s = *sp;
  for (uint32_t i = 0; i < n; i++) {
    pl[i].plan = s.plan(g[i].L_prb);
    if (!pl[i].plan) {
      return SRSRAN_ERROR;
    }
  }
  // Layout: the grants' REs packed one behind the other, ordered by allocation size -- four arrays of the same shape (symbols and estimates in the pinned
  // image, equalised and de-precoded symbols on the device), so that ONE equaliser launch, one transform launch per allocation size and ONE demodulator
  // launch serve all grants of the call (a launch costs 4-5 us whatever it carries: 25 grants x 3 kernels were 330 of the call's 390 us).
  std::vector<uint32_t> ord(n);
  for (uint32_t i = 0; i < n; i++) {
    ord[i] = i;
  }
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return g[a].L_prb < g[b].L_prb; });
  size_t tot = 0, tiles = 0;
  for (uint32_t k = 0; k < n; k++) {
    PuschPlan& p = pl[ord[k]];
    p.o_sym = p.o_x = tot;
    tot += (size_t)g[ord[k]].tb.nof_re * sizeof(cf_t);
    tiles += modem::tiles_of(g[ord[k]].tb.mod, g[ord[k]].tb.nof_re);
  }
  const size_t region = al256(tot);
  for (uint32_t i = 0; i < n; i++) {
    pl[i].o_ce = (est ? 2 * region : region) + pl[i].o_sym; // (est: in the device image)
    pl[i].o_z  = region + pl[i].o_x;
  }
  // (with an estimator the estimates' region and the equaliser's job list are DEVICE memory behind the other two regions: the estimator's kernel writes both)
  const size_t        o_eqj = est ? region : 2 * region;
  const JobListLayout jl    = job_list_layout(al256(o_eqj + (est ? 0 : n * sizeof(modem::EqJob))), n * sizeof(modem::Job), tiles);
  pin_need = jl.end;
  dev_need = est ? 3 * region + al256(n * sizeof(modem::EqJob)) : 2 * region;
  // with control information: the de-multiplexing demodulator's job list behind the others, then every grant's control image (the kernel stores the
  // control soft bits and chips straight into the pinned image: they are there after the call's one host wait).  Its workgroups are listed in the
  // one tile table: a 16-bit grant of such a call is in this list, an 8-bit one in the other
  const size_t o_uj = pin_need;
  if (uci) {
    pin_need = job_list_layout(o_uj, n * sizeof(modem::UciJob), 0).end;
    for (uint32_t i = 0; i < n; i++) {
      pl[i].o_uci = pin_need;
      pin_need    = al256(pin_need + modem::uci_image_bytes(uci[i].Q_prime_ack, uci[i].Q_prime_ri, uci[i].Q_prime_cqi, qm_of(g[i].tb.mod)));
    }
  }
  // with an estimator: its job list, its records and every grant's four reference rows behind everything else
  const size_t o_cj = al256(pin_need), o_rec = al256(o_cj + (est ? n * sizeof(chest_ul::Job) : 0));
  if (est) {
    pin_need = al256(o_rec + n * sizeof(chest_ul::Record));
    for (uint32_t i = 0; i < n; i++) {
      pl[i].o_refs = pin_need;
      pin_need += (size_t)4 * 12 * g[i].L_prb * sizeof(cf_t);
    }
  }
  if (!s.grow(pin_need, dev_need)) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pusch_decode: staging allocation failed\n");
    return SRSRAN_ERROR;
  }
  // the estimator's launch: job k is the k-th grant of the layout, as the equaliser's; it stores the slot's row to every data symbol of the slot in the
  // layout the equaliser reads (pusch_get order) and the equaliser's job k -- end of the grant's run of symbol pairs, noise estimate -- next to it
  auto*      cjobs = reinterpret_cast<chest_ul::Job*>(s.pin + o_cj);
  const auto enqueue_chest = [&](hipStream_t st) {
    const chest_ul::Params cp = {reinterpret_cast<const float2*>(s.pin.get()), reinterpret_cast<float2*>(s.dev + 2 * region), cjobs,
                                 reinterpret_cast<chest_ul::Record*>(s.pin + o_rec), reinterpret_cast<modem::EqJob*>(s.dev + 3 * region), n,
                                 (uint32_t)(pin_need / sizeof(cf_t)), (uint32_t)(tot / sizeof(cf_t))};
    if (chest_ul::launch(cp, st) != hipSuccess) {
      set_error("grant front end: channel estimator launch failed");
      return false;
    }
    return true;
  };
  bool front_done = false; // the front end of the call has been enqueued
  std::vector<sch::TbItem> items(n);
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_pusch_rx_t& x = g[i];
    PuschPlan&                   p = pl[i];
    // pusch.c:48-104 (pusch_get): the allocation's 12 L_prb sub-carriers of every symbol but the slot's reference symbol (and the SRS symbol)
    const uint32_t L_ref = x.cp_nsymb == 7 ? 3 : 2;
    const size_t   wid   = (size_t)x.L_prb * 12 * sizeof(cf_t);
    size_t         at    = 0;
    for (uint32_t slot = 0; slot < 2; slot++) {
      const uint32_t nl = x.cp_nsymb - ((x.shortened && slot == 1) ? 1u : 0u);
      for (uint32_t l = 0; l < nl; l++) {
        if (l == L_ref) {
          continue;
        }
        const size_t idx = ((size_t)(l + slot * x.cp_nsymb) * x.cell_nof_prb + x.n_prb_tilde[slot]) * 12;
        memcpy(s.pin + p.o_sym + at, sf_symbols[i] + idx, wid);
        if (!est) {
          memcpy(s.pin + p.o_ce + at, ce[i] + idx, wid);
        }
        at += wid;
      }
    }
    if (x.meas_epre) {
      res[i].epre = avg_power(reinterpret_cast<const float*>(s.pin + p.o_sym), x.tb.nof_re); // pusch.c:397-401
    }
    p.head = {x.tb.max_nof_iterations, 0.f, x.tb.llr_is_8bit != 0};
    const srsran_hip_grant_tb_t tb = x.tb;
    const uint8_t *psym = s.pin + p.o_sym, *pce = est ? nullptr : s.pin + p.o_ce;
    uint8_t *      dx = s.dev + p.o_x, *dz = s.dev + p.o_z;
    const float    noise = x.noise_estimate;
    const uint32_t L_prb = x.L_prb, nsymb = p.nof_symb;
    auto*          plan  = p.plan;
    if (est) { // the estimator's launch ahead, and the equaliser takes its rows and its noise estimate from the device image (pce is not looked at)
      const uint8_t*      dh  = s.dev + p.o_ce;
      const modem::EqJob* eqj = reinterpret_cast<const modem::EqJob*>(s.dev + 3 * region);
      p.front = [=, &enqueue_chest, &front_done](hipStream_t st, void* d_e) {
        front_done = true;
        return enqueue_chest(st) && enqueue_rx_front(st, tb, psym, dh, 1.0f, 0.f, L_prb, nsymb, dx, dz, plan, d_e, nullptr, eqj);
      };
    } else {
      p.front = [=](hipStream_t st, void* d_e) { return enqueue_rx_front(st, tb, psym, pce, 1.0f, noise, L_prb, nsymb, dx, dz, plan, d_e); };
    }
    // (with control information the transport block's e bits are what RI and CQI leave: G = H' - Q'ri - Q'cqi symbols, sch.c:1184-1190)
    const uint32_t G = uci ? x.tb.nof_re - uci[i].Q_prime_ri - uci[i].Q_prime_cqi : x.tb.nof_re;
    items[i] = {&p.head, softbuffers[i], &p.seg, qm_rm(x.tb), x.tb.rv, G * qm_of(x.tb.mod), nullptr, &p.front, data[i], false};
  }
  if (uci) { // a grant that does not reach the launch (sch_host.cpp refuses its soft buffer) leaves zeros
    memset(s.pin + pl[0].o_uci, 0, (est ? o_cj : pin_need) - pl[0].o_uci);
  }
  for (uint32_t k = 0; est && k < n; k++) {
    const srsran_hip_pusch_rx_t& x = g[ord[k]];
    chest_ul::Job&               j = cjobs[k];
    j          = stage_refs(s.pin, pl[ord[k]].o_refs, x, est[ord[k]], sf_symbols[ord[k]]);
    j.o_out    = (uint32_t)(pl[ord[k]].o_sym / sizeof(cf_t));
    j.row0[1]  = x.cp_nsymb - 1;
    j.rows[0]  = x.cp_nsymb - 1;
    j.rows[1]  = x.cp_nsymb - 1 - (x.shortened ? 1u : 0u);
    j.end_pair = (uint32_t)((pl[ord[k]].o_sym + (size_t)x.tb.nof_re * sizeof(cf_t)) / (2 * sizeof(cf_t)));
  }
  // the front end of all grants at once (n > 1 or control information)
  size_t                   job_cur = 0, tile_cur = 0;
  const sch::GroupFrontEnd group   = [&](hipStream_t st, const uint32_t* which, void* const* d_e, uint32_t m) -> bool {
    if (!front_done) {
      auto*          ej = reinterpret_cast<modem::EqJob*>(est ? s.dev + 3 * region : s.pin + o_eqj);
      const uint8_t* h  = est ? s.dev + 2 * region : s.pin + region;
      if (est && !enqueue_chest(st)) {
        return false;
      }
      for (uint32_t k = 0; !est && k < n; k++) {
        const srsran_hip_pusch_rx_t& x = g[ord[k]];
        ej[k] = {(uint32_t)((pl[ord[k]].o_sym + (size_t)x.tb.nof_re * sizeof(cf_t)) / (2 * sizeof(cf_t))), x.noise_estimate, x.noise_estimate > 0.f ? 1u : 0u};
      }
      if (modem::launch_eq_jobs(s.pin, h, s.dev, ej, n, (uint32_t)(tot / (2 * sizeof(cf_t))), 1.0f, st) != hipSuccess) {
        set_error("grant front end: equaliser launch failed");
        return false;
      }
      for (uint32_t k = 0; k < n;) { // one transform launch per run of grants of one allocation size
        uint32_t e = k, symb = 0;
        while (e < n && g[ord[e]].L_prb == g[ord[k]].L_prb) {
          symb += pl[ord[e]].nof_symb;
          e++;
        }
        const PuschPlan& p0 = pl[ord[k]];
        if (srsran_hip_dft_batch_run(p0.plan, (const cf_t*)(s.dev + p0.o_x), (cf_t*)(s.dev + p0.o_z), symb, st) != SRSRAN_SUCCESS) {
          return false;
        }
        k = e;
      }
      front_done = true;
    }
    const bool    llr8 = g[which[0]].tb.llr_is_8bit != 0;
    const size_t  es   = llr8 ? 1 : 2;
    modem::Params p;
    if (!modem::params_for(p, llr8 ? modem::LLR_I8 : modem::LLR_I16)) {
      return false;
    }
    uint8_t* base = static_cast<uint8_t*>(d_e[0]);
    for (uint32_t k = 1; k < m; k++) {
      base = static_cast<uint8_t*>(d_e[k]) < base ? static_cast<uint8_t*>(d_e[k]) : base;
    }
    // (a call's launches share the two arrays: each lists its jobs and workgroups behind those of the launches before it)
    const size_t o_tiles = jl.o_tj + tile_cur * sizeof(uint32_t);
    if (uci && !llr8) { // the 16-bit grants of the call, with and without control information, in one de-multiplexing demodulator launch
      JobList<modem::UciJob> jobs(s.pin, o_uj + job_cur * sizeof(modem::UciJob), o_tiles);
      for (uint32_t k = 0; k < m; k++) {
        const uint32_t               i   = which[k];
        const srsran_hip_pusch_rx_t& x   = g[i];
        const uint32_t               cnt = modem::tiles_of(x.tb.mod, x.tb.nof_re);
        jobs.jobs[k] = modem::UciJob{x.tb.mod, x.tb.nof_re, (uint32_t)(pl[i].o_x / sizeof(cf_t)), (uint32_t)((size_t)(static_cast<uint8_t*>(d_e[k]) - base) / es), x.tb.seed,
                                     jobs.append(k, cnt), cnt, 12 * x.L_prb, pl[i].nof_symb, uci[i].Q_prime_ack, uci[i].Q_prime_ri, uci[i].Q_prime_cqi, (uint32_t)pl[i].o_uci};
      }
      job_cur += m;
      tile_cur += jobs.n_tiles;
      modem::UciParams up = {s.dev + region, base, s.pin, jobs.jobs, jobs.tile_job, jobs.n_tiles, p.x1_bits, p.x2_cols, p.k};
      if (modem::launch_uci(up, st) != hipSuccess) {
        set_error("grant front end: demodulator launch failed");
        return false;
      }
      return true;
    }
    JobList<modem::Job> jobs(s.pin, jl.o_jobs + job_cur * sizeof(modem::Job), o_tiles);
    for (uint32_t k = 0; k < m; k++) {
      const srsran_hip_pusch_rx_t& x   = g[which[k]];
      const uint32_t               cnt = modem::tiles_of(x.tb.mod, x.tb.nof_re);
      jobs.jobs[k] = modem::Job{x.tb.mod, x.tb.nof_re, (uint32_t)(pl[which[k]].o_x / sizeof(cf_t)), (uint32_t)((size_t)(static_cast<uint8_t*>(d_e[k]) - base) / es), x.tb.seed, 1u,
                                jobs.append(k, cnt), cnt, 12 * x.L_prb, pl[which[k]].nof_symb};
    }
    job_cur += m;
    tile_cur += jobs.n_tiles;
    p.in       = s.dev + region;
    p.out      = base;
    p.jobs     = jobs.jobs;
    p.tile_job = jobs.tile_job;
    p.n_jobs   = m;
    p.n_tiles  = jobs.n_tiles;
    if (modem::launch(p, st) != hipSuccess) {
      set_error("grant front end: demodulator launch failed");
      return false;
    }
    return true;
  };
  const bool device_ok = sch::decode_tbs_staged(items.data(), n, (n > 1 || uci) ? &group : nullptr);
  for (uint32_t i = 0; i < n; i++) {
    res[i].crc_ok               = items[i].ok ? 1 : 0;
    res[i].avg_iterations_block = pl[i].head.avg_iterations;
  }
  if (!device_ok) { // not a CRC failure: the caller must not take it for a NACK
    return SRSRAN_ERROR;
  }
  if (est) {
    if (!front_done) { // no grant reached the launch (sch_host.cpp dropped every soft buffer): the measurements are still the call's
      hipStream_t st = sch::stage_stream();
      if (!st || !enqueue_chest(st) || hipStreamSynchronize(st) != hipSuccess) {
        return SRSRAN_ERROR;
      }
    }
    const auto* rec = reinterpret_cast<const chest_ul::Record*>(s.pin + o_rec);
    for (uint32_t k = 0; k < n; k++) {
      chest_ul::finish(rec[k], est[ord[k]].meas_ta_en != 0, &est_out[ord[k]]);
    }
  }
  for (uint32_t i = 0; uci && i < n; i++) {
    const srsran_hip_pusch_uci_t& u = uci[i];
    if (!has_uci(u)) {
      continue;
    }
    // the control image -> the caller's arrays; the positions are the closed form of uci.c:364-416
    const uint32_t Qm = qm_of(g[i].tb.mod), rows = 12 * g[i].L_prb;
    const bool     normal = pl[i].nof_symb > 10;
    const int16_t* llr = reinterpret_cast<const int16_t*>(s.pin + pl[i].o_uci);
    const uint8_t* chips = s.pin + pl[i].o_uci + modem::uci_image_chips(u.Q_prime_ack, u.Q_prime_ri, u.Q_prime_cqi, Qm);
    static const uint32_t ack_cols[2][4] = {{1, 2, 6, 7}, {2, 3, 8, 9}}, ri_cols[2][4] = {{0, 3, 5, 8}, {1, 4, 7, 10}};
    const size_t na = (size_t)u.Q_prime_ack * Qm, nr = (size_t)u.Q_prime_ri * Qm, nc = (size_t)u.Q_prime_cqi * Qm;
    if (na) {
      memcpy(out[i].ack_llr, llr, na * sizeof(int16_t));
      memcpy(out[i].ack_c, chips, na);
    }
    if (nr) {
      memcpy(out[i].ri_llr, llr + na, nr * sizeof(int16_t));
      memcpy(out[i].ri_c, chips + na, nr);
    }
    if (nc) {
      memcpy(out[i].cqi_llr, llr + na + nr, nc * sizeof(int16_t));
    }
    for (uint32_t k = 0; k < u.Q_prime_ack; k++) {
      for (uint32_t b = 0; b < Qm; b++) {
        out[i].ack_pos[k * Qm + b] = (rows - 1 - k / 4) * Qm + rows * ack_cols[normal][(3 * k) % 4] * Qm + b;
      }
    }
    for (uint32_t k = 0; k < u.Q_prime_ri; k++) {
      for (uint32_t b = 0; b < Qm; b++) {
        out[i].ri_pos[k * Qm + b] = (rows - 1 - k / 4) * Qm + rows * ri_cols[normal][(3 * k) % 4] * Qm + b;
      }
    }
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_pusch_decode_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const cf_t* const* sf_symbols, const cf_t* const* ce,
                                             srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data, srsran_hip_grant_res_t* res)
{
  return pusch_decode_grants(n, g, nullptr, sf_symbols, ce, softbuffers, data, res, nullptr);
}

extern "C" int srsran_hip_pusch_decode_uci_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* const* sf_symbols,
                                                 const cf_t* const* ce, srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data,
                                                 srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* out)
{
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !uci || !res) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  bool any = false;
  for (uint32_t i = 0; i < n; i++) {
    res[i] = {0, 0.f, NAN}; // every result, before anything is checked
    any    = any || has_uci(uci[i]);
  }
  // no control information anywhere: the call IS srsran_hip_pusch_decode_multi
  return pusch_decode_grants(n, g, any ? uci : nullptr, sf_symbols, ce, softbuffers, data, res, out);
}

extern "C" int srsran_hip_pusch_decode_uci(const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* sf_symbols, const cf_t* ce,
                                           srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_pusch_uci_out_t* out)
{
  return srsran_hip_pusch_decode_uci_multi(1, g, uci, &sf_symbols, &ce, &softbuffer, &data, res, out);
}

extern "C" int srsran_hip_pusch_decode(const srsran_hip_pusch_rx_t* g, const cf_t* sf_symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* data, srsran_hip_grant_res_t* res)
{
  return srsran_hip_pusch_decode_multi(1, g, &sf_symbols, &ce, &softbuffer, &data, res);
}

// ------------------------------------------------------------------------------------------------ PUSCH channel estimation

extern "C" int srsran_hip_pusch_decode_est_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const srsran_hip_pusch_uci_t* uci,
                                                 const cf_t* const* sf_symbols, srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data,
                                                 srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* uci_out, srsran_hip_chest_ul_res_t* est_out)
{
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  bool any = false;
  for (uint32_t i = 0; i < n; i++) { // every result, before anything is checked
    if (res) {
      res[i] = {0, 0.f, NAN};
    }
    if (est_out) {
      est_out[i] = {};
    }
    any = any || (uci && has_uci(uci[i]));
  }
  if (!g || !est || !res || !est_out) {
    return refuse("srsran_hip_pusch_decode_est: NULL argument");
  }
  return pusch_decode_grants(n, g, any ? uci : nullptr, sf_symbols, nullptr, softbuffers, data, res, uci_out, est, est_out);
}

extern "C" int srsran_hip_pusch_decode_est(const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const srsran_hip_pusch_uci_t* uci,
                                           const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res,
                                           srsran_hip_pusch_uci_out_t* uci_out, srsran_hip_chest_ul_res_t* est_out)
{
  return srsran_hip_pusch_decode_est_multi(1, g, est, uci, &sf_symbols, &softbuffer, &data, res, uci_out, est_out);
}

// the stage by itself: the kernel's rows come down in the pinned image, one per slot, and are copied to the grant's columns of every symbol of the slot
extern "C" int srsran_hip_chest_ul_estimate_pusch_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est,
                                                        const cf_t* const* sf_symbols, cf_t* const* ce, srsran_hip_chest_ul_res_t* out)
{
  static const char* who = "srsran_hip_chest_ul_estimate_pusch";
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  for (uint32_t i = 0; out && i < n; i++) {
    out[i] = {};
  }
  if (!g || !est || !sf_symbols || !out) {
    return refuse("%s: NULL argument", who);
  }
  size_t points = 0;
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_pusch_rx_t& x = g[i];
    if (!sf_symbols[i] || chest_ul::invalid(&est[i])) {
      return refuse("%s: grant %u: %s", who, i, sf_symbols[i] ? chest_ul::invalid(&est[i]) : "NULL sf_symbols");
    }
    if (!alloc_valid(x)) {
      return refuse("%s: grant %u: allocation (%u PRB at %u / %u of %u, %u symbols per slot) is not a PUSCH allocation", who, i, x.L_prb, x.n_prb_tilde[0],
                    x.n_prb_tilde[1], x.cell_nof_prb, x.cp_nsymb);
    }
    points += (size_t)12 * x.L_prb;
  }
  ChanStage*  s  = stage_for(who);
  hipStream_t st = s ? sch::stage_stream() : nullptr;
  // pinned: every grant's four input rows, every grant's two output rows, the jobs, the records
  const size_t o_out = al256(4 * points * sizeof(cf_t)), o_cj = al256(o_out + 2 * points * sizeof(cf_t)), o_rec = al256(o_cj + n * sizeof(chest_ul::Job));
  const size_t need  = o_rec + n * sizeof(chest_ul::Record);
  if (!st || !s->grow(need, 0)) {
    return SRSRAN_ERROR;
  }
  auto*  jobs = reinterpret_cast<chest_ul::Job*>(s->pin + o_cj);
  size_t at   = 0;
  for (uint32_t i = 0; i < n; i++) {
    jobs[i]         = stage_refs(s->pin, 4 * at * sizeof(cf_t), g[i], est[i], sf_symbols[i]);
    jobs[i].o_out   = (uint32_t)(2 * at);
    jobs[i].row0[1] = 1;
    jobs[i].rows[0] = jobs[i].rows[1] = 1;
    at += (size_t)12 * g[i].L_prb;
  }
  const auto*            rec = reinterpret_cast<const chest_ul::Record*>(s->pin + o_rec);
  const chest_ul::Params cp  = {reinterpret_cast<const float2*>(s->pin.get()), reinterpret_cast<float2*>(s->pin + o_out), jobs,
                                reinterpret_cast<chest_ul::Record*>(s->pin + o_rec), nullptr, n, (uint32_t)(4 * points), (uint32_t)(2 * points)};
  if (call::settle(chest_ul::launch(cp, st), st) != hipSuccess) {
    set_error("%s: channel estimator launch failed", who);
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_pusch_rx_t& x   = g[i];
    const size_t                 wid = (size_t)12 * x.L_prb * sizeof(cf_t);
    for (uint32_t l = 0; ce && ce[i] && l < 2 * x.cp_nsymb; l++) {
      const uint32_t slot = l / x.cp_nsymb;
      memcpy(ce[i] + ((size_t)l * x.cell_nof_prb + x.n_prb_tilde[slot]) * 12, s->pin + o_out + (size_t)jobs[i].o_out * sizeof(cf_t) + slot * wid, wid);
    }
    chest_ul::finish(rec[i], est[i].meas_ta_en != 0, &out[i]);
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_chest_ul_estimate_pusch(const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const cf_t* sf_symbols, cf_t* ce,
                                                  srsran_hip_chest_ul_res_t* out)
{
  return srsran_hip_chest_ul_estimate_pusch_multi(1, g, est, &sf_symbols, &ce, out);
}

// ------------------------------------------------------------------------------------------------ PDSCH receive, one codeword

// weight: the _csi forms (cfg->csi_enable).  ce != NULL: the equaliser files its channel-state values in device scratch; ce == NULL: the caller's row goes
// up in the pinned image with the symbols, and `symbols` are the equalised symbols already (no d is made).
// map: the _sf forms -- symbols and ce are grids.
static int pdsch_decode_one(const char* who, bool weight, const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, const float* csi,
                            srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out, float* csi_out,
                            const SfMap* map = nullptr, EstMap* est = nullptr)
{
  TraceRange trace_("srsran_hip_pdsch_decode");
  if (!g || !symbols || !softbuffer || !data || !res) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  *res = {0, 0.f, NAN};
  const bool eq = ce != nullptr || est != nullptr; // est: the estimates are made on the device (the _est calls)
  if (!tb_valid(g->tb, who) || (eq && !(g->scaling != 0.f))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (weight && eq == (csi != nullptr)) {
    return refuse("%s: %s", who, eq ? "the equaliser makes the CSI of a grant with channel estimates: csi must be NULL" : "a grant without channel estimates needs the caller's csi");
  }
  if (weight && csi && !csi_row_valid(csi, g->tb.nof_re)) {
    return refuse("%s: a csi entry is negative or not finite", who);
  }
  if (map && !sf_valid(who, map->sf, 1, g->tb.nof_re)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (est && !est_valid(who, est, map ? map->sf : nullptr, 1)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  cf_t *const  y[1] = {const_cast<cf_t*>(symbols)}, *const h[1] = {const_cast<cf_t*>(ce)};
  const size_t nd   = (size_t)g->tb.nof_re * sizeof(cf_t);
  PlaneGroup   in[2] = {{y, 1, nd, true, false}, {est ? nullptr : h, eq ? 1u : 0u, nd, true, false}};
  RxGrant      gr = {who, in, 2, map, csi, {{&g->tb, qm_rm(g->tb), softbuffer, data, res, d_out, e_out, csi_out}}, 1, eq ? 1u : 0u, eq, weight, est};
  // (the _est calls: get_noise() of this subframe's estimates, averaged on the device, or 0 for zero forcing; the caller's noise_estimate is not read)
  const bool dev_noise = est && !est->cfg->decoder_zf;
  return pdsch_decode_grant(gr, [&](hipStream_t st, void* const* d_e, float* const* row, uint8_t* d_d) {
    if (!est) {
      return enqueue_rx_front(st, g->tb, reinterpret_cast<uint8_t*>(in[0].pin[0]), reinterpret_cast<uint8_t*>(in[1].pin[0]), g->scaling, g->noise_estimate, 0, 0, d_d, nullptr,
                              nullptr, d_e[0], eq ? row[0] : nullptr);
    }
    return enqueue_rx_front(st, g->tb, reinterpret_cast<uint8_t*>(in[0].pin[0]), reinterpret_cast<uint8_t*>(in[1].pin[0]), g->scaling, 0.f, 0, 0, d_d, nullptr, nullptr,
                            d_e[0], row[0], nullptr, dev_noise ? &est->noise : nullptr);
  });
}

extern "C" int srsran_hip_pdsch_decode(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* data, srsran_hip_grant_res_t* res)
{
  return pdsch_decode_one("srsran_hip_pdsch_decode", false, g, symbols, ce, nullptr, softbuffer, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_dbg(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                           uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out)
{
  return pdsch_decode_one("srsran_hip_pdsch_decode", false, g, symbols, ce, nullptr, softbuffer, data, res, d_out, e_out, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_csi(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, const float* csi,
                                           srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res)
{
  return pdsch_decode_one("srsran_hip_pdsch_decode_csi", true, g, symbols, ce, csi, softbuffer, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_csi_dbg(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, const float* csi,
                                               srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                               float* csi_out)
{
  return pdsch_decode_one("srsran_hip_pdsch_decode_csi", true, g, symbols, ce, csi, softbuffer, data, res, d_out, e_out, csi_out);
}

// ------------------------------------------------------------------------------------------------ PDSCH receive from the subframe grids

bool phyhip::chan::sf_valid(const char* who, const srsran_hip_pdsch_sf_t* sf, uint32_t ports, uint32_t nof_re)
{
  const char* why = !sf ? "NULL sf" : pdsch_map::invalid(*sf);
  if (!why && sf->cell_nof_ports != ports) {
    why = "cell_nof_ports is not the call's";
  }
  if (why) {
    refuse("%s: subframe description: %s", who, why);
    return false;
  }
  const uint32_t n = pdsch_map::nof_re(*sf);
  if (n != nof_re) {
    refuse("%s: expecting %u symbols but got %u", who, nof_re, n); // pdsch.c:834
    return false;
  }
  return true;
}

extern "C" int srsran_hip_pdsch_nof_re(const srsran_hip_pdsch_sf_t* sf)
{
  return (!sf || pdsch_map::invalid(*sf)) ? -1 : (int)pdsch_map::nof_re(*sf);
}

extern "C" int srsran_hip_pdsch_get(const srsran_hip_pdsch_sf_t* sf, uint32_t n_planes, const cf_t* const* grids, cf_t* const* symbols)
{
  static const char* who = "srsran_hip_pdsch_get";
  const char*        why = !sf ? "NULL sf" : pdsch_map::invalid(*sf);
  why                    = why ? why : (!grids || !symbols || n_planes > 65535u) ? "NULL argument or more than 65535 planes" : nullptr;
  for (uint32_t i = 0; !why && i < n_planes; i++) {
    why = (grids[i] && symbols[i]) ? nullptr : "a NULL plane";
  }
  if (why) {
    refuse("%s: %s", who, why);
    return -1;
  }
  const pdsch_map::Window w = pdsch_map::window(*sf);
  if (w.nof_re == 0 || n_planes == 0) {
    return (int)w.nof_re;
  }
  ChanStage*  s  = stage_for(who);
  hipStream_t st = s ? sch::stage_stream() : nullptr;
  // pinned: the staged rows of every grid, the table, the planes
  const size_t sb = al256((size_t)w.staged_points() * sizeof(cf_t)), nd = (size_t)w.nof_re * sizeof(cf_t), nb = al256(nd);
  const size_t o_tab = n_planes * sb, o_out = o_tab + al256(w.n_seg * sizeof(pdsch_map::Seg));
  if (!st || !s->grow(o_out + n_planes * nb, 0)) {
    return -1;
  }
  for (uint32_t i = 0; i < n_planes; i++) {
    stage_grid(s->pin + i * sb, grids[i], *sf, w);
  }
  pdsch_map::fill_table(*sf, w, reinterpret_cast<pdsch_map::Seg*>(s->pin + o_tab));
  const pdsch_map::DemapParams dp = {reinterpret_cast<const float2*>(s->pin.get()), reinterpret_cast<float2*>(s->pin + o_out), reinterpret_cast<const pdsch_map::Seg*>(s->pin + o_tab),
                                     w.n_seg, n_planes, (uint32_t)(sb / sizeof(cf_t)), w.staged_points(), (uint32_t)(nb / sizeof(cf_t)), w.nof_re};
  if (call::settle(pdsch_map::launch_demap(dp, st), st) != hipSuccess) {
    return -1;
  }
  for (uint32_t i = 0; i < n_planes; i++) {
    memcpy(symbols[i], s->pin + o_out + i * nb, nd);
  }
  return (int)w.nof_re;
}

// the one-port call: a line on stderr for every refusal, then the twin's path with the grids in the planes' place
static int pdsch_decode_one_sf(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const cf_t* sf_symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                               uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out, float* csi_out, cf_t* sym_out, cf_t* ce_out)
{
  static const char* who = "srsran_hip_pdsch_decode_sf";
  if (res) {
    *res = {0, 0.f, NAN};
  }
  if (!g || !sf || !sf_symbols || !ce || !softbuffer || !data || !res) {
    return refuse("%s: NULL argument (the call needs the estimates' grid: there is no grid of equalised symbols)", who);
  }
  if (!(g->scaling != 0.f)) {
    return refuse("%s: scaling is 0", who);
  }
  const SfMap map    = {sf, {sym_out, ce_out}};
  const bool  weight = sf->csi_enable != 0;
  return pdsch_decode_one(who, weight, g, sf_symbols, ce, nullptr, softbuffer, data, res, d_out, e_out, weight ? csi_out : nullptr, &map);
}

extern "C" int srsran_hip_pdsch_decode_sf(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const cf_t* sf_symbols, const cf_t* ce,
                                          srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res)
{
  return pdsch_decode_one_sf(g, sf, sf_symbols, ce, softbuffer, data, res, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_sf_dbg(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const cf_t* sf_symbols, const cf_t* ce,
                                              srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                              float* csi_out, cf_t* sym_out, cf_t* ce_out)
{
  return pdsch_decode_one_sf(g, sf, sf_symbols, ce, softbuffer, data, res, d_out, e_out, csi_out, sym_out, ce_out);
}

// the one-port call from the grids alone: the _sf call's path with the estimator's kernel in front (chest_dl_kernels.hip)
static int pdsch_decode_one_est(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
                                const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out,
                                cf_t* d_out, void* e_out, float* csi_out, cf_t* sym_out, cf_t* ce_out, cf_t* ce_grid_out)
{
  static const char* who = "srsran_hip_pdsch_decode_est";
  if (res) {
    *res = {0, 0.f, NAN};
  }
  if (est_out) {
    *est_out = {};
  }
  if (!g || !sf || !est || !state_in || !sf_symbols || !softbuffer || !data || !res || !est_out) {
    return refuse("%s: NULL argument", who);
  }
  if (!(g->scaling != 0.f)) {
    return refuse("%s: scaling is 0", who);
  }
  const SfMap map    = {sf, {sym_out, ce_out}};
  EstMap      em     = {est, state_in, est_out, {{ce_grid_out}}, {}};
  const bool  weight = sf->csi_enable != 0;
  return pdsch_decode_one(who, weight, g, sf_symbols, nullptr, nullptr, softbuffer, data, res, d_out, e_out, weight ? csi_out : nullptr, &map, &em);
}

extern "C" int srsran_hip_pdsch_decode_est(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                           const srsran_hip_chest_dl_state_t* state_in, const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                           srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out)
{
  return pdsch_decode_one_est(g, sf, est, state_in, sf_symbols, softbuffer, data, res, est_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_est_dbg(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                               const srsran_hip_chest_dl_state_t* state_in, const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                               srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out, cf_t* d_out, void* e_out, float* csi_out, cf_t* sym_out,
                                               cf_t* ce_out, cf_t* ce_grid_out)
{
  return pdsch_decode_one_est(g, sf, est, state_in, sf_symbols, softbuffer, data, res, est_out, d_out, e_out, csi_out, sym_out, ce_out, ce_grid_out);
}

// ------------------------------------------------------------------------------------------------ PDSCH receive, the frame of every grant call

int phyhip::chan::pdsch_decode_grant(RxGrant& g, const RxFront& front)
{
  ChanStage* sp = stage_for(g.who);
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&     s      = *sp;
  const uint32_t nof_re = g.cw[0].tb->nof_re;
  const bool     llr8   = g.cw[0].tb->llr_is_8bit != 0;
  const size_t   nd = (size_t)nof_re * sizeof(cf_t), nb = al256(nd), nr = (size_t)nof_re * sizeof(float), nc = g.weight ? csi_plane(nof_re) : 0;
  bool           want_d = false;
  for (uint32_t k = 0; k < g.n_cw; k++) {
    want_d = want_d || (g.d_planes && g.cw[k].d_out);
  }
  // pinned: the planes, the equalised symbols, each codeword's soft bits, each codeword's CSI row; device: the equalised symbols, the front end's CSI rows
  // (with g.map: the staged rows of every grid and the segment table where the planes would be)
  const pdsch_map::Window w = g.map ? pdsch_map::window(*g.map->sf) : pdsch_map::Window{};
  uint32_t                n_pl = 0;
  for (uint32_t i = 0; i < g.n_in; i++) {
    n_pl += g.in[i].k;
  }
  // (with g.est: the estimator's input first -- whole grids, one behind the other -- and the table over whole grids)
  const chest_dl::Layout el      = g.est ? chest_dl::layout_of(*g.est->cfg) : chest_dl::Layout{};
  const uint32_t         n_pairs = g.est ? g.est->cfg->nof_rx * g.est->cfg->nof_ports : 0;
  const size_t           gb      = (size_t)el.grid_points * sizeof(cf_t);
  const size_t sb = g.est ? gb : al256((size_t)w.staged_points() * sizeof(cf_t)), o_tab = g.est ? al256((size_t)el.in_points * sizeof(cf_t)) : n_pl * sb;
  const size_t o_d = g.map ? o_tab + al256(w.n_seg * sizeof(pdsch_map::Seg)) : plane_room(g.in, g.n_in);
  size_t       ne[2] = {0, 0}, o_e[2] = {0, 0}, o_c = o_d + g.d_planes * nb;
  for (uint32_t k = 0; k < g.n_cw; k++) {
    ne[k]  = (size_t)nof_re * qm_of(g.cw[k].tb->mod) * (llr8 ? 1 : 2);
    o_e[k] = o_c;
    o_c += al256(ne[k]);
  }
  const bool   dev_rows = g.weight && !g.csi;
  const size_t o_dc     = (want_d || g.d_scratch) ? g.d_planes * nb : 0;
  // the de-mapped planes: device scratch behind the CSI rows; pinned room behind everything else for the ones _sf_dbg asked for
  bool want_m = false;
  for (uint32_t i = 0; g.map && i < n_pl; i++) {
    want_m = want_m || g.map->out[i];
  }
  const size_t o_dm = o_dc + (dev_rows ? g.n_cw * nc : 0), o_m = o_c + g.n_cw * nc;
  // the estimator's jobs and records, and pinned room for the ce grids _est_dbg asked for; device: its ce grids behind the planes, the pairs' noise estimates
  bool want_g = false;
  for (uint32_t i = 0; i < n_pairs; i++) {
    want_g = want_g || g.est->grid_out[i % g.est->cfg->nof_ports][i / g.est->cfg->nof_ports];
  }
  const size_t o_ej = al256(o_m + (want_m ? n_pl * nb : 0)), o_er = al256(o_ej + n_pairs * sizeof(chest_dl::Job));
  const size_t o_eg = al256(o_er + n_pairs * sizeof(chest_dl::Record)), pin_need = g.est ? o_eg + (want_g ? n_pairs * gb : 0) : o_m + (want_m ? n_pl * nb : 0);
  const size_t o_dg = al256(o_dm + (g.map ? n_pl * nb : 0)), o_dn = o_dg + al256(n_pairs * gb), dev_need = g.est ? o_dn + 256 : o_dm + (g.map ? n_pl * nb : 0);
  if (n_pl > PDSCH_MAX_RX_PLANES || (g.est && !g.map) || !s.grow(pin_need, dev_need)) {
    fprintf(stderr, "[srsran_phy_hip] %s: staging allocation failed\n", g.who);
    return SRSRAN_ERROR;
  }
  auto* ejobs = reinterpret_cast<chest_dl::Job*>(s.pin + o_ej);
  if (g.est) {
    const srsran_hip_chest_dl_t& c = *g.est->cfg;
    chest_dl::stage_input(reinterpret_cast<cf_t*>(s.pin.get()), c, el, g.in[0].host);
    chest_dl::make_jobs(ejobs, c, *g.est->state, el);
    for (uint32_t i = 0; i < n_pairs; i++) { // the ce grids in the order of the planes: [port][rx]
      ejobs[i].o_ce = ((i % c.nof_ports) * c.nof_rx + i / c.nof_ports) * el.grid_points;
    }
    for (uint32_t at = 0; at < n_pl; at++) {
      uint32_t i = 0, k = at;
      for (; k >= g.in[i].k; k -= g.in[i].k, i++) {
      }
      g.in[i].pin[k] = reinterpret_cast<cf_t*>(s.dev + o_dm + at * nb);
    }
    const pdsch_map::Window whole = {0, 2 * c.cp_nsymb, 0, c.nof_prb, w.n_seg, w.nof_re};
    pdsch_map::fill_table(*g.map->sf, whole, reinterpret_cast<pdsch_map::Seg*>(s.pin + o_tab));
    g.est->noise = {reinterpret_cast<const float*>(s.dev + o_dn), c.nof_rx, c.nof_ports};
  } else if (g.map) {
    uint32_t at = 0;
    for (uint32_t i = 0; i < g.n_in; i++) {
      for (uint32_t k = 0; k < g.in[i].k; k++, at++) {
        stage_grid(s.pin + at * sb, g.in[i].host[k], *g.map->sf, w);
        g.in[i].pin[k] = reinterpret_cast<cf_t*>(s.dev + o_dm + at * nb);
      }
    }
    pdsch_map::fill_table(*g.map->sf, w, reinterpret_cast<pdsch_map::Seg*>(s.pin + o_tab));
  } else {
    place_planes(s.pin, g.in, g.n_in);
  }
  if (g.csi) {
    memcpy(s.pin + o_c, g.csi, nr);
  }
  // the enabled codewords as items of one decoding pass
  static const sch::FrontEnd device_made = [](hipStream_t, void*) { return false; }; // (never called: the group front end below serves the call's codewords)
  srsran_cbsegm_t            seg[2];
  srsran_hip_sch_head_t      head[2];
  sch::TbItem                items[2];
  uint32_t                   cw_of[2] = {0, 0}, n_items = 0;
  float*                     row[2] = {nullptr, nullptr};
  for (uint32_t k = 0; k < g.n_cw; k++) {
    const RxCodeword& c = g.cw[k];
    if (g.weight) {
      row[k] = reinterpret_cast<float*>(dev_rows ? s.dev + o_dc + k * nc : s.pin + o_c + k * nc);
    }
    if (!c.sb) {
      continue;
    }
    if (!segment(&seg[k], c.tb->tbs)) { // (behind the caller's checks: it cannot fail for a grant tb_valid has passed)
      return SRSRAN_ERROR;
    }
    head[k]          = {c.tb->max_nof_iterations, 0.f, llr8};
    cw_of[n_items]   = k;
    items[n_items++] = {&head[k], c.sb, &seg[k], c.Qm, c.tb->rv, nof_re * qm_of(c.tb->mod), nullptr, &device_made, c.data, false};
  }
  // what the front end actually made: it does not run for a codeword the transport-block stage drops
  bool                     d_made = false, e_made[2] = {false, false}, c_made[2] = {false, false}, m_made = false, est_made = false, g_made = false;
  const sch::GroupFrontEnd group  = [&](hipStream_t st, const uint32_t* which, void* const* d_e, uint32_t m) -> bool {
    void*       de[2] = {nullptr, nullptr};
    CsiCodeword wj[2];
    for (uint32_t j = 0; j < m && j < 2; j++) {
      const uint32_t k = cw_of[which[j]];
      de[k] = d_e[j];
      wj[j] = {d_e[j], row[k], g.cw[k].tb->mod};
    }
    if (g.est) {
      const chest_dl::Params cp = {reinterpret_cast<const float2*>(s.pin.get()), reinterpret_cast<float2*>(s.dev + o_dg), ejobs, reinterpret_cast<chest_dl::Record*>(s.pin + o_er),
                                   reinterpret_cast<float*>(s.dev + o_dn), n_pairs, el.in_points, n_pairs * el.grid_points};
      if (chest_dl::launch(cp, st) != hipSuccess) {
        set_error("grant front end: channel estimator launch failed");
        return false;
      }
      est_made = true;
    }
    if (g.map) {
      pdsch_map::DemapParams dp = {reinterpret_cast<const float2*>(s.pin.get()), reinterpret_cast<float2*>(s.dev + o_dm), reinterpret_cast<const pdsch_map::Seg*>(s.pin + o_tab),
                                   w.n_seg, n_pl, (uint32_t)(sb / sizeof(cf_t)), g.est ? el.grid_points : w.staged_points(), (uint32_t)(nb / sizeof(cf_t)), nof_re};
      if (g.est) { // the received grids from the pinned image, the ce grids from where the estimator left them
        dp.in_b     = reinterpret_cast<const float2*>(s.dev + o_dg);
        dp.planes_a = g.est->cfg->nof_rx;
      }
      if (pdsch_map::launch_demap(dp, st) != hipSuccess) {
        set_error("grant front end: RE de-mapping launch failed");
        return false;
      }
    }
    if (!front(st, de, row, o_dc ? s.dev.get() : nullptr) || (g.weight && !enqueue_csi_weight(st, wj, m, nof_re, llr8))) {
      return false;
    }
    bool copied = !want_d || hipMemcpyAsync(s.pin + o_d, s.dev, (g.d_planes - 1) * nb + nd, hipMemcpyDeviceToHost, st) == hipSuccess;
    d_made      = want_d && copied;
    if (copied && want_m) {
      copied = m_made = hipMemcpyAsync(s.pin + o_m, s.dev + o_dm, (n_pl - 1) * nb + nd, hipMemcpyDeviceToHost, st) == hipSuccess;
    }
    if (copied && want_g) {
      copied = g_made = hipMemcpyAsync(s.pin + o_eg, s.dev + o_dg, n_pairs * gb, hipMemcpyDeviceToHost, st) == hipSuccess;
    }
    for (uint32_t j = 0; copied && j < m; j++) {
      const uint32_t k = cw_of[which[j]];
      if (g.weight && g.cw[k].csi_out) { // (the caller's row is in the image already)
        copied = c_made[k] = !dev_rows || hipMemcpyAsync(s.pin + o_c + k * nc, row[k], nr, hipMemcpyDeviceToHost, st) == hipSuccess;
      }
      if (copied && g.cw[k].e_out) {
        copied = e_made[k] = hipMemcpyAsync(s.pin + o_e[k], d_e[j], ne[k], hipMemcpyDeviceToHost, st) == hipSuccess;
      }
    }
    if (!copied) {
      set_error("grant front end: copy of the intermediate results failed");
    }
    return copied;
  };
  const bool device_ok = sch::decode_tbs_staged(items, n_items, &group);
  for (uint32_t i = 0; i < n_items; i++) {
    const RxCodeword& c = g.cw[cw_of[i]];
    c.res->crc_ok               = items[i].ok ? 1 : 0;
    c.res->avg_iterations_block = head[cw_of[i]].avg_iterations;
  }
  if (!device_ok) {
    return SRSRAN_ERROR;
  }
  // what _dbg was asked for and the front end did not make is an error, not a silently untouched buffer
  bool missing = false;
  const auto hand_back = [&](void* out, bool made, size_t off, size_t bytes) {
    if (out && made) {
      memcpy(out, s.pin + off, bytes);
    }
    missing = missing || (out && !made);
  };
  for (uint32_t k = 0; k < g.n_cw; k++) {
    const RxCodeword& c = g.cw[k];
    hand_back(g.d_planes ? c.d_out : nullptr, d_made, o_d + k * nb, nd);
    hand_back(c.sb ? c.e_out : nullptr, e_made[k], o_e[k], ne[k]);
    hand_back(c.sb && g.weight ? c.csi_out : nullptr, c_made[k], o_c + k * nc, nr);
  }
  for (uint32_t i = 0; g.map && i < n_pl; i++) {
    hand_back(g.map->out[i], m_made, o_m + i * nb, nd);
  }
  if (g.est) { // the measurements from the pairs' records (behind the host wait); the front end did not run: they stay zeroed
    const srsran_hip_chest_dl_t& c = *g.est->cfg;
    if (est_made) {
      chest_dl::finish(c, *g.est->state, reinterpret_cast<const chest_dl::Record*>(s.pin + o_er), srsran_symbol_sz(c.nof_prb), g.est->out);
    }
    missing = missing || !est_made;
    for (uint32_t i = 0; i < n_pairs; i++) {
      hand_back(g.est->grid_out[i % c.nof_ports][i / c.nof_ports], g_made, o_eg + (size_t)ejobs[i].o_ce * sizeof(cf_t), gb);
    }
  }
  if (missing) {
    set_error("%s: an intermediate result that was asked for was not produced (the front end did not run for that codeword)", g.who);
    fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ transmit side

namespace {
bool enqueue_mod(hipStream_t st, const uint8_t* d_bits, uint32_t mod, uint32_t n, uint32_t seed, bool scramble, float scale, uint8_t* p_out)
{
  modem::Params sp;
  if (!modem::params_for(sp, modem::LLR_I16)) {
    return false;
  }
  const float2* tab = modem::mod_tables();
  if (!tab) {
    return false;
  }
  modem::ModParams p = {};
  p.bits     = d_bits;
  p.out      = reinterpret_cast<float2*>(p_out);
  p.table    = tab;
  p.mod      = mod;
  p.n        = n;
  p.seed     = seed;
  p.scramble = scramble ? 1u : 0u;
  p.scale    = scale;
  p.x1_bits  = sp.x1_bits;
  p.x2_cols  = sp.x2_cols;
  if (modem::launch_mod(p, st) != hipSuccess) {
    set_error("modulator launch failed");
    return false;
  }
  return true;
}
} // namespace

extern "C" int srsran_hip_pdsch_encode(const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* symbols)
{
  return srsran_hip_pdsch_encode_dbg(g, softbuffer, data, symbols, nullptr);
}

extern "C" int srsran_hip_pdsch_encode_dbg(const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* symbols, uint8_t* e_out)
{
  TraceRange trace_("srsran_hip_pdsch_encode");
  if (!g || !softbuffer || !symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!tb_valid(g->tb, "srsran_hip_pdsch_encode")) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_encode");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&      s = *sp;
  srsran_cbsegm_t seg;
  if (!segment(&seg, g->tb.tbs)) {
    return SRSRAN_ERROR;
  }
  const size_t nb = (size_t)g->tb.nof_re * sizeof(cf_t);
  const size_t nw = (((size_t)g->tb.nof_re * qm_of(g->tb.mod) + 31) / 32) * 4; // scrambled bits, whole words
  if (!s.grow(al256(nb) + al256(nw), al256(nw))) {
    return SRSRAN_ERROR;
  }
  const srsran_hip_grant_tb_t tb    = g->tb;
  uint8_t *                   pout = s.pin, *p_e = s.pin + al256(nb), *d_scr = s.dev;
  const float                 scale = g->scaling != 0.f ? g->scaling : 1.0f;
  const bool                  want_e = e_out != nullptr;
  const sch::BackEnd          back  = [=](hipStream_t st, const uint8_t* d_e) {
    if (!want_e) {
      return enqueue_mod(st, d_e, tb.mod, tb.nof_re, tb.seed, true, scale, pout);
    }
    // the scrambled bits are wanted by themselves (q->e): scramble in packed form, hand that to the modulator and to the host
    modem::Params sp;
    if (!modem::params_for(sp, modem::LLR_I16)) {
      return false;
    }
    if (modem::launch_scramble_packed(d_e, d_scr, tb.nof_re * qm_of(tb.mod), tb.seed, sp.x1_bits, sp.x2_cols, st) != hipSuccess ||
        hipMemcpyAsync(p_e, d_scr, nw, hipMemcpyDeviceToHost, st) != hipSuccess) {
      set_error("packed scrambler launch failed");
      return false;
    }
    return enqueue_mod(st, d_scr, tb.mod, tb.nof_re, 0, false, scale, pout);
  };
  const int rc = sch::encode_tb_staged(softbuffer, &seg, qm_rm(tb), tb.rv, tb.nof_re * qm_of(tb.mod), data, nullptr, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  memcpy(symbols, s.pin, nb);
  if (want_e) {
    memcpy(e_out, p_e, ((size_t)tb.nof_re * qm_of(tb.mod) + 7) / 8);
  }
  return SRSRAN_SUCCESS;
}

// the codewords of a TTI (srsenb/src/phy/lte/cc_worker.cc encode_pdsch: one srsran_enb_dl_put_pdsch per scheduled UE) in ONE call: one coding launch over
// the code blocks of all of them, one scrambling + modulation launch, one host wait
extern "C" int srsran_hip_pdsch_encode_multi(uint32_t n, const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* const* softbuffers, uint8_t* const* data,
                                             cf_t* const* symbols)
{
  TraceRange trace_("srsran_hip_pdsch_encode");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !softbuffers || !data || !symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (n == 1) {
    return srsran_hip_pdsch_encode(&g[0], softbuffers[0], data[0], symbols[0]);
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_encode");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&              s = *sp;
  std::vector<TxCodeword> cw(n);
  for (uint32_t i = 0; i < n; i++) {
    if (!softbuffers[i] || !symbols[i] || !tb_valid(g[i].tb, "srsran_hip_pdsch_encode")) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    cw[i] = {&g[i].tb, qm_rm(g[i].tb), 1, softbuffers[i], data[i], &symbols[i], 0};
  }
  return pdsch_encode_codewords<modem::ModJob>(s, cw.data(), n, [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, JobList<modem::ModJob>& jobs) {
    modem::Params sp;
    const float2* tab = modem::mod_tables();
    if (!modem::params_for(sp, modem::LLR_I16) || !tab) {
      return false;
    }
    for (uint32_t i = 0; i < n; i++) {
      jobs.jobs[i] = {g[i].tb.mod, g[i].tb.nof_re, g[i].tb.seed, 1u, g[i].scaling != 0.f ? g[i].scaling : 1.0f, e_byte_off[i], (uint32_t)(cw[i].o_out / sizeof(cf_t)),
                      jobs.append(i, modem::tiles_of(g[i].tb.mod, g[i].tb.nof_re))};
    }
    modem::ModParams p = {};
    p.bits     = d_e;
    p.out      = reinterpret_cast<float2*>(s.pin.get());
    p.table    = tab;
    p.x1_bits  = sp.x1_bits;
    p.x2_cols  = sp.x2_cols;
    p.jobs     = jobs.jobs;
    p.tile_job = jobs.tile_job;
    if (modem::launch_mod_jobs(p, jobs.n_tiles, st) != hipSuccess) {
      set_error("modulator launch failed");
      return false;
    }
    return true;
  });
}

extern "C" int srsran_hip_ulsch_encode(const srsran_hip_grant_tb_t* tbp, uint32_t nof_symb, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, uint8_t* q_bits)
{
  TraceRange trace_("srsran_hip_ulsch_encode");
  if (!tbp || !softbuffer || !q_bits) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const srsran_hip_grant_tb_t tb = *tbp;
  if (!tb_valid(tb, "srsran_hip_ulsch_encode") || nof_symb == 0 || tb.nof_re % nof_symb || tb.mod < SRSRAN_MOD_QPSK || tb.mod > SRSRAN_MOD_64QAM) {
    fprintf(stderr, "Invalid input\n"); // sch.c:1213-1221
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = stage_for("srsran_hip_ulsch_encode");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&      s = *sp;
  srsran_cbsegm_t seg;
  if (!segment(&seg, tb.tbs)) {
    return SRSRAN_ERROR;
  }
  const uint32_t Qm = qm_of(tb.mod);
  const size_t   nb = ((size_t)tb.nof_re * Qm + 7) / 8;
  if (!s.grow(al256(nb), 0)) {
    return SRSRAN_ERROR;
  }
  uint8_t*           pout = s.pin;
  const sch::BackEnd back = [=](hipStream_t st, const uint8_t* d_e) {
    if (chan::launch_ul_interleave_bits(d_e, pout, tb.nof_re, Qm, nof_symb, st) != hipSuccess) {
      set_error("channel interleaver launch failed");
      return false;
    }
    return true;
  };
  const int rc = sch::encode_tb_staged(softbuffer, &seg, Qm, tb.rv, tb.nof_re * Qm, data, nullptr, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  memcpy(q_bits, s.pin, nb);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_modulate_bytes(uint32_t mod, const uint8_t* bits, cf_t* symbols, uint32_t nbits, uint32_t seed, uint32_t scramble, float scaling)
{
  if (mod > SRSRAN_MOD_256QAM || !bits || !symbols) {
    return -1;
  }
  const uint32_t Qm = qm_of(mod);
  if (nbits % Qm) {
    fprintf(stderr, "Error modulator expects number of bits (%d) to be multiple of %d\n", nbits, Qm); // mod.c:141-144
    return -1;
  }
  const uint32_t n = nbits / Qm;
  if (n == 0) {
    return 0;
  }
  if (scramble && nbits > SRSRAN_HIP_SEQUENCE_MAX_LEN) {
    return -1;
  }
  ChanStage* sp = stage_for("srsran_hip_modulate_bytes");
  if (!sp) {
    return -1;
  }
  ChanStage&  s  = *sp;
  hipStream_t st = sch::stage_stream();
  const size_t o_out = al256((nbits + 7) / 8 + 1);
  if (!st || !s.grow(o_out + (size_t)n * sizeof(cf_t), 0)) {
    return -1;
  }
  memcpy(s.pin, bits, (nbits + 7) / 8);
  if (!enqueue_mod(st, s.pin, mod, n, seed, scramble != 0, scaling != 0.f ? scaling : 1.0f, s.pin + o_out)) {
    (void)hipStreamSynchronize(st);
    return -1;
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    return -1;
  }
  memcpy(symbols, s.pin + o_out, (size_t)n * sizeof(cf_t));
  return (int)n;
}

