// chan_host.cpp -- one device call per grant (include/srsran_amd/phy_chan_abi.h): the stages between the resource grid and the transport
// block of srsran_pusch_decode (pusch.c:358-478), srsran_pdsch_decode / _encode (pdsch.c:662-760, 949-1015) and srsran_ulsch_encode
// (sch.c:1194) chained on the calling thread's transport-block stream, nothing but the inputs and the results crossing the bus.
#include "chan_device.h"
#include "hip_common.h"
#include "modem_device.h"
#include "sch_stage.h"
#include "stage.h"
#include "txdiv_device.h"
#include "srsran_amd/phy_chan_abi.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

using namespace phyhip;

namespace {

inline uint32_t qm_of(uint32_t mod)
{
  return mod == 0 ? 1u : 2u * mod;
}
inline uint32_t qm_rm(const srsran_hip_grant_tb_t& tb) // what decode_tb / encode_tb get as Qm (sch.c:590,632)
{
  return qm_of(tb.mod) * (tb.nl ? tb.nl : 1u);
}

// per calling thread: pinned images the kernels read the grant's symbols / channel estimates from and write transmit symbols into, device
// scratch between the front-end kernels, the transform plans of the allocation sizes seen so far
struct ChanStage {
  HostImage pin;
  DeviceBuf dev;
  std::map<uint32_t, srsran_hip_dft_batch_t*> idft; // L_prb -> backward, normalised plan of 12 L_prb points (srsran_dft_precoding_init_rx)
  ~ChanStage()
  {
    for (auto& kv : idft) {
      srsran_hip_dft_batch_free(kv.second);
    }
  }
  bool grow(size_t need_pin, size_t need_dev) { return pin.grow(need_pin, need_pin / 2) && dev.grow(need_dev, need_dev / 2); }
  srsran_hip_dft_batch_t* plan(uint32_t L_prb)
  {
    auto it = idft.find(L_prb);
    if (it != idft.end()) {
      return it->second;
    }
    srsran_hip_dft_batch_t* h = nullptr;
    if (srsran_hip_dft_batch_create(&h, (int)(12 * L_prb), SRSRAN_DFT_BACKWARD, false, false, true) != SRSRAN_SUCCESS) {
      return nullptr;
    }
    idft[L_prb] = h;
    return h;
  }
};

ChanStage& stage()
{
  static thread_local StageRef<ChanStage> r;
  return r.get();
}

// the calling thread's stage; nullptr (one line on stderr) without a device
ChanStage* stage_for(const char* who)
{
  if (!device_available()) {
    fprintf(stderr, "[srsran_phy_hip] %s: %s (there is no CPU fallback)\n", who, get_error());
    return nullptr;
  }
  bind_thread();
  return &stage();
}

bool segment(srsran_cbsegm_t* seg, uint32_t tbs)
{
  if (srsran_cbsegm(seg, tbs) != SRSRAN_SUCCESS) {
    fprintf(stderr, "Error computing segmentation for TBS=%d\n", tbs); // sch.c:637-640, 1133-1136, 1224-1228
    return false;
  }
  return true;
}

bool tb_valid(const srsran_hip_grant_tb_t& tb, const char* who)
{
  if (tb.mod > SRSRAN_MOD_256QAM || tb.nl > 2 || tb.nof_re == 0 || tb.tbs == 0 || (tb.tbs & 7u) || tb.rv > 3 ||
      (uint64_t)tb.nof_re * qm_of(tb.mod) > SRSRAN_HIP_SEQUENCE_MAX_LEN) {
    set_error("%s: invalid grant (mod %u, %u REs, tbs %u, rv %u)", who, tb.mod, tb.nof_re, tb.tbs, tb.rv);
    fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
    return false;
  }
  return true;
}

// the receive front end of one grant, enqueued on `st`: [equaliser] -> [transform de-precoding] -> demodulator + descrambler (+ UL channel
// de-interleaver in its store) -> d_e.  p_sym / p_ce: the grant's REs in the pinned image; d_x / d_z: device scratch of nof_re points each.
bool enqueue_rx_front(hipStream_t st, const srsran_hip_grant_tb_t& tb, const uint8_t* p_sym, const uint8_t* p_ce, float scaling, float noise, uint32_t L_prb,
                      uint32_t nof_symb, uint8_t* d_x, uint8_t* d_z, srsran_hip_dft_batch_t* plan, void* d_e)
{
  const uint8_t* cur = p_sym;
  if (p_ce) {
    if (modem::launch_eq(p_sym, p_ce, d_x, nullptr, tb.nof_re, scaling, noise, st) != hipSuccess) {
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
};

inline bool has_uci(const srsran_hip_pusch_uci_t& u)
{
  return (u.Q_prime_ack | u.Q_prime_ri | u.Q_prime_cqi) != 0;
}

} // namespace

// ------------------------------------------------------------------------------------------------ PUSCH receive

// the grants of a call.  uci == nullptr: srsran_hip_pusch_decode{,_multi}; else uci[i] / out[i] are grant i's control-information counts and outputs
// (srsran_hip_pusch_decode_uci{,_multi}) and the 16-bit grants' demodulator launch is the de-multiplexing one (modem::launch_uci).
static int pusch_decode_grants(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* const* sf_symbols, const cf_t* const* ce,
                               srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data, srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* out)
{
  TraceRange trace_("srsran_hip_pusch_decode");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !sf_symbols || !ce || !softbuffers || !data || !res) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = stage_for("srsran_hip_pusch_decode");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&             s = *sp;
  std::vector<PuschPlan> pl(n);
  size_t                 pin_need = 0, dev_need = 0;
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_pusch_rx_t& x = g[i];
    res[i] = {0, 0.f, NAN};
    if (!tb_valid(x.tb, "srsran_hip_pusch_decode") || !sf_symbols[i] || !ce[i] || !softbuffers[i] || !data[i]) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    const uint32_t nsymb = 2 * (x.cp_nsymb - 1) - (x.shortened ? 1u : 0u);
    if ((x.cp_nsymb != 7 && x.cp_nsymb != 6) || x.L_prb == 0 || !srsran_dft_precoding_valid_prb(x.L_prb) || x.n_prb_tilde[0] + x.L_prb > x.cell_nof_prb ||
        x.n_prb_tilde[1] + x.L_prb > x.cell_nof_prb || x.tb.nof_re != nsymb * 12 * x.L_prb || x.tb.mod < SRSRAN_MOD_QPSK || x.tb.mod > SRSRAN_MOD_64QAM) {
      set_error("srsran_hip_pusch_decode: grant %u: allocation (%u PRB at %u / %u of %u, %u REs, mod %u) is not a PUSCH allocation", i, x.L_prb, x.n_prb_tilde[0],
                x.n_prb_tilde[1], x.cell_nof_prb, x.tb.nof_re, x.tb.mod);
      fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
      return SRSRAN_ERROR_INVALID_INPUTS;
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
        set_error("srsran_hip_pusch_decode_uci: grant %u (Q'ack %u, Q'ri %u, Q'cqi %u, %u PRB): %s", i, u.Q_prime_ack, u.Q_prime_ri, u.Q_prime_cqi, x.L_prb, why);
        fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
        return SRSRAN_ERROR_INVALID_INPUTS;
      }
    }
    PuschPlan& p = pl[i];
    p.nof_symb   = nsymb;
    if (!segment(&p.seg, x.tb.tbs)) {
      return SRSRAN_ERROR;
    }
    p.plan = s.plan(x.L_prb);
    if (!p.plan) {
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
    pl[i].o_ce = region + pl[i].o_sym;
    pl[i].o_z  = region + pl[i].o_x;
  }
  const size_t o_eqj = 2 * region, o_mj = al256(o_eqj + n * sizeof(modem::EqJob)), o_tj = al256(o_mj + n * sizeof(modem::Job));
  pin_need = al256(o_tj + tiles * sizeof(uint32_t));
  dev_need = 2 * region;
  // with control information: the de-multiplexing demodulator's job list behind the others, then every grant's control image (the kernel stores the
  // control soft bits and chips straight into the pinned image: they are there after the call's one host wait)
  const size_t o_uj = pin_need;
  if (uci) {
    pin_need = al256(o_uj + n * sizeof(modem::UciJob));
    for (uint32_t i = 0; i < n; i++) {
      pl[i].o_uci = pin_need;
      pin_need    = al256(pin_need + modem::uci_image_bytes(uci[i].Q_prime_ack, uci[i].Q_prime_ri, uci[i].Q_prime_cqi, qm_of(g[i].tb.mod)));
    }
  }
  if (!s.grow(pin_need, dev_need)) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pusch_decode: staging allocation failed\n");
    return SRSRAN_ERROR;
  }
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
        memcpy(s.pin + p.o_ce + at, ce[i] + idx, wid);
        at += wid;
      }
    }
    if (x.meas_epre) {
      res[i].epre = avg_power(reinterpret_cast<const float*>(s.pin + p.o_sym), x.tb.nof_re); // pusch.c:397-401
    }
    p.head = {x.tb.max_nof_iterations, 0.f, x.tb.llr_is_8bit != 0};
    const srsran_hip_grant_tb_t tb = x.tb;
    const uint8_t *psym = s.pin + p.o_sym, *pce = s.pin + p.o_ce;
    uint8_t *      dx = s.dev + p.o_x, *dz = s.dev + p.o_z;
    const float    noise = x.noise_estimate;
    const uint32_t L_prb = x.L_prb, nsymb = p.nof_symb;
    auto*          plan  = p.plan;
    p.front = [=](hipStream_t st, void* d_e) { return enqueue_rx_front(st, tb, psym, pce, 1.0f, noise, L_prb, nsymb, dx, dz, plan, d_e); };
    // (with control information the transport block's e bits are what RI and CQI leave: G = H' - Q'ri - Q'cqi symbols, sch.c:1184-1190)
    const uint32_t G = uci ? x.tb.nof_re - uci[i].Q_prime_ri - uci[i].Q_prime_cqi : x.tb.nof_re;
    items[i] = {&p.head, softbuffers[i], &p.seg, qm_rm(x.tb), x.tb.rv, G * qm_of(x.tb.mod), nullptr, &p.front, data[i], false};
  }
  if (uci) { // a grant that does not reach the launch (sch_host.cpp refuses its soft buffer) leaves zeros
    memset(s.pin + pl[0].o_uci, 0, pin_need - pl[0].o_uci);
  }
  // the front end of all grants at once (n > 1)
  bool                     front_done = false;
  size_t                   job_cur = 0, tile_cur = 0;
  const sch::GroupFrontEnd group   = [&](hipStream_t st, const uint32_t* which, void* const* d_e, uint32_t m) -> bool {
    if (!front_done) {
      auto* ej = reinterpret_cast<modem::EqJob*>(s.pin + o_eqj);
      for (uint32_t k = 0; k < n; k++) {
        const srsran_hip_pusch_rx_t& x = g[ord[k]];
        ej[k] = {(uint32_t)((pl[ord[k]].o_sym + (size_t)x.tb.nof_re * sizeof(cf_t)) / (2 * sizeof(cf_t))), x.noise_estimate, x.noise_estimate > 0.f ? 1u : 0u};
      }
      if (modem::launch_eq_jobs(s.pin, s.pin + region, s.dev, ej, n, (uint32_t)(tot / (2 * sizeof(cf_t))), 1.0f, st) != hipSuccess) {
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
    if (uci && !llr8) { // the 16-bit grants of the call, with and without control information, in one de-multiplexing demodulator launch
      auto*    uj = reinterpret_cast<modem::UciJob*>(s.pin + o_uj) + job_cur;
      auto*    tj = reinterpret_cast<uint32_t*>(s.pin + o_tj) + tile_cur;
      uint32_t nt = 0;
      for (uint32_t k = 0; k < m; k++) {
        const uint32_t               i   = which[k];
        const srsran_hip_pusch_rx_t& x   = g[i];
        const uint32_t               cnt = modem::tiles_of(x.tb.mod, x.tb.nof_re);
        uj[k] = modem::UciJob{x.tb.mod, x.tb.nof_re, (uint32_t)(pl[i].o_x / sizeof(cf_t)), (uint32_t)((size_t)(static_cast<uint8_t*>(d_e[k]) - base) / es), x.tb.seed, nt, cnt,
                              12 * x.L_prb, pl[i].nof_symb, uci[i].Q_prime_ack, uci[i].Q_prime_ri, uci[i].Q_prime_cqi, (uint32_t)pl[i].o_uci};
        for (uint32_t t = 0; t < cnt; t++) {
          tj[nt++] = k;
        }
      }
      job_cur += m;
      tile_cur += nt;
      modem::UciParams up = {s.dev + region, base, s.pin, uj, tj, nt, p.x1_bits, p.x2_cols, p.k};
      if (modem::launch_uci(up, st) != hipSuccess) {
        set_error("grant front end: demodulator launch failed");
        return false;
      }
      return true;
    }
    auto*    mj  = reinterpret_cast<modem::Job*>(s.pin + o_mj) + job_cur;
    auto*    tj  = reinterpret_cast<uint32_t*>(s.pin + o_tj) + tile_cur;
    uint32_t nt  = 0;
    for (uint32_t k = 0; k < m; k++) {
      const srsran_hip_pusch_rx_t& x  = g[which[k]];
      const uint32_t               t0 = nt, cnt = modem::tiles_of(x.tb.mod, x.tb.nof_re);
      mj[k] = modem::Job{x.tb.mod, x.tb.nof_re, (uint32_t)(pl[which[k]].o_x / sizeof(cf_t)), (uint32_t)((size_t)(static_cast<uint8_t*>(d_e[k]) - base) / es), x.tb.seed, 1u, t0, cnt,
                         12 * x.L_prb, pl[which[k]].nof_symb};
      for (uint32_t t = 0; t < cnt; t++) {
        tj[nt++] = k;
      }
    }
    job_cur += m;
    tile_cur += nt;
    p.in       = s.dev + region;
    p.out      = base;
    p.jobs     = mj;
    p.tile_job = tj;
    p.n_jobs   = m;
    p.n_tiles  = nt;
    if (modem::launch(p, st) != hipSuccess) {
      set_error("grant front end: demodulator launch failed");
      return false;
    }
    return true;
  };
  sch::decode_tbs_staged(items.data(), n, (n > 1 || uci) ? &group : nullptr);
  for (uint32_t i = 0; i < n; i++) {
    res[i].crc_ok               = items[i].ok ? 1 : 0;
    res[i].avg_iterations_block = pl[i].head.avg_iterations;
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

// ------------------------------------------------------------------------------------------------ PDSCH receive, one codeword

extern "C" int srsran_hip_pdsch_decode(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* data, srsran_hip_grant_res_t* res)
{
  return srsran_hip_pdsch_decode_dbg(g, symbols, ce, softbuffer, data, res, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_dbg(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                           uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out)
{
  TraceRange trace_("srsran_hip_pdsch_decode");
  if (!g || !symbols || !softbuffer || !data || !res) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  *res = {0, 0.f, NAN};
  if (!tb_valid(g->tb, "srsran_hip_pdsch_decode") || (ce && !(g->scaling != 0.f))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_decode");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&      s = *sp;
  srsran_cbsegm_t seg;
  if (!segment(&seg, g->tb.tbs)) {
    return SRSRAN_ERROR;
  }
  const size_t nb = al256((size_t)g->tb.nof_re * sizeof(cf_t));
  const size_t ne = (size_t)g->tb.nof_re * qm_of(g->tb.mod) * (g->tb.llr_is_8bit ? 1 : 2);
  if (!s.grow(3 * nb + al256(ne), nb)) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_decode: staging allocation failed\n");
    return SRSRAN_ERROR;
  }
  memcpy(s.pin, symbols, (size_t)g->tb.nof_re * sizeof(cf_t));
  if (ce) {
    memcpy(s.pin + nb, ce, (size_t)g->tb.nof_re * sizeof(cf_t));
  }
  srsran_hip_sch_head_t       head = {g->tb.max_nof_iterations, 0.f, g->tb.llr_is_8bit != 0};
  const srsran_hip_grant_tb_t tb   = g->tb;
  const uint8_t *             psym = s.pin, *pce = ce ? s.pin + nb : nullptr;
  uint8_t*                    dx = s.dev;
  const float                 scaling = g->scaling, noise = g->noise_estimate;
  uint8_t *                   p_d = s.pin + 2 * nb, *p_e = s.pin + 3 * nb;
  const bool                  want_d = d_out && ce, want_e = e_out != nullptr;
  const sch::FrontEnd front = [=](hipStream_t st, void* d_e) {
    if (!enqueue_rx_front(st, tb, psym, pce, scaling, noise, 0, 0, dx, nullptr, nullptr, d_e)) {
      return false;
    }
    // what the reference leaves in q->d / q->e for its callers to look at
    if ((want_d && hipMemcpyAsync(p_d, dx, (size_t)tb.nof_re * sizeof(cf_t), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (want_e && hipMemcpyAsync(p_e, d_e, ne, hipMemcpyDeviceToHost, st) != hipSuccess)) {
      set_error("grant front end: copy of the intermediate results failed");
      return false;
    }
    return true;
  };
  const bool ok = sch::decode_tb_staged(&head, softbuffer, &seg, qm_rm(tb), tb.rv, tb.nof_re * qm_of(tb.mod), nullptr, &front, data);
  if (want_d) {
    memcpy(d_out, p_d, (size_t)tb.nof_re * sizeof(cf_t));
  }
  if (want_e) {
    memcpy(e_out, p_e, ne);
  }
  res->crc_ok               = ok ? 1 : 0;
  res->avg_iterations_block = head.avg_iterations;
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
  ChanStage&                   s = *sp;
  std::vector<srsran_cbsegm_t> seg(n);
  std::vector<sch::TxItem>     items(n);
  std::vector<size_t>          o_out(n);
  size_t                       out_bytes = 0, tiles = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!softbuffers[i] || !symbols[i] || !tb_valid(g[i].tb, "srsran_hip_pdsch_encode")) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (!segment(&seg[i], g[i].tb.tbs)) {
      return SRSRAN_ERROR;
    }
    items[i] = {softbuffers[i], &seg[i], qm_rm(g[i].tb), g[i].tb.rv, g[i].tb.nof_re * qm_of(g[i].tb.mod), data[i], 0};
    o_out[i] = out_bytes;
    out_bytes += al256((size_t)g[i].tb.nof_re * sizeof(cf_t));
    tiles += (g[i].tb.nof_re + MODEM_TILE_SYMS - 1) / MODEM_TILE_SYMS;
  }
  const size_t o_jobs = out_bytes, o_tj = al256(o_jobs + n * sizeof(modem::ModJob));
  if (!s.grow(al256(o_tj + tiles * sizeof(uint32_t)), 0)) {
    return SRSRAN_ERROR;
  }
  const sch::GroupBackEnd back = [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, uint32_t m) -> bool {
    modem::Params sp;
    const float2* tab = modem::mod_tables();
    if (m != n || !modem::params_for(sp, modem::LLR_I16) || !tab) {
      return false;
    }
    auto*    mj = reinterpret_cast<modem::ModJob*>(s.pin + o_jobs);
    auto*    tj = reinterpret_cast<uint32_t*>(s.pin + o_tj);
    uint32_t nt = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t cnt = (g[i].tb.nof_re + MODEM_TILE_SYMS - 1) / MODEM_TILE_SYMS;
      mj[i] = {g[i].tb.mod, g[i].tb.nof_re, g[i].tb.seed, 1u, g[i].scaling != 0.f ? g[i].scaling : 1.0f, e_byte_off[i], (uint32_t)(o_out[i] / sizeof(cf_t)), nt};
      for (uint32_t t = 0; t < cnt; t++) {
        tj[nt++] = i;
      }
    }
    modem::ModParams p = {};
    p.bits     = d_e;
    p.out      = reinterpret_cast<float2*>(s.pin.get());
    p.table    = tab;
    p.x1_bits  = sp.x1_bits;
    p.x2_cols  = sp.x2_cols;
    p.jobs     = mj;
    p.tile_job = tj;
    if (modem::launch_mod_jobs(p, nt, st) != hipSuccess) {
      set_error("modulator launch failed");
      return false;
    }
    return true;
  };
  const int rc = sch::encode_tbs_staged(items.data(), n, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  for (uint32_t i = 0; i < n; i++) {
    memcpy(symbols[i], s.pin + o_out[i], (size_t)g[i].tb.nof_re * sizeof(cf_t));
  }
  return SRSRAN_SUCCESS;
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

// ------------------------------------------------------------------------------------------------ transmit diversity on 2 and 4 ports
//
// The reference-named stages on HOST buffers (one kernel each on the calling thread's stage, like srsran_hip_modulate_bytes), their device-pointer twins, and
// the PDSCH codeword of a multi-port cell in one call each way (txdiv_kernels.hip).

namespace {

bool txdiv_shape(const char* who, int nof_ports, int nof_rx, int nof_symbols)
{
  if (nof_ports != 2 && nof_ports != 4) {
    fprintf(stderr, "Number of ports must be 2 or 4 for transmit diversity (nof_ports=%d)\n", nof_ports); // precoding.c:775
    return false;
  }
  if (nof_rx != 1 && nof_rx != 2) {
    fprintf(stderr, "[srsran_phy_hip] %s: 1 or 2 receive antennas are taken (nof_rxant=%d)\n", who, nof_rx);
    return false;
  }
  if (nof_symbols % nof_ports) {
    fprintf(stderr, "[srsran_phy_hip] %s: %d symbols are not whole groups of %d\n", who, nof_symbols, nof_ports);
    return false;
  }
  return true;
}

// the transmit factor as the reference computes it (precoding.c:1958, :1962): double arithmetic on the float argument, converted to float once
inline float txdiv_tx_scale(uint32_t nof_ports, float scaling)
{
  return nof_ports == 2 ? (float)(scaling * M_SQRT1_2) : (float)(scaling / M_SQRT2);
}

inline bool al16(const void* p)
{
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

} // namespace

extern "C" int srsran_hip_predecoding_diversity_multi(const cf_t* const d_y[SRSRAN_MAX_PORTS], const cf_t* const d_h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS],
                                                      cf_t* const d_x[SRSRAN_MAX_LAYERS], float* d_csi, uint32_t nof_rxant, uint32_t nof_ports,
                                                      uint32_t nof_symbols, float scaling, void* stream)
{
  if (!d_y || !d_h || !d_x || nof_symbols > 0x7fffffffu || !txdiv_shape("srsran_hip_predecoding_diversity_multi", (int)nof_ports, (int)nof_rxant, (int)nof_symbols) ||
      (reinterpret_cast<uintptr_t>(d_csi) & 7u)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  txdiv::EqParams p = {};
  for (uint32_t r = 0; r < nof_rxant; r++) {
    p.y[r] = reinterpret_cast<const float4*>(d_y[r]);
    for (uint32_t k = 0; k < nof_ports; k++) {
      p.h[k][r] = reinterpret_cast<const float4*>(d_h[k][r]);
      if (nof_symbols && (!d_h[k][r] || !al16(d_h[k][r]))) {
        return SRSRAN_ERROR_INVALID_INPUTS;
      }
    }
    if (nof_symbols && (!d_y[r] || !al16(d_y[r]))) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  for (uint32_t k = 0; k < nof_ports; k++) {
    p.x[k] = reinterpret_cast<float2*>(d_x[k]);
    if (nof_symbols && (!d_x[k] || !al16(d_x[k]))) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  p.csi      = d_csi;
  p.x_stride = 1;
  p.ports    = nof_ports;
  p.nof_rx   = nof_rxant;
  p.n        = nof_symbols;
  p.scaling  = scaling;
  PHY_HIP_CHECK(txdiv::launch_eq(p, (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_precoding_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* const d_y[SRSRAN_MAX_PORTS], uint32_t nof_ports,
                                              uint32_t nof_symbols, float scaling, void* stream)
{
  if (!d_x || !d_y || nof_symbols > 0x7fffffffu / 4 || !txdiv_shape("srsran_hip_precoding_diversity", (int)nof_ports, 1, 0)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  txdiv::PrecodeParams p = {};
  for (uint32_t k = 0; k < nof_ports; k++) {
    p.x[k] = reinterpret_cast<const float2*>(d_x[k]);
    p.y[k] = reinterpret_cast<float2*>(d_y[k]);
    if (nof_symbols && (!d_x[k] || !d_y[k] || !al16(d_y[k]) || (reinterpret_cast<uintptr_t>(d_x[k]) & 7u))) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  p.ports = nof_ports;
  p.n     = nof_symbols;
  p.scale = txdiv_tx_scale(nof_ports, scaling);
  PHY_HIP_CHECK(txdiv::launch_precode(p, (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

static int hip_layers(const cf_t* const* d_x, const cf_t* d_d, uint32_t nof_layers, uint32_t n, bool to_layers, void* stream)
{
  if (!d_x || nof_layers == 0 || nof_layers > SRSRAN_MAX_LAYERS || (uint64_t)n * nof_layers > 0x7fffffffu) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  txdiv::LayerParams p = {};
  for (uint32_t k = 0; k < nof_layers; k++) {
    p.x[k] = reinterpret_cast<float2*>(const_cast<cf_t*>(d_x[k]));
    if (n && (!d_x[k] || (reinterpret_cast<uintptr_t>(d_x[k]) & 7u))) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (n && (!d_d || (reinterpret_cast<uintptr_t>(d_d) & 7u))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  p.d         = reinterpret_cast<float2*>(const_cast<cf_t*>(d_d));
  p.layers    = nof_layers;
  p.n         = n;
  p.to_layers = to_layers ? 1u : 0u;
  PHY_HIP_CHECK(txdiv::launch_layers(p, (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_layermap_diversity(const cf_t* d_d, cf_t* const d_x[SRSRAN_MAX_LAYERS], uint32_t nof_layers, uint32_t nof_symbols, void* stream)
{
  return hip_layers(d_x, d_d, nof_layers, nof_layers ? nof_symbols / nof_layers : 0u, true, stream);
}

extern "C" int srsran_hip_layerdemap_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* d_d, uint32_t nof_layers, uint32_t nof_layer_symbols,
                                               void* stream)
{
  return hip_layers(d_x, d_d, nof_layers, nof_layer_symbols, false, stream);
}

// the HOST-buffer forms: planes into the thread's pinned image (the kernels work on it directly), one kernel, one wait, planes out
extern "C" int srsran_predecoding_diversity_multi(cf_t* y[SRSRAN_MAX_PORTS], cf_t* h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS], cf_t* x[SRSRAN_MAX_LAYERS],
                                                  float* csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_symbols, float scaling)
{
  if (!y || !h || !x || nof_symbols < 0 || !txdiv_shape("srsran_predecoding_diversity_multi", nof_ports, nof_rxant, nof_symbols)) {
    return -1;
  }
  if (nof_symbols == 0) {
    return 0;
  }
  for (int r = 0; r < nof_rxant; r++) {
    bool ok = y[r] != nullptr;
    for (int k = 0; k < nof_ports && ok; k++) {
      ok = h[k][r] != nullptr && x[k] != nullptr;
    }
    if (!ok) {
      return -1;
    }
  }
  ChanStage* sp = stage_for("srsran_predecoding_diversity_multi");
  if (!sp) {
    return -1;
  }
  ChanStage&   s  = *sp;
  hipStream_t  st = sch::stage_stream();
  const size_t n = (size_t)nof_symbols, nb = al256(n * sizeof(cf_t)), nl = al256(n / nof_ports * sizeof(cf_t));
  const size_t o_h = (size_t)nof_rxant * nb, o_x = o_h + (size_t)nof_rxant * nof_ports * nb, o_csi = o_x + (size_t)nof_ports * nl;
  float*       c = (csi && csi[0]) ? csi[0] : nullptr;
  if (!st || !s.grow(o_csi + al256(n * sizeof(float)), 0)) {
    return -1;
  }
  txdiv::EqParams p = {};
  for (int r = 0; r < nof_rxant; r++) {
    memcpy(s.pin + (size_t)r * nb, y[r], n * sizeof(cf_t));
    p.y[r] = reinterpret_cast<const float4*>(s.pin + (size_t)r * nb);
    for (int k = 0; k < nof_ports; k++) {
      uint8_t* at = s.pin + o_h + ((size_t)k * nof_rxant + r) * nb;
      memcpy(at, h[k][r], n * sizeof(cf_t));
      p.h[k][r] = reinterpret_cast<const float4*>(at);
    }
  }
  for (int k = 0; k < nof_ports; k++) {
    p.x[k] = reinterpret_cast<float2*>(s.pin + o_x + (size_t)k * nl);
  }
  p.csi      = c ? reinterpret_cast<float*>(s.pin + o_csi) : nullptr;
  p.x_stride = 1;
  p.ports    = (uint32_t)nof_ports;
  p.nof_rx   = (uint32_t)nof_rxant;
  p.n        = (uint32_t)nof_symbols;
  p.scaling  = scaling;
  const bool launched = txdiv::launch_eq(p, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess || !launched) {
    return -1;
  }
  for (int k = 0; k < nof_ports; k++) {
    memcpy(x[k], s.pin + o_x + (size_t)k * nl, n / nof_ports * sizeof(cf_t));
  }
  if (c) {
    memcpy(c, s.pin + o_csi, n * sizeof(float));
  }
  return nof_symbols / nof_ports;
}

extern "C" int srsran_precoding_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* y[SRSRAN_MAX_PORTS], int nof_ports, int nof_symbols, float scaling)
{
  if (!x || !y || nof_symbols < 0 || nof_symbols > 0x7fffffff / 4 || !txdiv_shape("srsran_precoding_diversity", nof_ports, 1, 0)) {
    return -1;
  }
  if (nof_symbols == 0) {
    return 0;
  }
  for (int k = 0; k < nof_ports; k++) {
    if (!x[k] || !y[k]) {
      return -1;
    }
  }
  ChanStage* sp = stage_for("srsran_precoding_diversity");
  if (!sp) {
    return -1;
  }
  ChanStage&   s  = *sp;
  hipStream_t  st = sch::stage_stream();
  const size_t n = (size_t)nof_symbols, nl = al256(n * sizeof(cf_t)), nb = al256(n * nof_ports * sizeof(cf_t));
  const size_t o_y = (size_t)nof_ports * nl;
  if (!st || !s.grow(o_y + (size_t)nof_ports * nb, 0)) {
    return -1;
  }
  txdiv::PrecodeParams p = {};
  for (int k = 0; k < nof_ports; k++) {
    memcpy(s.pin + (size_t)k * nl, x[k], n * sizeof(cf_t));
    p.x[k] = reinterpret_cast<const float2*>(s.pin + (size_t)k * nl);
    p.y[k] = reinterpret_cast<float2*>(s.pin + o_y + (size_t)k * nb);
  }
  p.ports = (uint32_t)nof_ports;
  p.n     = (uint32_t)nof_symbols;
  p.scale = txdiv_tx_scale((uint32_t)nof_ports, scaling);
  const bool launched = txdiv::launch_precode(p, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess || !launched) {
    return -1;
  }
  for (int k = 0; k < nof_ports; k++) {
    memcpy(y[k], s.pin + o_y + (size_t)k * nb, n * nof_ports * sizeof(cf_t));
  }
  return nof_ports * nof_symbols;
}

static int host_layers(cf_t* d, cf_t* x[SRSRAN_MAX_LAYERS], int nof_layers, int n, bool to_layers, const char* who)
{
  if (!d || !x || nof_layers < 1 || nof_layers > SRSRAN_MAX_LAYERS || n < 0 || (int64_t)n * nof_layers > 0x7fffffff) {
    return -1;
  }
  if (n == 0) {
    return 0;
  }
  for (int k = 0; k < nof_layers; k++) {
    if (!x[k]) {
      return -1;
    }
  }
  ChanStage* sp = stage_for(who);
  if (!sp) {
    return -1;
  }
  ChanStage&   s  = *sp;
  hipStream_t  st = sch::stage_stream();
  const size_t nl = al256((size_t)n * sizeof(cf_t)), nd = al256((size_t)n * nof_layers * sizeof(cf_t));
  if (!st || !s.grow(nd + (size_t)nof_layers * nl, 0)) {
    return -1;
  }
  txdiv::LayerParams p = {};
  p.d = reinterpret_cast<float2*>(s.pin.get());
  for (int k = 0; k < nof_layers; k++) {
    p.x[k] = reinterpret_cast<float2*>(s.pin + nd + (size_t)k * nl);
    if (!to_layers) {
      memcpy(p.x[k], x[k], (size_t)n * sizeof(cf_t));
    }
  }
  if (to_layers) {
    memcpy(p.d, d, (size_t)n * nof_layers * sizeof(cf_t));
  }
  p.layers    = (uint32_t)nof_layers;
  p.n         = (uint32_t)n;
  p.to_layers = to_layers ? 1u : 0u;
  const bool launched = txdiv::launch_layers(p, st) == hipSuccess;
  if (hipStreamSynchronize(st) != hipSuccess || !launched) {
    return -1;
  }
  if (to_layers) {
    for (int k = 0; k < nof_layers; k++) {
      memcpy(x[k], p.x[k], (size_t)n * sizeof(cf_t));
    }
  } else {
    memcpy(d, p.d, (size_t)n * nof_layers * sizeof(cf_t));
  }
  return to_layers ? n : n * nof_layers;
}

extern "C" int srsran_layermap_diversity(cf_t* d, cf_t* x[SRSRAN_MAX_LAYERS], int nof_layers, int nof_symbols)
{
  return host_layers(d, x, nof_layers, (nof_layers > 0 && nof_symbols >= 0) ? nof_symbols / nof_layers : -1, true, "srsran_layermap_diversity");
}

extern "C" int srsran_layerdemap_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* d, int nof_layers, int nof_layer_symbols)
{
  return host_layers(d, x, nof_layers, nof_layer_symbols, false, "srsran_layerdemap_diversity");
}

// ---- PDSCH codeword with transmit diversity, receive

extern "C" int srsran_hip_pdsch_decode_txdiv(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                             srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res)
{
  return srsran_hip_pdsch_decode_txdiv_dbg(g, symbols, ce, softbuffer, data, res, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                 srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out)
{
  TraceRange trace_("srsran_hip_pdsch_decode_txdiv");
  if (res) {
    *res = {0, 0.f, NAN};
  }
  if (!g || !symbols || !ce || !softbuffer || !data || !res) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_decode_txdiv: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!tb_valid(g->tb, "srsran_hip_pdsch_decode_txdiv")) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t ports = g->nof_ports, nrx = g->nof_rx, nof_re = g->tb.nof_re;
  bool           planes = (ports == 2 || ports == 4) && (nrx == 1 || nrx == 2);
  for (uint32_t r = 0; planes && r < nrx; r++) {
    planes = symbols[r] != nullptr;
    for (uint32_t k = 0; planes && k < ports; k++) {
      planes = ce[k][r] != nullptr;
    }
  }
  if (!planes || nof_re % ports || !(g->scaling != 0.f) || !std::isfinite(g->scaling)) {
    set_error("srsran_hip_pdsch_decode_txdiv: %u ports, %u receive antennas, %u REs, scaling %g%s is not a transmit-diversity grant", ports, nrx, nof_re, (double)g->scaling,
              (ports == 2 || ports == 4) && (nrx == 1 || nrx == 2) && !planes ? ", a NULL plane" : "");
    fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_decode_txdiv");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&      s = *sp;
  srsran_cbsegm_t seg;
  if (!segment(&seg, g->tb.tbs)) {
    return SRSRAN_ERROR;
  }
  // staging image: nof_rx symbol planes, then nof_ports x nof_rx estimate planes, each 256-byte aligned; behind them room for what _dbg hands back
  const srsran_hip_grant_tb_t tb = g->tb;
  const uint32_t              Qm = qm_of(tb.mod);
  const size_t                nb = al256((size_t)nof_re * sizeof(cf_t));
  const size_t                ne = (size_t)nof_re * Qm * (tb.llr_is_8bit ? 1 : 2);
  const size_t                o_d = (size_t)nrx * (1 + ports) * nb, o_e = o_d + nb;
  const bool                  want_d = d_out != nullptr, want_e = e_out != nullptr;
  if (!s.grow(o_e + al256(ne), want_d ? nb : 0)) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_decode_txdiv: staging allocation failed\n");
    return SRSRAN_ERROR;
  }
  txdiv::FrontParams fp = {};
  txdiv::EqParams    ep = {};
  for (uint32_t r = 0; r < nrx; r++) {
    memcpy(s.pin + (size_t)r * nb, symbols[r], (size_t)nof_re * sizeof(cf_t));
    fp.y[r] = ep.y[r] = reinterpret_cast<const float4*>(s.pin + (size_t)r * nb);
    for (uint32_t k = 0; k < ports; k++) {
      uint8_t* at = s.pin + ((size_t)nrx + (size_t)k * nrx + r) * nb;
      memcpy(at, ce[k][r], (size_t)nof_re * sizeof(cf_t));
      fp.h[k][r] = ep.h[k][r] = reinterpret_cast<const float4*>(at);
    }
  }
  fp.mod     = tb.mod;
  fp.n       = nof_re;
  fp.seed    = tb.seed;
  fp.ports   = ports;
  fp.nof_rx  = nrx;
  fp.scaling = g->scaling;
  for (uint32_t k = 0; k < ports; k++) { // the combined symbols layer-demapped: layer k's symbol i is d[ports i + k]
    ep.x[k] = reinterpret_cast<float2*>(s.dev.get()) + k;
  }
  ep.x_stride = ports;
  ep.ports    = ports;
  ep.nof_rx   = nrx;
  ep.n        = nof_re;
  ep.scaling  = g->scaling;
  srsran_hip_sch_head_t head = {tb.max_nof_iterations, 0.f, tb.llr_is_8bit != 0};
  uint8_t *             p_d = s.pin + o_d, *p_e = s.pin + o_e, *dx = s.dev;
  const sch::FrontEnd   front = [=](hipStream_t st, void* d_e) mutable {
    modem::Params mp;
    if (!modem::params_for(mp, tb.llr_is_8bit ? modem::LLR_I8 : modem::LLR_I16)) {
      return false;
    }
    fp.out     = d_e;
    fp.x1_bits = mp.x1_bits;
    fp.x2_cols = mp.x2_cols;
    fp.k       = mp.k;
    if (txdiv::launch_front(fp, tb.llr_is_8bit != 0, st) != hipSuccess) {
      set_error("grant front end: transmit-diversity front-end launch failed");
      return false;
    }
    // what the reference leaves in q->d / q->e: the symbols exist in the front end's registers only, so the per-stage kernel makes them (same arithmetic)
    if (want_d && (txdiv::launch_eq(ep, st) != hipSuccess || hipMemcpyAsync(p_d, dx, (size_t)nof_re * sizeof(cf_t), hipMemcpyDeviceToHost, st) != hipSuccess)) {
      set_error("grant front end: the combined symbols could not be produced");
      return false;
    }
    if (want_e && hipMemcpyAsync(p_e, d_e, ne, hipMemcpyDeviceToHost, st) != hipSuccess) {
      set_error("grant front end: copy of the intermediate results failed");
      return false;
    }
    return true;
  };
  const bool ok = sch::decode_tb_staged(&head, softbuffer, &seg, 2 * Qm, tb.rv, nof_re * Qm, nullptr, &front, data);
  if (want_d) {
    memcpy(d_out, p_d, (size_t)nof_re * sizeof(cf_t));
  }
  if (want_e) {
    memcpy(e_out, p_e, ne);
  }
  res->crc_ok               = ok ? 1 : 0;
  res->avg_iterations_block = head.avg_iterations;
  return SRSRAN_SUCCESS;
}

// ---- PDSCH codeword with transmit diversity, transmit

extern "C" int srsran_hip_pdsch_encode_txdiv(const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* const symbols[])
{
  return srsran_hip_pdsch_encode_txdiv_multi(1, g, &softbuffer, &data, &symbols);
}

extern "C" int srsran_hip_pdsch_encode_txdiv_multi(uint32_t n, const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* const* softbuffers,
                                                   uint8_t* const* data, cf_t* const* const* symbols)
{
  TraceRange trace_("srsran_hip_pdsch_encode_txdiv");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !softbuffers || !data || !symbols) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_encode_txdiv: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t ports = g[i].nof_ports;
    bool           ok    = softbuffers[i] && symbols[i] && (ports == 2 || ports == 4);
    for (uint32_t k = 0; ok && k < ports; k++) {
      ok = symbols[i][k] != nullptr;
    }
    if (!ok || !(g[i].scaling != 0.f) || !std::isfinite(g[i].scaling)) {
      set_error("srsran_hip_pdsch_encode_txdiv: codeword %u: %u ports, scaling %g or a NULL argument", i, ports, (double)g[i].scaling);
      fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (!tb_valid(g[i].tb, "srsran_hip_pdsch_encode_txdiv")) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (g[i].tb.nof_re % ports) {
      set_error("srsran_hip_pdsch_encode_txdiv: codeword %u: %u REs are not whole groups of %u", i, g[i].tb.nof_re, ports);
      fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_encode_txdiv");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&                   s = *sp;
  std::vector<srsran_cbsegm_t> seg(n);
  std::vector<sch::TxItem>     items(n);
  std::vector<size_t>          o_out(n); // codeword i: nof_ports planes of al256(nof_re points) from here
  size_t                       out_bytes = 0, tiles = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!segment(&seg[i], g[i].tb.tbs)) {
      return SRSRAN_ERROR;
    }
    const uint32_t Qm = qm_of(g[i].tb.mod);
    items[i] = {softbuffers[i], &seg[i], 2 * Qm, g[i].tb.rv, g[i].tb.nof_re * Qm, data[i], 0};
    o_out[i] = out_bytes;
    out_bytes += g[i].nof_ports * al256((size_t)g[i].tb.nof_re * sizeof(cf_t));
    tiles += (g[i].tb.nof_re + MODEM_TILE_SYMS - 1) / MODEM_TILE_SYMS;
  }
  const size_t o_jobs = out_bytes, o_tj = al256(o_jobs + n * sizeof(txdiv::ModJob));
  if (out_bytes / sizeof(cf_t) > 0xffffffffull || !s.grow(al256(o_tj + tiles * sizeof(uint32_t)), 0)) {
    return SRSRAN_ERROR;
  }
  const sch::GroupBackEnd back = [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, uint32_t m) -> bool {
    modem::Params mp;
    const float2* tab = modem::mod_tables();
    if (m != n || !modem::params_for(mp, modem::LLR_I16) || !tab) {
      return false;
    }
    auto*    mj = reinterpret_cast<txdiv::ModJob*>(s.pin + o_jobs);
    auto*    tj = reinterpret_cast<uint32_t*>(s.pin + o_tj);
    uint32_t nt = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t cnt   = (g[i].tb.nof_re + MODEM_TILE_SYMS - 1) / MODEM_TILE_SYMS;
      const size_t   plane = al256((size_t)g[i].tb.nof_re * sizeof(cf_t));
      mj[i] = {g[i].tb.mod, g[i].tb.nof_re, g[i].tb.seed, g[i].nof_ports, txdiv_tx_scale(g[i].nof_ports, g[i].scaling), e_byte_off[i], {0, 0, 0, 0}, nt};
      for (uint32_t k = 0; k < g[i].nof_ports; k++) {
        mj[i].out_off[k] = (uint32_t)((o_out[i] + k * plane) / sizeof(cf_t));
      }
      for (uint32_t t = 0; t < cnt; t++) {
        tj[nt++] = i;
      }
    }
    txdiv::ModParams p = {d_e, reinterpret_cast<float2*>(s.pin.get()), tab, mj, tj, nt, mp.x1_bits, mp.x2_cols};
    if (txdiv::launch_mod(p, st) != hipSuccess) {
      set_error("transmit-diversity modulator launch failed");
      return false;
    }
    return true;
  };
  const int rc = sch::encode_tbs_staged(items.data(), n, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  for (uint32_t i = 0; i < n; i++) {
    const size_t plane = al256((size_t)g[i].tb.nof_re * sizeof(cf_t));
    for (uint32_t k = 0; k < g[i].nof_ports; k++) {
      memcpy(symbols[i][k], s.pin + o_out[i] + k * plane, (size_t)g[i].tb.nof_re * sizeof(cf_t));
    }
  }
  return SRSRAN_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ warm start
//
// The first grant of a process used to cost 20-28 ms (profiles/r03_ref_programs.json: pdsch_test -X 1): the device code of every kernel on the path is
// loaded at its first launch, the thread's staging contexts create their stream, pinned and device images, decoder and encoder objects, transform plans,
// and every (block size, redundancy version) brings its rate-matching table.  The reference does that kind of work in srsran_sch_init (sch.c:159-197:
// allocation, srsran_tdec_init, srsran_rm_turbo_gentables) -- so does the library: srsran_rm_turbo_gentables() builds every rate-matching table in
// one allocation and warms ONE worker's contexts; srsran_hip_warmup(n) makes that n.  A warm context is made by running real calls -- the largest
// grant of a 100-PRB cell, a one-block grant and a scalar-decoder grant, receive and transmit side, 16- and 8-bit soft bits -- on a short-lived
// thread whose contexts go back to the pools (hip_common.h: StagePool) when it ends.

#include <atomic>
#include <condition_variable>
#include <thread>

#include "srsran_amd/phy_nr_chan_abi.h"
#include "turbo_device.h"
namespace phyhip {
namespace rm {
bool build_all_tables(); // rm_host.cpp
}
} // namespace phyhip

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
      if (!llr8) { // transmit
        srsran_hip_pdsch_tx_t tx = {tb, 1.0f};
        (void)srsran_hip_pdsch_encode_dbg(&tx, &sb.tx, data.data(), sym.data(), qbits.data());
        (void)srsran_hip_ulsch_encode(&tb, nsymb, &sb.tx, data.data(), qbits.data());
      }
    }
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
