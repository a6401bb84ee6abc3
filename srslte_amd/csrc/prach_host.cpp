// prach_host.cpp -- random-access detection in one device call (include/srsran_amd/phy_prach_abi.h): the plan of a cell (srsran_prach_set_cell_ and
// srsran_prach_gen_seqs, prach.c:359-460, 528-654, restated as written), the handle with the root spectra, and the detection calls.  A call is one round trip
// (call_frame.h) with the two launches of prach_kernels.hip on the calling thread's staging context; the decisions of
// srsran_prach_process (:830-859) are taken here from the records that came down.  One layout serves the pinned image and the device buffer:
//   [the first N_ifft_prach samples of every occasion || the roots' records | prach_bins | corr] and, on the device alone, the first stage's streams
// what is in front of || goes up, what is behind comes down (the last two only for the _dbg call).
#include "call_frame.h"
#include "prach_device.h"
#include "tables/lte_prach_tables.h"
#include "srsran_amd/phy_prach_abi.h"

#include <cmath>
#include <complex>

using namespace phyhip;

extern "C" int srsran_symbol_sz(uint32_t nof_prb);

static_assert(sizeof(srsran_hip_prach_cfg_t) == 32 && sizeof(srsran_hip_prach_info_t) == 548 && sizeof(srsran_hip_prach_occ_t) == 16 &&
                  sizeof(srsran_hip_prach_res_t) == 1540 && sizeof(srsran_hip_prach_dbg_t) == 48,
              "phy_prach_abi.h layout");
static_assert(prach::kNzc == SRSRAN_HIP_PRACH_N_ZC && prach::kMaxOcc == SRSRAN_HIP_PRACH_MAX_OCC, "phy_prach_abi.h constants");

struct srsran_hip_prach {
  DeviceTag               tag;
  srsran_hip_prach_cfg_t  cfg;
  srsran_hip_prach_info_t info;
  float                   detect_factor;
  DeviceBuf               tab; // [tw_first | tw_n (both double) | tw_zc | root spectra]; what create alone needs lies behind
  size_t                  o_tw_n, o_tw_zc, o_spec;
};

namespace {

constexpr uint32_t kDetectFactor = 18; // PRACH_DETECT_FACTOR
constexpr uint32_t kDeltaF = 15000, kDeltaFRa = 1250, kPhi = 7, kRbSc = 12;

struct PrachStage : call::Stage {};

PrachStage& prach_stage() // of the calling thread, on the device it is bound to
{
  static thread_local StageRef<PrachStage> r;
  return r.get();
}

// Table 5.7.2-4 as the application handed it in (srsran_hip_prach_set_root_order): process-wide, copied under the lock
std::mutex g_order_mu;
uint32_t   g_order[838];
bool       g_have_order = false;

// srsran_prach_set_cell_ and srsran_prach_gen_seqs; nullptr, or why the configuration is refused
const char* plan(const srsran_hip_prach_cfg_t& c, srsran_hip_prach_info_t& p)
{
  memset(&p, 0, sizeof(p));
  if (c.nof_prb != 6 && c.nof_prb != 15 && c.nof_prb != 25 && c.nof_prb != 50 && c.nof_prb != 75 && c.nof_prb != 100) {
    return "nof_prb is not 6, 15, 25, 50, 75 or 100";
  }
  const uint32_t N_ifft_ul = (uint32_t)srsran_symbol_sz(c.nof_prb);
  if (N_ifft_ul >= 2049 || N_ifft_ul % 128 != 0) {
    return "N_ifft_ul is not a multiple of 128 up to 2048";
  }
  if (c.config_idx >= 64) { // the reference's format is config_idx / 16: what it accepts is format 0 .. 3
    return "config_idx out of range";
  }
  if (c.root_seq_idx >= 838) {
    return "root_seq_idx out of range";
  }
  if (c.zero_corr_zone >= (c.hs_flag ? 15u : 16u)) {
    return c.hs_flag ? "invalid zero_corr_zone for the restricted set" : "invalid zero_corr_zone";
  }
  uint32_t order[838];
  {
    std::lock_guard<std::mutex> lk(g_order_mu);
    if (!g_have_order) {
      return "the logical root order has not been set (srsran_hip_prach_set_root_order)";
    }
    memcpy(order, g_order, sizeof(order));
  }
  const uint32_t f = c.config_idx / 16;
  p.N_zc           = prach::kNzc;
  p.N_cs           = c.hs_flag ? prach::kPrachNcsRestricted[c.zero_corr_zone] : prach::kPrachNcsUnrestricted[c.zero_corr_zone];
  // gen_seqs, :359-460: the variables of the restricted-set branch live across roots, as there
  uint32_t u = 0, v = 1, p_ = 0, d_u = 0, d_start = 0, N_shift = 0, N_group = 0;
  int      v_max = 0, N_neg_shift = 0;
  for (int i = 0; i < 64; i++) {
    if (v > (uint32_t)v_max) {
      u                           = order[(c.root_seq_idx + p.N_roots) % 838];
      p.root_u[p.N_roots]         = u;
      p.root_seqs_idx[p.N_roots++] = (uint32_t)i;
      if (c.hs_flag) {
        for (p_ = 1; p_ <= p.N_zc; p_++) {
          if (((p_ * u) % p.N_zc) == 1) {
            break;
          }
        }
        d_u = p_ < p.N_zc / 2 ? p_ : p.N_zc - p_;
        if (d_u >= p.N_cs && d_u < p.N_zc / 3) {
          N_shift = d_u / p.N_cs;
          d_start = 2 * d_u + N_shift * p.N_cs;
          N_group = p.N_zc / d_start;
          if (p.N_zc > 2 * d_u + N_group * d_start) {
            N_neg_shift = (int)((p.N_zc - 2 * d_u - N_group * d_start) / p.N_cs);
          } else {
            N_neg_shift = 0;
          }
        } else if (p.N_zc / 3 <= d_u && d_u <= (p.N_zc - p.N_cs) / 2) {
          N_shift = (p.N_zc - 2 * d_u) / p.N_cs;
          d_start = p.N_zc - 2 * d_u + N_shift * p.N_cs;
          N_group = d_u / d_start;
          if (d_u > N_group * d_start) {
            N_neg_shift = (int)((d_u - N_group * d_start) / p.N_cs);
          } else {
            N_neg_shift = 0;
          }
          if (N_neg_shift > (int)N_shift) {
            N_neg_shift = (int)N_shift;
          }
        } else {
          N_shift = 0; // N_group and N_neg_shift keep the last root's values, :420-423
        }
        v_max = (int)(N_shift * N_group + (uint32_t)N_neg_shift - 1);
        if (v_max < 0) {
          v_max = 0;
        }
      } else {
        v_max = p.N_cs == 0 ? 0 : (int)(p.N_zc / p.N_cs) - 1;
      }
      v = 0;
    }
    v++;
  }
  p.num_ra_preambles = c.num_ra_preambles;
  if (p.num_ra_preambles < 4 || p.num_ra_preambles > p.N_roots) { // :602: compared with the number of ROOTS
    p.num_ra_preambles = p.N_roots;
  }
  p.N_ifft_ul    = N_ifft_ul;
  p.N_ifft_prach = N_ifft_ul * kDeltaF / kDeltaFRa;
  p.N_seq        = prach::kPrachTseq[f] * N_ifft_ul / 2048;
  p.N_cp         = prach::kPrachTcp[f] * N_ifft_ul / 2048;
  p.n_wins       = p.N_zc / (p.N_cs ? p.N_cs : p.N_zc);
  return nullptr;
}

template <class T>
std::vector<std::complex<T>> twiddles(int N) // e^{-j 2 pi i / N}
{
  std::vector<std::complex<T>> tw(N);
  for (int i = 0; i < N; i++) {
    const double a = -2.0 * M_PI * (double)i / (double)N;
    tw[i]          = std::complex<T>((T)cos(a), (T)sin(a));
  }
  return tw;
}

// srsran_prach_calculate_time_offset_secs, :750-760
float phase_offset_secs(const srsran_hip_prach_info_t& p, float cross_re, float cross_im)
{
  const float freq_domain_phase = atan2f(cross_im, cross_re); // cargf
  const float ratio             = (float)(p.N_ifft_ul * kDeltaF) / (float)(SRSRAN_HIP_PRACH_N_ZC * kDeltaFRa);
  const float num_samples       = roundf((float)((ratio * freq_domain_phase * p.N_zc) / (2 * M_PI)));
  return num_samples / ((float)p.N_ifft_ul * kDeltaF);
}

struct Out {
  uint32_t* indices;
  float*    t_offsets;
  float*    peak_to_avg;
  uint32_t  max_det;
  uint32_t* n_indices;
};

// srsran_prach_process, :787-861, on the records of one occasion
void decide(const srsran_hip_prach& h, const uint32_t* rec, uint32_t rec_words, const Out& o)
{
  const srsran_hip_prach_info_t& p = h.info;
  uint32_t                       n = 0;
  for (uint32_t i = 0; i < p.num_ra_preambles; i++) {
    const uint32_t* r = rec + (size_t)i * rec_words;
    float           corr_ave, cre, cim, max_peak = 0;
    memcpy(&corr_ave, r, 4);
    memcpy(&cre, r + 1, 4);
    memcpy(&cim, r + 2, 4);
    const float*    peak_values  = reinterpret_cast<const float*>(r + prach::kRecHead);
    const uint32_t* peak_offsets = r + prach::kRecHead + p.n_wins;
    for (uint32_t j = 0; j < p.n_wins; j++) {
      if (peak_values[j] > max_peak) {
        max_peak = peak_values[j];
      }
    }
    if (max_peak > (h.detect_factor * corr_ave)) {
      for (uint32_t j = 0; j < p.n_wins; j++) {
        if (peak_values[j] > h.detect_factor * corr_ave && n < o.max_det) {
          o.indices[n] = (i * p.n_wins) + j;
          if (o.peak_to_avg) {
            o.peak_to_avg[n] = peak_values[j] / corr_ave;
          }
          if (o.t_offsets) {
            o.t_offsets[n] =
                h.cfg.freq_domain_offset_calc ? phase_offset_secs(p, cre, cim) : (float)peak_offsets[j] / (float)(kDeltaFRa * p.N_zc); // :742-746
          }
          n++;
        }
      }
    }
  }
  *o.n_indices = n;
}

// n occasions in one call
int run(const char* who, srsran_hip_prach* h, uint32_t n, const srsran_hip_prach_occ_t* occ, const Out* out, const srsran_hip_prach_dbg_t* dbg)
{
  TraceRange  trace_(who);
  const char* why = nullptr;
  if (!h) {
    return call::refused(who, "NULL handle");
  }
  const srsran_hip_prach_info_t& p = h->info;
  for (uint32_t o = 0; !why && o < n; o++) {
    if (!occ[o].signal) {
      why = "NULL signal";
    } else if (occ[o].sig_len < p.N_ifft_prach) {
      why = "the signal is shorter than N_ifft_prach";
    } else if (6 + (uint64_t)occ[o].freq_offset > h->cfg.nof_prb) {
      why = "no space for the PRACH at this freq_offset";
    }
  }
  if (why) {
    return call::refused(who, why);
  }
  PHY_DEV_GUARD(h->tag, who, SRSRAN_ERROR);
  PrachStage& s = prach_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  const uint32_t N = p.N_ifft_prach, D = N / prach::kFirst, R = p.num_ra_preambles, rec_words = prach::kRecHead + 2 * p.n_wins;
  const size_t   up = al256((size_t)n * N * sizeof(cf_t)), o_bins = al256(up + (size_t)n * R * rec_words * 4);
  const size_t   o_corr = al256(o_bins + (dbg ? (size_t)n * prach::kNzc * sizeof(cf_t) : 0));
  const size_t   down = al256(o_corr + (dbg ? (size_t)n * R * prach::kNzc * 4 : 0)), end = down + (size_t)n * D * prach::kNzc * sizeof(double2);
  if (!s.grow(down, end)) {
    return call::failed(who, "the staging allocation failed");
  }
  prach::Params k = {};
  for (uint32_t o = 0; o < n; o++) {
    memcpy(s.pin + (size_t)o * N * sizeof(cf_t), occ[o].signal, (size_t)N * sizeof(cf_t));
    const uint32_t k_0   = occ[o].freq_offset * kRbSc - h->cfg.nof_prb * kRbSc / 2 + p.N_ifft_ul / 2; // :896-898
    const uint32_t K     = kDeltaF / kDeltaFRa;
    const uint32_t begin = kPhi + (K * k_0) + (K / 2);
    k.k0[o]              = (int)((begin + N / 2) % N);
  }
  k.sig       = reinterpret_cast<const float2*>(s.dev.get());
  k.streams   = reinterpret_cast<double2*>(s.dev + down);
  k.tw_first  = reinterpret_cast<const double2*>(h->tab.get());
  k.tw_n      = reinterpret_cast<const double2*>(h->tab + h->o_tw_n);
  k.tw_zc     = reinterpret_cast<const float2*>(h->tab + h->o_tw_zc);
  k.root_spec = reinterpret_cast<const float2*>(h->tab + h->o_spec);
  k.rec       = reinterpret_cast<uint32_t*>(s.dev + up);
  k.bins_out  = dbg ? reinterpret_cast<float2*>(s.dev + o_bins) : nullptr;
  k.corr_out  = dbg ? reinterpret_cast<float*>(s.dev + o_corr) : nullptr;
  k.N         = (int)N;
  k.D         = (int)D;
  k.n_occ     = (int)n;
  k.n_search  = (int)R;
  k.n_wins    = (int)p.n_wins;
  k.N_cs      = (int)p.N_cs;
  k.rec_words = (int)rec_words;
  k.norm      = 1.0 / sqrt((double)N);
  if (!call::round_trip(who, s.st, s.pin, s.dev, (size_t)n * N * sizeof(cf_t), up, down - up, [&](hipStream_t st) { return prach::launch(k, st); })) {
    return SRSRAN_ERROR;
  }
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(s.pin + up);
  for (uint32_t o = 0; o < n; o++) {
    decide(*h, rec + (size_t)o * R * rec_words, rec_words, out[o]);
  }
  if (dbg) { // one occasion
    if (dbg->prach_bins) {
      memcpy(dbg->prach_bins, s.pin + o_bins, prach::kNzc * sizeof(cf_t));
    }
    if (dbg->corr) {
      memcpy(dbg->corr, s.pin + o_corr, (size_t)R * prach::kNzc * 4);
    }
    for (uint32_t i = 0; i < R; i++) {
      const uint32_t* r = rec + (size_t)i * rec_words;
      if (dbg->corr_ave) {
        memcpy(&dbg->corr_ave[i], r, 4);
      }
      if (dbg->cross_sum) {
        memcpy(&dbg->cross_sum[i], r + 1, 8);
      }
      if (dbg->peak_values) {
        memcpy(&dbg->peak_values[(size_t)i * p.n_wins], r + prach::kRecHead, 4 * p.n_wins);
      }
      if (dbg->peak_offsets) {
        memcpy(&dbg->peak_offsets[(size_t)i * p.n_wins], r + prach::kRecHead + p.n_wins, 4 * p.n_wins);
      }
    }
  }
  return SRSRAN_SUCCESS;
}

int detect(const char* who, srsran_hip_prach_t* h, uint32_t freq_offset, const cf_t* signal, uint32_t sig_len, uint32_t* indices, float* t_offsets,
           float* peak_to_avg, uint32_t max_det, uint32_t* n_indices, const srsran_hip_prach_dbg_t* dbg)
{
  if (n_indices) {
    *n_indices = 0;
  }
  if (!h || !signal || !indices || !n_indices) {
    return call::refused(who, "NULL argument");
  }
  if (max_det == 0) {
    return call::refused(who, "max_det is 0");
  }
  const srsran_hip_prach_occ_t occ = {freq_offset, sig_len, signal};
  const Out                    out = {indices, t_offsets, peak_to_avg, max_det, n_indices};
  return run(who, h, 1, &occ, &out, dbg);
}

} // namespace

extern "C" int srsran_hip_prach_set_root_order(const uint32_t* order)
{
  std::lock_guard<std::mutex> lk(g_order_mu);
  if (!order) {
    g_have_order = false;
    return SRSRAN_SUCCESS;
  }
  bool seen[839] = {};
  for (int i = 0; i < 838; i++) {
    if (order[i] < 1 || order[i] > 838 || seen[order[i]]) {
      return call::refused("srsran_hip_prach_set_root_order", "not a permutation of 1 .. 838");
    }
    seen[order[i]] = true;
  }
  memcpy(g_order, order, sizeof(g_order));
  g_have_order = true;
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_prach_plan(const srsran_hip_prach_cfg_t* cfg, srsran_hip_prach_info_t* info)
{
  if (info) {
    memset(info, 0, sizeof(*info));
  }
  if (!cfg || !info) {
    return call::refused("srsran_hip_prach_plan", "NULL argument");
  }
  const char* why = plan(*cfg, *info);
  if (why) {
    memset(info, 0, sizeof(*info));
    return call::refused("srsran_hip_prach_plan", why);
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_prach_create(srsran_hip_prach_t** hp, const srsran_hip_prach_cfg_t* cfg)
{
  const char* who = "srsran_hip_prach_create";
  if (hp) {
    *hp = nullptr;
  }
  if (!hp || !cfg) {
    return call::refused(who, "NULL argument");
  }
  srsran_hip_prach_info_t info;
  const char*             why = plan(*cfg, info);
  if (why) {
    return call::refused(who, why);
  }
  PrachStage& s = prach_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  srsran_hip_prach* h = new srsran_hip_prach;
  h->cfg              = *cfg;
  h->info             = info;
  h->detect_factor    = cfg->detect_factor != 0.0f ? cfg->detect_factor : (float)kDetectFactor;
  const uint32_t N = info.N_ifft_prach, R = info.num_ra_preambles;
  h->o_tw_n           = al256(prach::kFirst * sizeof(double2));
  h->o_tw_zc          = al256(h->o_tw_n + (size_t)N * sizeof(double2));
  h->o_spec           = al256(h->o_tw_zc + prach::kNzc * sizeof(cf_t));
  const size_t o_seq  = al256(h->o_spec + (size_t)R * prach::kNzc * sizeof(cf_t)), end = o_seq + (size_t)R * prach::kNzc * sizeof(cf_t);
  std::vector<uint8_t> img(end, 0);
  const auto put = [&](size_t at, const auto& v) { memcpy(img.data() + at, v.data(), v.size() * sizeof(v[0])); };
  put(0, twiddles<double>(prach::kFirst));
  put(h->o_tw_n, twiddles<double>((int)N));
  put(h->o_tw_zc, twiddles<float>(prach::kNzc));
  // prach_cexp, :73-100: the table is cexpf of the float image of -2 pi i / 1678
  std::vector<std::complex<float>> lut(2 * prach::kNzc), seq((size_t)R * prach::kNzc);
  for (int i = 0; i < 2 * prach::kNzc; i++) {
    const float a = (float)(-(2.0f * M_PI * (float)i / (float)(2 * prach::kNzc)));
    lut[i]        = std::complex<float>(cosf(a), sinf(a));
  }
  for (uint32_t r = 0; r < R; r++) {
    for (uint32_t j = 0; j < (uint32_t)prach::kNzc; j++) {
      seq[(size_t)r * prach::kNzc + j] = lut[(info.root_u[r] * j * (j + 1)) % (2 * prach::kNzc)];
    }
  }
  put(o_seq, seq);
  int rc = SRSRAN_SUCCESS;
  if (!h->tab.grow(end)) {
    rc = call::failed(who, "the device allocation failed");
  } else {
    hipError_t e = upload(h->tab, img.data(), end);
    if (e == hipSuccess) { // get_precoded_dft, :346-357: forward, norm, no mirror
      e = call::settle(prach::launch_root_spectra(reinterpret_cast<const float2*>(h->tab + o_seq), reinterpret_cast<float2*>(h->tab + h->o_spec), (int)R, s.st), s.st);
    }
    if (e != hipSuccess) {
      set_error("%s: %s", who, hipGetErrorString(e));
      fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
      rc = SRSRAN_ERROR;
    }
  }
  if (rc != SRSRAN_SUCCESS) {
    delete h;
    return rc;
  }
  *hp = h;
  return SRSRAN_SUCCESS;
}

extern "C" void srsran_hip_prach_destroy(srsran_hip_prach_t* h)
{
  delete h;
}

extern "C" int srsran_hip_prach_info(const srsran_hip_prach_t* h, srsran_hip_prach_info_t* info)
{
  if (!h || !info) {
    return call::refused("srsran_hip_prach_info", "NULL argument");
  }
  *info = h->info;
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_prach_root_spectrum(srsran_hip_prach_t* h, uint32_t i, cf_t out[SRSRAN_HIP_PRACH_N_ZC])
{
  const char* who = "srsran_hip_prach_root_spectrum";
  if (!h || !out) {
    return call::refused(who, "NULL argument");
  }
  if (i >= h->info.num_ra_preambles) {
    return call::refused(who, "root index beyond the roots searched");
  }
  PHY_DEV_GUARD(h->tag, who, SRSRAN_ERROR);
  bind_thread();
  PHY_HIP_CHECK(hipMemcpy(out, h->tab + h->o_spec + (size_t)i * prach::kNzc * sizeof(cf_t), prach::kNzc * sizeof(cf_t), hipMemcpyDeviceToHost), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_prach_detect_offset(srsran_hip_prach_t* h, uint32_t freq_offset, const cf_t* signal, uint32_t sig_len, uint32_t* indices,
                                              float* t_offsets, float* peak_to_avg, uint32_t max_det, uint32_t* n_indices)
{
  return detect("srsran_hip_prach_detect_offset", h, freq_offset, signal, sig_len, indices, t_offsets, peak_to_avg, max_det, n_indices, nullptr);
}

extern "C" int srsran_hip_prach_detect_offset_dbg(srsran_hip_prach_t* h, uint32_t freq_offset, const cf_t* signal, uint32_t sig_len, uint32_t* indices,
                                                  float* t_offsets, float* peak_to_avg, uint32_t max_det, uint32_t* n_indices,
                                                  const srsran_hip_prach_dbg_t* dbg)
{
  const char* who = "srsran_hip_prach_detect_offset_dbg";
  if (!dbg) {
    if (n_indices) {
      *n_indices = 0;
    }
    return call::refused(who, "NULL argument");
  }
  return detect(who, h, freq_offset, signal, sig_len, indices, t_offsets, peak_to_avg, max_det, n_indices, dbg);
}

extern "C" int srsran_hip_prach_detect_multi(srsran_hip_prach_t* h, uint32_t n, const srsran_hip_prach_occ_t* occ, srsran_hip_prach_res_t* res)
{
  const char* who = "srsran_hip_prach_detect_multi";
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (n > SRSRAN_HIP_PRACH_MAX_OCC) {
    return call::refused(who, "more than 8 occasions");
  }
  if (res) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  if (!h || !occ || !res) {
    return call::refused(who, "NULL argument");
  }
  Out out[SRSRAN_HIP_PRACH_MAX_OCC];
  for (uint32_t o = 0; o < n; o++) {
    out[o] = {res[o].indices, res[o].t_offsets, res[o].peak_to_avg, SRSRAN_HIP_PRACH_MAX_DET, &res[o].n_indices};
  }
  return run(who, h, n, occ, out, nullptr);
}
