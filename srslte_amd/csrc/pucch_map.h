// pucch_map.h -- the PUCCH resource rules, restated once, as written: srsran_pucch_m / _n_prb (pucch.c:975-1015), srsran_pucch_alpha_format1 (:1150-1207, with
// the n_oc *= 2 / n_oc_div branch of the extended prefix for data and not for DMRS), srsran_pucch_alpha_format2 (:1210-1234, with its signed x), get_N_sf,
// get_pucch_symbol, srsran_pucch_n_cs_cell (:1018-1035), srsran_group_hopping_f_gh (phy_common.c:471-489), srsran_refsignal_dmrs_N_rs / _pucch_symbol and
// the float arguments of the orthogonal covers (pucch.c:211-217, refsignal_ul.c:46-51).  From a plan: the device job (pucch_device.h), and from the
// record a job leaves: the host's part of srsran_chest_ul_estimate_pucch and srsran_pucch_decode (the float expressions of the measurements, the
// thresholds).  Plain C++: pure host code, no device.
#pragma once
#include "pucch_device.h"
#include "srsran_amd/phy_pucch_abi.h"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace phyhip {
namespace pucch {

// TS 36.211 7.2: c(n) = x1(n + 1600) + x2(n + 1600), x1 from 1, x2 from c_init; n < len <= 1120
inline void gold(uint32_t c_init, uint32_t len, uint8_t* c)
{
  uint8_t a[1600 + 1120 + 31], b[1600 + 1120 + 31];
  for (int i = 0; i < 31; i++) {
    a[i] = i == 0;
    b[i] = (c_init >> i) & 1u;
  }
  for (uint32_t n = 0; n < 1600 + len; n++) {
    a[n + 31] = a[n + 3] ^ a[n];
    b[n + 31] = b[n + 3] ^ b[n + 2] ^ b[n + 1] ^ b[n];
  }
  for (uint32_t n = 0; n < len; n++) {
    c[n] = a[n + 1600] ^ b[n + 1600];
  }
}

inline bool is_f1(uint32_t format)
{
  return format <= SRSRAN_HIP_PUCCH_FORMAT_1B;
}

struct CellSeq { // what srsran_pucch_init_ / srsran_refsignal_ul_set_cell keep per cell
  uint32_t n_cs_cell[20][7];
  uint32_t f_gh[20];
};
inline void cell_seq(const srsran_hip_pucch_cell_t& cell, CellSeq& s)
{
  const uint32_t nsymb = cell.cp ? 6 : 7;
  uint8_t        c[8 * 7 * 20];
  memset(&s, 0, sizeof(s));
  gold(cell.id, 8 * nsymb * 20, c);
  for (uint32_t ns = 0; ns < 20; ns++) {
    for (uint32_t l = 0; l < nsymb; l++) {
      for (uint32_t i = 0; i < 8; i++) {
        s.n_cs_cell[ns][l] += (uint32_t)c[8 * nsymb * ns + 8 * l + i] << i;
      }
    }
  }
  gold(cell.id / 30, 160, c);
  for (uint32_t ns = 0; ns < 20; ns++) {
    for (uint32_t i = 0; i < 8; i++) {
      s.f_gh[ns] += (uint32_t)c[8 * ns + i] << i;
    }
  }
}

inline uint32_t pucch_m(const srsran_hip_pucch_job_t& j, bool ext)
{
  if (is_f1(j.format)) {
    uint32_t       m = j.n_rb_2;
    const uint32_t c = ext ? 2 : 3;
    if (j.n_pucch >= c * j.N_cs / j.delta_pucch_shift) {
      m = (j.n_pucch - c * j.N_cs / j.delta_pucch_shift) / (c * kNre / j.delta_pucch_shift) + j.n_rb_2 + (uint32_t)ceilf((float)j.N_cs / 8);
    }
    return m;
  }
  return j.n_pucch / kNre;
}

// srsran_pucch_alpha_format1: n_cs (alpha = 2 pi n_cs / 12), n_oc, n_prime(ns)
inline uint32_t n_cs_format1(const CellSeq& s, const srsran_hip_pucch_job_t& j, bool ext, bool is_dmrs, uint32_t ns, uint32_t l, uint32_t* n_oc_out, uint32_t* n_prime_ns)
{
  const uint32_t c = ext ? 2 : 3, edge = c * j.N_cs / j.delta_pucch_shift;
  const uint32_t N_prime = j.n_pucch < edge ? j.N_cs : kNre;
  uint32_t       n_prime = j.n_pucch;
  if (j.n_pucch >= edge) {
    n_prime = (j.n_pucch - edge) % (c * kNre / j.delta_pucch_shift);
  }
  if (ns % 2) {
    if (j.n_pucch >= edge) {
      n_prime = (c * (n_prime + 1)) % (c * kNre / j.delta_pucch_shift + 1) - 1;
    } else {
      const uint32_t d = ext ? 0 : 2;
      const uint32_t h = (n_prime + d) % (c * N_prime / j.delta_pucch_shift);
      n_prime          = (h / c) + (h % c) * N_prime / j.delta_pucch_shift;
    }
  }
  *n_prime_ns             = n_prime;
  const uint32_t n_oc_div = (!is_dmrs && ext) ? 2 : 1;
  uint32_t       n_oc     = (n_prime * j.delta_pucch_shift) / N_prime;
  if (!is_dmrs && ext) {
    n_oc *= 2;
  }
  *n_oc_out = n_oc;
  if (!ext) {
    return (s.n_cs_cell[ns][l] + (n_prime * j.delta_pucch_shift + (n_oc % j.delta_pucch_shift)) % N_prime) % kNre;
  }
  return (s.n_cs_cell[ns][l] + (n_prime * j.delta_pucch_shift + n_oc / n_oc_div) % N_prime) % kNre;
}

inline uint32_t n_cs_format2(const CellSeq& s, const srsran_hip_pucch_job_t& j, uint32_t ns, uint32_t l, uint32_t* n_prime_out)
{
  uint32_t n_prime = j.n_pucch % kNre;
  if (j.n_pucch >= kNre * j.n_rb_2) {
    n_prime = (j.n_pucch + j.N_cs + 1) % kNre;
  }
  if (ns % 2) {
    n_prime = (kNre * (n_prime + 1)) % (kNre + 1) - 1;
    if (j.n_pucch >= kNre * j.n_rb_2) {
      const int x = ((int)kNre - 2 - (int)j.n_pucch) % (int)kNre;
      n_prime     = x >= 0 ? (uint32_t)x : (uint32_t)((int)kNre + x);
    }
  }
  *n_prime_out = n_prime;
  return (s.n_cs_cell[ns][l] + n_prime) % kNre;
}

// nullptr, or why the job is refused.  `p` is zeroed first.  s: cell_seq(cell), made once for the jobs of a call
inline const char* plan(const srsran_hip_pucch_cell_t& cell, const CellSeq& s, const srsran_hip_pucch_sf_t& sf, const srsran_hip_pucch_job_t& j, srsran_hip_pucch_plan_t& p)
{
  static const uint32_t sym_f1[2][4] = {{0, 1, 5, 6}, {0, 1, 4, 5}}, sym_f2[2][5] = {{0, 2, 3, 4, 6}, {0, 1, 2, 4, 5}}; // pucch.c:206-209
  static const uint32_t rs_f1[2][3] = {{2, 3, 4}, {2, 3, 0}}, rs_f2[2][2] = {{1, 5}, {3, 0}};                           // refsignal_ul.c:53-56
  memset(&p, 0, sizeof(p));
  if (cell.nof_prb < 6 || cell.nof_prb > 110 || cell.cp > 1 || cell.id >= 504) {
    return "invalid cell";
  }
  if (j.format > SRSRAN_HIP_PUCCH_FORMAT_2B) {
    return "the format is not one of 1, 1A, 1B, 2, 2A, 2B";
  }
  const bool ext = cell.cp != 0;
  if (ext && j.format >= SRSRAN_HIP_PUCCH_FORMAT_2A) {
    return "formats 2A and 2B are not taken on the extended cyclic prefix";
  }
  if (!(j.delta_pucch_shift > 0 && j.delta_pucch_shift < 4 && j.N_cs < 8 && (j.N_cs % j.delta_pucch_shift) == 0 && j.n_rb_2 <= cell.nof_prb)) {
    return "srsran_pucch_cfg_isvalid refuses the configuration";
  }
  if (j.n_pucch >= 2048) { // n_PUCCH^(1) and n_PUCCH^(2) are below 2048 and 1186 (TS 36.213 10.1); keeps every product of the rules inside 32 bits
    return "n_pucch out of range";
  }
  const uint32_t m = pucch_m(j, ext);
  for (uint32_t ns = 0; ns < 2; ns++) {
    p.n_prb[ns] = (m + ns) % 2 ? cell.nof_prb - 1 - m / 2 : m / 2;
    if (p.n_prb[ns] >= cell.nof_prb) { // (cell.nof_prb - 1 - m / 2 wraps for m / 2 >= nof_prb, as there)
      memset(&p, 0, sizeof(p));
      return "n_prb is outside the cell";
    }
  }
  const bool f1 = is_f1(j.format);
  p.n_rs        = f1 ? (ext ? 2 : 3) : (j.format == SRSRAN_HIP_PUCCH_FORMAT_2 && ext ? 1 : 2);
  // encode_signal_format12 (pucch.c:419) calls srsran_pucch_alpha_format1 with is_dmrs = TRUE for the data symbols too: the n_oc *= 2 / n_oc_div branch of
  // the extended prefix is restated above and, as there, never taken by the receive side
  for (uint32_t slot = 0; slot < 2; slot++) {
    const uint32_t ns = 2 * (sf.tti % 10) + slot;
    p.u[slot]         = ((j.group_hopping_en ? s.f_gh[ns] : 0) + cell.id % 30) % 30;
    p.N_sf[slot]      = f1 ? (slot && sf.shortened ? 3 : 4) : 5;
    for (uint32_t i = 0; i < p.N_sf[slot]; i++) {
      const uint32_t l = f1 ? sym_f1[ext][i] : sym_f2[ext][i];
      p.sym[slot][i]   = l;
      p.n_cs[slot][i]  = f1 ? n_cs_format1(s, j, ext, true, ns, l, &p.n_oc[slot][i], &p.n_prime_ns[slot][i]) : n_cs_format2(s, j, ns, l, &p.n_prime_ns[slot][i]);
    }
    for (uint32_t i = 0; i < p.n_rs; i++) {
      const uint32_t l     = f1 ? rs_f1[ext][i] : rs_f2[j.format == SRSRAN_HIP_PUCCH_FORMAT_2 && ext][i];
      uint32_t       unused = 0;
      p.dmrs_sym[slot][i]  = l;
      p.dmrs_n_cs[slot][i] = f1 ? n_cs_format1(s, j, ext, true, ns, l, &p.dmrs_n_oc[slot][i], &unused) : n_cs_format2(s, j, ns, l, &unused);
    }
  }
  return nullptr;
}

// what of the job the device cannot take: the settings the plan does not read
inline const char* invalid_settings(const srsran_hip_pucch_job_t& j)
{
  if (j.filter_len != 0 && j.filter_len != 3) {
    return "filter_len is neither 0 nor 3";
  }
  for (uint32_t i = 0; i < j.filter_len; i++) {
    if (!std::isfinite(j.filter[i])) {
      return "a filter tap is not finite";
    }
  }
  if (j.format >= SRSRAN_HIP_PUCCH_FORMAT_2 && j.nof_uci_bits >= kWordBits) {
    return "nof_uci_bits above 12 (srsran_uci_decode_cqi_pucch refuses it)";
  }
  if (j.rnti > 0xffff) {
    return "rnti above 16 bits";
  }
  return nullptr;
}

// the device job of a planned resource.  phi: the caller's Table 5.5.1.2-1 as recovered by srsran_hip_pucch_set_tables
inline void device_job(const srsran_hip_pucch_cell_t& cell, const srsran_hip_pucch_sf_t& sf, const srsran_hip_pucch_job_t& j, const srsran_hip_pucch_plan_t& p,
                       const int8_t phi[30][12], bool decode, Job& d)
{
  // pucch.c:211-217 and refsignal_ul.c:46-51: float tables there
  static const float w_n_oc[2][3][4] = {{{0, 0, 0, 0}, {0, (float)M_PI, 0, (float)M_PI}, {0, (float)M_PI, (float)M_PI, 0}},
                                        {{0, 0, 0, 0}, {0, (float)(2 * M_PI / 3), (float)(4 * M_PI / 3), 0}, {0, (float)(4 * M_PI / 3), (float)(2 * M_PI / 3), 0}}};
  static const float w_arg_f1_norm[3][3] = {{0, 0, 0}, {0, (float)(2 * M_PI / 3), (float)(4 * M_PI / 3)}, {0, (float)(4 * M_PI / 3), (float)(2 * M_PI / 3)}};
  static const float w_arg_f1_ext[3][2]  = {{0, 0}, {0, (float)M_PI}, {0, 0}};
  const bool         ext = cell.cp != 0, f1 = is_f1(j.format);
  memset(&d, 0, sizeof(d));
  d.format = j.format;
  d.nsymb  = ext ? 6 : 7;
  d.n_rs   = p.n_rs;
  for (uint32_t s = 0; s < 2; s++) {
    d.N_sf[s] = p.N_sf[s];
    for (uint32_t i = 0; i < p.N_sf[s]; i++) {
      d.sym[s][i]   = p.sym[s][i];
      d.alpha[s][i] = (float)(2 * M_PI * (p.n_cs[s][i]) / kNre);
      if (f1) {
        float S_ns = 0;
        if (p.n_prime_ns[s][i] % 2) {
          S_ns = (float)(M_PI / 2);
        }
        d.w_data[s][i] = w_n_oc[p.N_sf[s] == 3 ? 1 : 0][p.n_oc[s][i] % 3][i] + S_ns;
      }
    }
    for (uint32_t i = 0; i < p.n_rs; i++) {
      d.dmrs_sym[s][i]   = p.dmrs_sym[s][i];
      d.dmrs_alpha[s][i] = (float)(2 * M_PI * (p.dmrs_n_cs[s][i]) / kNre);
      d.w_dmrs[s][i]     = f1 ? (ext ? w_arg_f1_ext[p.dmrs_n_oc[s][i]][i] : w_arg_f1_norm[p.dmrs_n_oc[s][i]][i]) : 0.0f;
    }
    for (uint32_t k = 0; k < kNre; k++) {
      d.phi_arg[s][k] = (float)phi[p.u[s]][k] * (float)M_PI_4; // srsran_vec_sc_prod_fcc(phi, M_PI_4, .)
    }
  }
  if (!f1) {
    uint8_t c[kBits2];
    gold(((((2 * (sf.tti % 10)) / 2 + 1) * (2 * cell.id + 1)) << 16) + j.rnti, kBits2, c); // srsran_sequence_pucch, sequences.c:169-172
    for (uint32_t i = 0; i < kBits2; i++) {
      d.scramble |= (uint32_t)c[i] << i;
    }
  }
  d.nof_uci_bits   = j.nof_uci_bits;
  d.filter_len     = j.filter_len;
  d.filter[0]      = j.filter[0];
  d.filter[1]      = j.filter[1];
  d.filter[2]      = j.filter[2];
  d.threshold_dmrs = j.threshold_dmrs_detection;
  d.dmrs_detection = std::isnormal(j.threshold_dmrs_detection) ? 1 : 0;
  d.decode         = decode ? 1 : 0;
}

// chest_ul.c:482-521, :565-574 and pucch.c:640-728, :843-866 from the record
inline void finish(const srsran_hip_pucch_job_t& j, uint32_t n_rs, const Record& r, bool decode, srsran_hip_pucch_res_t& o)
{
  memset(&o, 0, sizeof(o));
  float rsrp_avg = 0.0f;
  for (uint32_t i = 0; i < 2 * n_rs; i++) { // the same whole-row sum, added 2 n_rs times
    const float re = r.pe_sum[0] / (float)kNre, im = r.pe_sum[1] / (float)kNre;
    rsrp_avg += re * re + im * im;
  }
  rsrp_avg /= (float)(2 * n_rs);
  o.epre      = r.epre;
  o.epre_dBfs = 10.0f * log10f(o.epre);
  o.rsrp      = rsrp_avg < r.epre ? rsrp_avg : r.epre; // SRSRAN_MIN
  o.rsrp_dBfs = 10.0f * log10f(o.rsrp);
  if (j.meas_ta_en) {
    float ta_err = 0.0f;
    for (uint32_t i = 0; i < 2 * n_rs; i++) {
      ta_err += (float)(-atan2f(r.ta[i][1], r.ta[i][0]) * M_1_PI * 0.5f) / (float)(2 * n_rs); // vector_simd.c:1783
    }
    if (std::isnormal(ta_err)) {
      ta_err /= 15e3f;
      ta_err *= 1e6f;
      o.ta_us = roundf(ta_err * 10.0f) / 10.0f;
    }
  }
  o.noise_estimate     = r.noise_estimate;
  o.noise_estimate_dbm = 10.0f * log10f(o.noise_estimate) + 30.0f;
  if (std::isnormal(o.noise_estimate)) {
    o.snr    = o.rsrp / o.noise_estimate;
    o.snr_db = 10.0f * log10f(o.snr);
  } else {
    o.snr = o.snr_db = NAN;
  }
  o.drs_bits[0] = (uint8_t)(r.drs % 2);
  o.drs_bits[1] = (uint8_t)(r.drs / 2);
  if (!decode) {
    return;
  }
  o.dmrs_correlation = r.dmrs_correlation;
  if (r.early) { // correlation 0, not detected, the bits untouched
    return;
  }
  switch (j.format) {
    case SRSRAN_HIP_PUCCH_FORMAT_1:
      o.correlation = r.correlation;
      o.detected    = o.correlation >= j.threshold_format1;
      break;
    case SRSRAN_HIP_PUCCH_FORMAT_1A:
    case SRSRAN_HIP_PUCCH_FORMAT_1B:
      o.correlation = r.correlation;
      o.detected    = o.correlation > j.threshold_format1;
      if (j.format == SRSRAN_HIP_PUCCH_FORMAT_1A) {
        o.pucch_bits[0] = (uint8_t)(r.word & 1u);
      } else {
        o.pucch_bits[0] = (uint8_t)((r.word >> 1) & 1u);
        o.pucch_bits[1] = (uint8_t)(r.word & 1u);
      }
      o.ack_valid = o.correlation > j.threshold_data_valid_format1a;
      break;
    default:
      if (std::isnormal(r.llr_pow)) {
        const float llr_rms = sqrtf(r.llr_pow) * (float)kBits2;
        o.correlation       = ((float)(int16_t)r.max_corr) / llr_rms; // the decoder returns int16_t
      }
      for (uint32_t n = 0; n < kWordBits; n++) {
        o.pucch_bits[n] = (uint8_t)((r.word >> (kWordBits - 1 - n)) & 1u); // srsran_bit_unpack
      }
      o.detected  = o.correlation > j.threshold_data_valid_format2;
      o.ack_valid = (uint8_t)o.detected;
      break;
  }
}

} // namespace pucch
} // namespace phyhip
