// chest_ul.h -- what the PUSCH channel estimator's kernel (chest_ul_kernels.hip) and its two callers (the stage call and the _est grant calls, chan_host.cpp)
// share: the job and the record of one grant, and the host's part of srsran_chest_ul_estimate_pusch (chest_ul.c:291-368) -- arg(), the rounding, the
// NAN / isnormal rules and the dB conversions, from the record, after the call's host wait.  Plain C++: no HIP header.
#pragma once
#include "srsran_amd/phy_chan_abi.h"

#include <cmath>
#include <cstdint>

namespace phyhip {
namespace chest_ul {

#define CHEST_UL_MAX_REFS 1296u // 12 L_prb, L_prb <= 108 (srsran_dft_precoding_valid_prb below 110)

// one grant = one workgroup.  Offsets in points (cf_t) from the launch's `in` / `out`.  The output is rows of n points: rows[0] rows of slot 0's
// estimate from row row0[0], rows[1] of slot 1's from row row0[1] (a grant call: every data symbol of the slot, in pusch_get order; the stage: one each).
struct Job {
  uint32_t n;        // references per slot: 12 L_prb
  uint32_t o_rx;     // the two received reference rows, slot 0 then slot 1: 2 n points
  uint32_t o_r;      // the grant's DMRS row: 2 n points
  uint32_t o_out;    // first point of the grant's rows
  uint32_t row0[2];
  uint32_t rows[2];
  uint32_t filter_len; // 0 or 3
  float    filter[3];
  uint32_t end_pair; // the equaliser job's (modem::EqJob), passed through with the noise estimate
};

// what the kernel leaves per grant (pinned image: read after the host wait)
struct Record {
  float noise_estimate; // calibrated (chest_ul.c:211-219); 0 without smoothing
  float rx_power;       // srsran_vec_avg_power_cf over the 2 n received references
  float cfo[2];         // sum ls[0][k] conj(ls[1][k]): re, im
  float ta[2][2];       // per slot: sum ls[k] conj(ls[k - 1]), k >= 1: re, im
};

// chest_ul.c:300-326, :358-367 and vector_simd.c:1783 from the record
inline void finish(const Record& r, bool meas_ta_en, srsran_hip_chest_ul_res_t* o)
{
  o->cfo_hz   = atan2f(r.cfo[1], r.cfo[0]) / (2.0f * (float)M_PI * 0.0005f);
  float ta_err = 0.0f;
  if (meas_ta_en) {
    for (int i = 0; i < 2; i++) {
      ta_err += (float)(-atan2f(r.ta[i][1], r.ta[i][0]) * M_1_PI * 0.5f) / 2;
    }
  }
  if (std::isnormal(ta_err)) {
    ta_err /= 15e3f;
    ta_err *= 1e6f;
    ta_err   = roundf(ta_err * 10.0f) / 10.0f;
    o->ta_us = ta_err;
  } else {
    o->ta_us = 0.0f;
  }
  o->noise_estimate     = r.noise_estimate;
  o->snr                = std::isnormal(r.noise_estimate) ? r.rx_power / r.noise_estimate : NAN;
  o->snr_db             = 10.0f * log10f(o->snr);
  o->noise_estimate_dbm = 10.0f * log10f(o->noise_estimate) + 30.0f;
}

// nullptr, or why the estimator's description is refused
inline const char* invalid(const srsran_hip_chest_ul_t* est)
{
  if (!est || !est->r) {
    return "NULL est or est->r";
  }
  if (est->filter_len != 0 && est->filter_len != 3) {
    return "filter_len is neither 0 nor 3";
  }
  for (uint32_t i = 0; i < est->filter_len; i++) {
    if (!std::isfinite(est->filter[i])) {
      return "a filter tap is not finite";
    }
  }
  return nullptr;
}

} // namespace chest_ul
} // namespace phyhip
