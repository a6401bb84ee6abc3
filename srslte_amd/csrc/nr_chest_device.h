// nr_chest_device.h -- jobs, records and launchers of nr_chest_kernels.hip: the NR shared channels' DMRS estimator (srsran_dmrs_sch_estimate,
// dmrs_sch.c:763-986) and RE extraction (srsran_pdsch_nr_cp, pdsch_nr.c:225-270) for the codewords of a call, and the host's part of the estimator's
// outputs (the dB conversions), from the record, after the call's host wait.
#pragma once
#include "modem_device.h"
#include "nr_map.h"

#include <hip/hip_runtime.h>

namespace phyhip {
namespace nr_chest {

// one codeword = one workgroup of the estimator.  Offsets count in entries of the launch's arrays.
struct EstJob {
  uint32_t nof_prb;  // carrier
  uint32_t n_prbs;   // granted PRBs
  uint32_t type;     // 0: type 1 (6 pilots per PRB, every 2nd subcarrier), 1: type 2 (4 pilots, pairs every 6)
  uint32_t n_sym;    // DMRS symbols, 1 .. 4
  uint32_t sym[4];
  uint32_t seed[4];
  float    amplitude; // M_SQRT1_2 (/ beta_dmrs)
  float    subc_hz;   // stride x SRSRAN_SUBC_SPACING_NR(scs): sync_error = sync_err / subc_hz
  uint32_t o_prb;     // Params::prbs: the carrier PRB of every granted one, ascending
  uint32_t o_tab;     // Params::tab: the codeword's table
  uint32_t n_seg;     // 0: measurements only
  uint32_t o_ce;      // Params::ce: the codeword's extracted estimates
  uint32_t nof_re;
  float    filter[5]; // srsran_chest_set_smooth_filter_gauss(., 4, 2)
  float    dist_next[3]; // srsran_symbol_distance_s(sym[i], sym[i + 1], scs)
  float    dist0[14];    // srsran_symbol_distance_s(0, l, scs)
};

// what the estimator leaves per codeword (pinned image: read after the host wait)
struct Record {
  float noise_estimate, rsrp, epre, cfo, sync_error, sync_err;
};

struct EstParams {
  const float2*       grid;   // the slot grid, device-readable: 14 x 12 nof_prb points
  uint32_t            grid_points;
  const EstJob*       jobs;   // device-readable, n_jobs entries
  const uint16_t*     prbs;
  uint32_t            n_prbs_total;
  const nr_map::Seg*  tab;
  uint32_t            n_tab;
  float2*             ce;     // extracted estimates of all codewords
  uint32_t            ce_points;
  Record*             rec;    // n_jobs entries
  float*              noise;  // nullptr, or n_jobs floats of DEVICE memory: the noise estimate for the front end behind (nrchan::FrontParams::noise_dev)
  uint32_t            n_jobs;
  uint32_t            max_seg; // the longest table of the call
  const uint32_t*     x1_bits; // modem::Params: the sequence tables
  const uint32_t*     x2_cols;
};
// A job outside the kernel's bounds writes nothing but a record of NANs (and a noise of 0).
hipError_t launch_est(const EstParams& p, hipStream_t stream);

struct DemapJob {
  uint32_t o_tab, n_seg; // Params::tab
  uint32_t o_out;        // DemapParams::out: the codeword's symbols
  uint32_t nof_re;
};
#define NR_DEMAP_SEGS 16u // table entries per workgroup
struct DemapParams {
  const float2*      grid;
  uint32_t           grid_points;
  const DemapJob*    jobs; // device-readable
  uint32_t           n_jobs;
  uint32_t           max_seg; // the longest table of the call
  const nr_map::Seg* tab;
  uint32_t           n_tab;
  float2*            out;
  uint32_t           out_points;
};
hipError_t launch_demap(const DemapParams& p, hipStream_t stream);

// dmrs_sch.c:848-854 from the record
inline void finish(const Record& r, uint32_t nof_re, srsran_hip_nr_chest_res_t* o)
{
  o->rsrp               = r.rsrp;
  o->rsrp_dbm           = 10.0f * log10f(o->rsrp);
  o->noise_estimate     = r.noise_estimate;
  o->noise_estimate_dbm = 10.0f * log10f(o->noise_estimate);
  o->snr_db             = o->rsrp_dbm - o->noise_estimate_dbm;
  o->cfo                = r.cfo;
  o->sync_error         = r.sync_error;
  o->nof_re             = nof_re;
}

// the job of a grid description that has passed nr_map::invalid(); prbs receives nr_map::granted_prbs(g) entries
inline void fill_job(const srsran_hip_nr_grid_t& g, EstJob* j, uint16_t* prbs)
{
  *j         = EstJob{};
  j->nof_prb = g.nof_prb;
  j->type    = g.dmrs_type;
  j->n_sym   = (uint32_t)nr_map::dmrs_symbols(g, j->sym);
  for (uint32_t i = 0; i < j->n_sym; i++) {
    j->seed[i] = nr_map::dmrs_seed(g, j->sym[i]);
  }
  for (uint32_t i = 0; i + 1 < j->n_sym; i++) {
    j->dist_next[i] = nr_map::symbol_distance_s(j->sym[i], j->sym[i + 1], g.scs);
  }
  for (uint32_t l = 0; l < nr_map::NSYMB; l++) {
    j->dist0[l] = nr_map::symbol_distance_s(0, l, g.scs);
  }
  float amplitude = (float)M_SQRT1_2; // dmrs_sch.c:690-693
  if (std::isnormal(g.beta_dmrs)) {
    amplitude /= g.beta_dmrs;
  }
  j->amplitude = amplitude;
  j->subc_hz   = (float)nr_map::dmrs_stride(g) * (float)(15000u << g.scs);
  nr_map::smooth_filter(j->filter);
  uint32_t n = 0;
  for (uint32_t rb = 0; rb < g.nof_prb; rb++) {
    if (g.prb_idx[rb]) {
      prbs[n++] = (uint16_t)rb;
    }
  }
  j->n_prbs = n;
}

} // namespace nr_chest
} // namespace phyhip
