// pucch_host.cpp -- PUCCH receive in one device call (include/srsran_amd/phy_pucch_abi.h): the caller's tables, the plan (pucch_map.h), and the calls.  A call
// is one round trip (call_frame.h) with the launch of pucch_kernels.hip on the calling thread's grant staging context (chan_internal.h); what the
// reference decides in float on the host (the measurements' dB and rounding rules, the thresholds) is taken from the records that came down
// (pucch_map.h finish).  One layout serves the pinned image and the device buffer:
//   [the jobs | the column blocks || the records | the intermediates]
// what is in front of || goes up, what is behind comes down (the last only for the _dbg and the estimator call).  A column block is the nsymb x 12 points
// of one slot at one PRB; jobs that share a PRB share its block.
#include "chan_internal.h"
#include "pucch_device.h"
#include "pucch_map.h"
#include "srsran_amd/phy_pucch_abi.h"

#include <complex>
#include <string>

using namespace phyhip;

static_assert(sizeof(srsran_hip_pucch_cell_t) == 12 && sizeof(srsran_hip_pucch_sf_t) == 8 && sizeof(srsran_hip_pucch_job_t) == 68 &&
                  sizeof(srsran_hip_pucch_plan_t) == 260 && sizeof(srsran_hip_pucch_res_t) == 64 && sizeof(srsran_hip_pucch_dbg_t) == 32,
              "phy_pucch_abi.h layout");
static_assert(pucch::kMaxZ == SRSRAN_HIP_PUCCH_MAX_SYMBOLS && pucch::kWordBits == SRSRAN_HIP_PUCCH_MAX_BITS && pucch::kBits2 == SRSRAN_HIP_PUCCH2_NOF_BITS,
              "phy_pucch_abi.h constants");
static_assert(sizeof(pucch::Job) == 352 && sizeof(pucch::Record) == 96 && sizeof(pucch::Dbg) == 1768, "pucch_device.h layout: the staging offsets count on it");

namespace {

// the caller's tables (srsran_hip_pucch_set_tables): process-wide, copied under the lock
std::mutex g_tab_mu;
int8_t     g_phi[30][12];
uint32_t   g_basis[pucch::kWordBits];
bool       g_have_tables = false;

bool tables(int8_t phi[30][12], uint32_t* basis)
{
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (g_have_tables) {
    memcpy(phi, g_phi, sizeof(g_phi));
    memcpy(basis, g_basis, sizeof(g_basis));
  }
  return g_have_tables;
}

// n jobs on one grid.  ce_grid: the estimator stage alone
int run(const char* who, const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, uint32_t n, const srsran_hip_pucch_job_t* jobs, const cf_t* sf_symbols,
        srsran_hip_pucch_res_t* res, const srsran_hip_pucch_dbg_t* dbg, cf_t* ce_grid)
{
  TraceRange trace_(who);
  int8_t     phi[30][12];
  pucch::Params k = {};
  if (!tables(phi, k.basis)) {
    return call::refused(who, "the tables have not been set (srsran_hip_pucch_set_tables)");
  }
  std::vector<srsran_hip_pucch_plan_t> plans(n);
  pucch::CellSeq                       seq;
  pucch::cell_seq(*cell, seq);
  for (uint32_t i = 0; i < n; i++) {
    const char* why = pucch::plan(*cell, seq, *sf, jobs[i], plans[i]);
    if (!why) {
      why = pucch::invalid_settings(jobs[i]);
    }
    if (why) {
      const std::string text = "job " + std::to_string(i) + ": " + why;
      return call::refused(who, text.c_str());
    }
  }
  chan::ChanStage* s  = chan::stage_for(who);
  hipStream_t      st = s ? sch::stage_stream() : nullptr;
  if (!st) {
    return s ? call::failed(who, "no stream on the calling thread's staging context") : SRSRAN_ERROR;
  }
  // the column blocks the jobs touch: (slot, PRB) -> block
  const uint32_t        nsymb = cell->cp ? 6 : 7, block_pts = nsymb * pucch::kNre;
  std::vector<int32_t>  block_of(2 * 110, -1);
  std::vector<uint32_t> blocks;
  for (uint32_t i = 0; i < n; i++) {
    for (uint32_t ns = 0; ns < 2; ns++) {
      int32_t& b = block_of[ns * 110 + plans[i].n_prb[ns]];
      if (b < 0) {
        b = (int32_t)blocks.size();
        blocks.push_back(ns * 110 + plans[i].n_prb[ns]);
      }
    }
  }
  const bool   want_dbg = dbg || ce_grid;
  const size_t o_cols = al256((size_t)n * sizeof(pucch::Job)), o_rec = al256(o_cols + blocks.size() * block_pts * sizeof(cf_t));
  const size_t o_dbg = al256(o_rec + (size_t)n * sizeof(pucch::Record)), end = o_dbg + (want_dbg ? (size_t)n * sizeof(pucch::Dbg) : 0);
  if (!s->grow(end, end)) {
    return call::failed(who, "the staging allocation failed");
  }
  auto* dj = reinterpret_cast<pucch::Job*>(s->pin.get());
  for (uint32_t i = 0; i < n; i++) {
    pucch::device_job(*cell, *sf, jobs[i], plans[i], phi, ce_grid == nullptr, dj[i]);
    for (uint32_t ns = 0; ns < 2; ns++) {
      dj[i].col[ns] = (uint32_t)block_of[ns * 110 + plans[i].n_prb[ns]];
    }
  }
  for (size_t b = 0; b < blocks.size(); b++) {
    const uint32_t ns = blocks[b] / 110, prb = blocks[b] % 110;
    for (uint32_t l = 0; l < nsymb; l++) {
      memcpy(s->pin + o_cols + (b * block_pts + l * pucch::kNre) * sizeof(cf_t), sf_symbols + ((size_t)(ns * nsymb + l) * cell->nof_prb + prb) * pucch::kNre,
             pucch::kNre * sizeof(cf_t));
    }
  }
  k.jobs   = reinterpret_cast<const pucch::Job*>(s->dev.get());
  k.cols   = reinterpret_cast<const float2*>(s->dev + o_cols);
  k.rec    = reinterpret_cast<pucch::Record*>(s->dev + o_rec);
  k.dbg    = want_dbg ? reinterpret_cast<pucch::Dbg*>(s->dev + o_dbg) : nullptr;
  k.n_jobs = n;
  k.n_cols = (uint32_t)blocks.size();
  k.qpsk_s = (float)(-100 * M_SQRT2);
  if (!call::round_trip(who, st, s->pin, s->dev, o_rec, o_rec, end - o_rec, [&](hipStream_t q) { return pucch::launch(k, q); })) {
    return SRSRAN_ERROR;
  }
  const auto* rec = reinterpret_cast<const pucch::Record*>(s->pin + o_rec);
  const auto* d   = reinterpret_cast<const pucch::Dbg*>(s->pin + o_dbg);
  for (uint32_t i = 0; i < n; i++) {
    if (rec[i].bad) {
      return call::failed(who, "the kernel refused a job record");
    }
    pucch::finish(jobs[i], plans[i].n_rs, rec[i], ce_grid == nullptr, res[i]);
  }
  if (ce_grid) { // one job: the slot's row on every symbol of the slot, in the 12 columns of that slot's PRB
    for (uint32_t l = 0; l < 2 * nsymb; l++) {
      const uint32_t ns = l / nsymb;
      memcpy(ce_grid + ((size_t)l * cell->nof_prb + plans[0].n_prb[ns]) * pucch::kNre, d[0].ce[ns], pucch::kNre * sizeof(cf_t));
    }
  }
  if (dbg) { // one job
    if (dbg->z) {
      memcpy(dbg->z, d[0].z, sizeof(d[0].z));
    }
    if (dbg->llr) {
      memcpy(dbg->llr, d[0].llr, sizeof(d[0].llr));
    }
    if (dbg->ce) {
      memcpy(dbg->ce, d[0].ce, sizeof(d[0].ce));
    }
    if (dbg->pilot_estimates) {
      memcpy(dbg->pilot_estimates, d[0].pe, (size_t)2 * plans[0].n_rs * pucch::kNre * sizeof(cf_t));
    }
  }
  return SRSRAN_SUCCESS;
}

int one(const char* who, const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* job, const cf_t* sf_symbols,
        srsran_hip_pucch_res_t* res, const srsran_hip_pucch_dbg_t* dbg, cf_t* ce_grid)
{
  if (res) {
    memset(res, 0, sizeof(*res));
  }
  if (!cell || !sf || !job || !sf_symbols || !res) {
    return call::refused(who, "NULL argument");
  }
  return run(who, cell, sf, 1, job, sf_symbols, res, dbg, ce_grid);
}

} // namespace

extern "C" int srsran_hip_pucch_set_tables(const cf_t base[30][12], const uint8_t basis[13][20])
{
  const char*                 who = "srsran_hip_pucch_set_tables";
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (!base || !basis) {
    g_have_tables = false;
    return SRSRAN_SUCCESS;
  }
  int8_t   phi[30][12];
  uint32_t masks[pucch::kWordBits] = {};
  for (int u = 0; u < 30; u++) {
    for (int k = 0; k < 12; k++) {
      // base[u][k] = cexpf(j phi pi / 4): phi = 4 arg / pi must be one of -3, -1, 1, 3, the modulus 1, both to a few float roundings
      const std::complex<float> v(reinterpret_cast<const float*>(&base[u][k])[0], reinterpret_cast<const float*>(&base[u][k])[1]);
      const float               q = std::arg(v) * 4.0f / (float)M_PI;
      const int                 f = (int)lroundf(q);
      if (!(fabsf(std::abs(v) - 1.0f) < 1e-5f) || !(fabsf(q - (float)f) < 1e-4f) || (f != -3 && f != -1 && f != 1 && f != 3)) {
        return call::refused(who, "a base sequence value is not unit-modulus with phi in {-3, -1, 1, 3}");
      }
      phi[u][k] = (int8_t)f;
    }
  }
  for (uint32_t n = 0; n < pucch::kWordBits; n++) {
    for (uint32_t i = 0; i < pucch::kBits2; i++) {
      if (basis[n][i] > 1) {
        return call::refused(who, "a basis entry is neither 0 nor 1");
      }
      masks[n] |= (uint32_t)basis[n][i] << i;
    }
  }
  memcpy(g_phi, phi, sizeof(g_phi));
  memcpy(g_basis, masks, sizeof(g_basis));
  g_have_tables = true;
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_pucch_plan(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* job,
                                     srsran_hip_pucch_plan_t* plan)
{
  const char* who = "srsran_hip_pucch_plan";
  if (plan) {
    memset(plan, 0, sizeof(*plan));
  }
  if (!cell || !sf || !job || !plan) {
    return call::refused(who, "NULL argument");
  }
  int8_t   phi[30][12];
  uint32_t basis[pucch::kWordBits];
  if (!tables(phi, basis)) {
    return call::refused(who, "the tables have not been set (srsran_hip_pucch_set_tables)");
  }
  pucch::CellSeq seq;
  pucch::cell_seq(*cell, seq);
  const char* why = pucch::plan(*cell, seq, *sf, *job, *plan);
  if (why) {
    memset(plan, 0, sizeof(*plan));
    return call::refused(who, why);
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_pucch_decode_multi(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, uint32_t n, const srsran_hip_pucch_job_t* jobs,
                                             const cf_t* sf_symbols, srsran_hip_pucch_res_t* res)
{
  const char* who = "srsran_hip_pucch_decode_multi";
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (n > SRSRAN_HIP_PUCCH_MAX_JOBS) {
    return call::refused(who, "more than 256 jobs");
  }
  if (res) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  if (!cell || !sf || !jobs || !sf_symbols || !res) {
    return call::refused(who, "NULL argument");
  }
  const int rc = run(who, cell, sf, n, jobs, sf_symbols, res, nullptr, nullptr);
  if (rc != SRSRAN_SUCCESS) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  return rc;
}

extern "C" int srsran_hip_pucch_decode(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* job, const cf_t* sf_symbols,
                                       srsran_hip_pucch_res_t* res)
{
  return one("srsran_hip_pucch_decode", cell, sf, job, sf_symbols, res, nullptr, nullptr);
}

extern "C" int srsran_hip_pucch_decode_dbg(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* job,
                                           const cf_t* sf_symbols, srsran_hip_pucch_res_t* res, const srsran_hip_pucch_dbg_t* dbg)
{
  const char* who = "srsran_hip_pucch_decode_dbg";
  if (!dbg) {
    if (res) {
      memset(res, 0, sizeof(*res));
    }
    return call::refused(who, "NULL argument");
  }
  return one(who, cell, sf, job, sf_symbols, res, dbg, nullptr);
}

extern "C" int srsran_hip_chest_ul_estimate_pucch(const srsran_hip_pucch_cell_t* cell, const srsran_hip_pucch_sf_t* sf, const srsran_hip_pucch_job_t* job,
                                                  const cf_t* sf_symbols, cf_t* ce, srsran_hip_pucch_res_t* res)
{
  const char* who = "srsran_hip_chest_ul_estimate_pucch";
  if (!ce) {
    if (res) {
      memset(res, 0, sizeof(*res));
    }
    return call::refused(who, "NULL argument");
  }
  return one(who, cell, sf, job, sf_symbols, res, nullptr, ce);
}
