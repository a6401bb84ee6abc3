// chest_dl_host.cpp -- the downlink channel estimator's entry points (include/srsran_amd/phy_chan_abi.h: srsran_hip_chest_dl_estimate): the received grids,
// the caller's pilot rows and PSS into the calling thread's pinned image, ONE launch of chest_dl_kernel (one workgroup per (rx antenna, port) pair), one host
// wait, the ce grids copied to the caller's and the per-call values finished from the pairs' records (chest_dl.h).
#include "chan_internal.h"
#include "chest_dl_device.h"

using namespace phyhip;
using namespace phyhip::chan;

bool phyhip::chan::est_valid(const char* who, EstMap* est, const srsran_hip_pdsch_sf_t* sf, uint32_t nof_rx)
{
  if (est && est->out) {
    *est->out = {};
  }
  const char* why = (!est || !est->cfg || !est->state || !est->out || !sf) ? "NULL estimator description, state, est_out or sf" : chest_dl::invalid(est->cfg, est->state);
  if (!why) {
    const srsran_hip_chest_dl_t& c = *est->cfg;
    if (c.nof_prb != sf->cell_nof_prb || c.nof_ports != sf->cell_nof_ports || c.id != sf->cell_id || c.cp_nsymb != sf->cp_nsymb || c.sf_idx != sf->sf_idx) {
      why = "the estimator's cell or subframe is not sf's";
    } else if (c.nof_rx != nof_rx) {
      why = "the estimator's nof_rx is not the grant's";
    } else if (sf->nof_symb_slot[0] != c.cp_nsymb || sf->nof_symb_slot[1] != c.cp_nsymb) {
      why = "the estimator needs the grids of both whole slots (nof_symb_slot == cp_nsymb)";
    } else if (c.decoder_zf > 1) {
      why = "decoder_zf is not 0 or 1";
    }
  }
  if (why) {
    refuse("%s: channel estimator: %s", who, why);
    return false;
  }
  return true;
}

extern "C" int srsran_hip_chest_dl_estimate(const srsran_hip_chest_dl_t* cfg, const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                            cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_hip_chest_dl_res_t* res)
{
  static const char* who = "srsran_hip_chest_dl_estimate";
  if (res) {
    *res = {};
  }
  if (!cfg || !state_in || !sf_symbols || !res) {
    return refuse("%s: NULL argument", who);
  }
  if (const char* why = chest_dl::invalid(cfg, state_in)) {
    return refuse("%s: %s", who, why);
  }
  for (uint32_t a = 0; a < cfg->nof_rx; a++) {
    if (!sf_symbols[a]) {
      return refuse("%s: NULL grid of antenna %u", who, a);
    }
  }
  const srsran_hip_chest_dl_t& c = *cfg;
  const chest_dl::Layout       l = chest_dl::layout_of(c);
  const uint32_t               n = c.nof_rx * c.nof_ports;
  uint32_t                     n_out = 0;
  for (uint32_t p = 0; ce && p < c.nof_ports; p++) {
    for (uint32_t a = 0; a < c.nof_rx; a++) {
      n_out += ce[p][a] != nullptr;
    }
  }
  ChanStage*  s  = stage_for(who);
  hipStream_t st = s ? sch::stage_stream() : nullptr;
  // pinned: the input, the ce grids that were asked for, the jobs, the records
  const size_t o_out = al256((size_t)l.in_points * sizeof(cf_t)), o_jobs = al256(o_out + (size_t)n_out * l.grid_points * sizeof(cf_t));
  const size_t o_rec = al256(o_jobs + n * sizeof(chest_dl::Job)), need = o_rec + n * sizeof(chest_dl::Record);
  if (!st || !s->grow(need, 0)) {
    return SRSRAN_ERROR;
  }
  chest_dl::stage_input(reinterpret_cast<cf_t*>(s->pin.get()), c, l, sf_symbols);
  auto* jobs = reinterpret_cast<chest_dl::Job*>(s->pin + o_jobs);
  chest_dl::make_jobs(jobs, c, *state_in, l);
  uint32_t at = 0;
  for (uint32_t a = 0; ce && a < c.nof_rx; a++) {
    for (uint32_t p = 0; p < c.nof_ports; p++) {
      if (ce[p][a]) {
        jobs[a * c.nof_ports + p].o_ce = at;
        at += l.grid_points;
      }
    }
  }
  const auto*            rec = reinterpret_cast<const chest_dl::Record*>(s->pin + o_rec);
  const chest_dl::Params cp  = {reinterpret_cast<const float2*>(s->pin.get()), reinterpret_cast<float2*>(s->pin + o_out), jobs,
                                reinterpret_cast<chest_dl::Record*>(s->pin + o_rec), nullptr, n, l.in_points, n_out * l.grid_points};
  if (call::settle(chest_dl::launch(cp, st), st) != hipSuccess) {
    set_error("%s: channel estimator launch failed", who);
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < n; i++) {
    if (jobs[i].o_ce != CHEST_DL_NONE) {
      memcpy(ce[i % c.nof_ports][i / c.nof_ports], s->pin + o_out + (size_t)jobs[i].o_ce * sizeof(cf_t), (size_t)l.grid_points * sizeof(cf_t));
    }
  }
  chest_dl::finish(c, *state_in, rec, srsran_symbol_sz(c.nof_prb), res);
  return SRSRAN_SUCCESS;
}
