// nr_chest_host.cpp -- the two stages in front of an NR codeword by themselves (include/srsran_amd/phy_nr_chan_abi.h): srsran_hip_nr_sch_get
// (srsran_pdsch_nr_get / srsran_pusch_nr_get) and srsran_hip_dmrs_sch_estimate (srsran_dmrs_sch_estimate), and the RE count of a grant.  The grid calls
// that run both in front of the codeword's front end are in nr_chan_host.cpp; the rules are in nr_map.h, the kernels in nr_chest_kernels.hip.
// The staging context is the transport-block one (sch_nr_internal.h).  One layout serves the pinned image and the device buffer:
//   [grid | table | granted PRBs | estimator job | de-mapper job | record | output]
// the regions in front of the record go up in the one copy of a round trip (call_frame.h) that brings nothing down: the record and the output are written to
// the pinned image by the kernels themselves.
#include "call_frame.h"
#include "hip_common.h"
#include "nr_chest_device.h"
#include "sch_nr_internal.h"
#include "srsran_amd/phy_nr_chan_abi.h"

using namespace phyhip;
using namespace phyhip::nrtb;

namespace {

// what = 0: de-mapping into out; 1: estimation, out may be nullptr
int nr_grid_stage(const char* who, int what, const srsran_hip_nr_grid_t* grid, const cf_t* sf_symbols, cf_t* out, srsran_hip_nr_chest_res_t* res)
{
  if (res) {
    memset(res, 0, sizeof(*res));
  }
  if (!grid || !sf_symbols || (what == 0 && !out) || (what == 1 && !res)) {
    return call::refused(who, "NULL argument");
  }
  if (const char* why = nr_map::invalid(*grid)) {
    return call::refused(who, why);
  }
  const uint32_t nof_re = nr_map::nof_re(*grid), n_seg = nr_map::nof_seg(*grid), n_prbs = nr_map::granted_prbs(*grid);
  const uint32_t grid_points = nr_map::NSYMB * 12 * grid->nof_prb;
  NrTbStage&     s           = tb_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  const size_t o_grid = 0, o_tab = al256((size_t)grid_points * sizeof(cf_t)), o_prbs = al256(o_tab + (size_t)n_seg * sizeof(nr_map::Seg));
  const size_t o_ej = al256(o_prbs + (size_t)n_prbs * sizeof(uint16_t)), o_dj = al256(o_ej + sizeof(nr_chest::EstJob));
  const size_t o_rec = al256(o_dj + sizeof(nr_chest::DemapJob)), o_out = al256(o_rec + sizeof(nr_chest::Record));
  const size_t end = al256(o_out + (size_t)nof_re * sizeof(cf_t));
  modem::Params mp;
  if (!s.grow(end) || !modem::params_for(mp, modem::LLR_I8)) {
    return call::failed(who, get_error());
  }
  memcpy(s.pin + o_grid, sf_symbols, (size_t)grid_points * sizeof(cf_t));
  nr_map::Seg*        tab  = reinterpret_cast<nr_map::Seg*>(s.pin + o_tab);
  uint16_t*           prbs = reinterpret_cast<uint16_t*>(s.pin + o_prbs);
  nr_chest::EstJob*   ej   = reinterpret_cast<nr_chest::EstJob*>(s.pin + o_ej);
  nr_chest::DemapJob* dj   = reinterpret_cast<nr_chest::DemapJob*>(s.pin + o_dj);
  nr_chest::Record*   rec  = reinterpret_cast<nr_chest::Record*>(s.pin + o_rec);
  float2*             dout = reinterpret_cast<float2*>(s.pin + o_out);
  const float2*       dgrid = reinterpret_cast<const float2*>(s.dev + o_grid);
  nr_map::fill_table(*grid, tab);
  const nr_map::Seg* d_tab = reinterpret_cast<const nr_map::Seg*>(s.dev + o_tab);
  if (what == 0) {
    *dj = nr_chest::DemapJob{0, n_seg, 0, nof_re};
  } else {
    nr_chest::fill_job(*grid, ej, prbs);
    ej->o_prb = 0, ej->o_tab = 0, ej->n_seg = out ? n_seg : 0, ej->o_ce = 0, ej->nof_re = out ? nof_re : 0;
  }
  const auto enqueue = [&](hipStream_t st) {
    if (what == 0) {
      nr_chest::DemapParams dp{dgrid, grid_points, reinterpret_cast<const nr_chest::DemapJob*>(s.dev + o_dj), 1, n_seg, d_tab, n_seg, dout, nof_re};
      return nr_chest::launch_demap(dp, st);
    }
    const nr_chest::EstJob* d_ej   = reinterpret_cast<const nr_chest::EstJob*>(s.dev + o_ej);
    const uint16_t*         d_prbs = reinterpret_cast<const uint16_t*>(s.dev + o_prbs);
    nr_chest::EstParams ep{dgrid, grid_points, d_ej, d_prbs, n_prbs, d_tab, n_seg, out ? dout : nullptr, out ? nof_re : 0, rec, nullptr, 1, out ? n_seg : 0, mp.x1_bits,
                           mp.x2_cols};
    return nr_chest::launch_est(ep, st);
  };
  // the grid, the table and the jobs go up; nothing comes down: the output and the record are written to the pinned image
  if (!call::round_trip(who, s.st, s.pin, s.dev, o_rec, o_rec, 0, enqueue)) {
    return SRSRAN_ERROR;
  }
  if (out) {
    memcpy(out, s.pin + o_out, (size_t)nof_re * sizeof(cf_t));
  }
  if (what == 1) {
    nr_chest::finish(*rec, nof_re, res);
  }
  return what == 0 ? (int)nof_re : SRSRAN_SUCCESS;
}

} // namespace

extern "C" uint32_t srsran_hip_nr_sch_nof_re(const srsran_hip_nr_grid_t* grid)
{
  return (grid && !nr_map::invalid(*grid)) ? nr_map::nof_re(*grid) : 0u;
}

extern "C" int srsran_hip_nr_sch_get(const srsran_hip_nr_grid_t* grid, const cf_t* sf_symbols, cf_t* symbols)
{
  TraceRange trace_("srsran_hip_nr_sch_get");
  return nr_grid_stage("nr_sch_get", 0, grid, sf_symbols, symbols, nullptr);
}

extern "C" int srsran_hip_dmrs_sch_estimate(const srsran_hip_nr_grid_t* grid, const cf_t* sf_symbols, cf_t* ce, srsran_hip_nr_chest_res_t* res)
{
  TraceRange trace_("srsran_hip_dmrs_sch_estimate");
  return nr_grid_stage("dmrs_sch_estimate", 1, grid, sf_symbols, ce, res);
}
