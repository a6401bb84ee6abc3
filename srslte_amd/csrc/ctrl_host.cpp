// ctrl_host.cpp -- the PCFICH and the PHICH of a subframe (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pcfich_table / _phich_ngroups / _phich_table,
// srsran_hip_pcfich_decode{,_dbg}, srsran_hip_phich_decode_multi).  The REs are pdcch_map.h's; the receivers are ctrl_kernels.hip's one kernel.  A call is one
// round trip (call_frame.h) with one launch on the calling thread's staging context.  One layout serves the pinned image and the device
// buffer:
//   [the PHICH jobs | the rows of every plane the channel reaches || the PCFICH's row | the PHICH rows]
// what is in front of || goes up, what is behind comes down.  The PCFICH stages row 0 alone, the PHICH the rows its mapping units reach (at most 3).
#include "call_frame.h"
#include "ctrl_device.h"
#include "srsran_amd/phy_conv_abi.h"

using namespace phyhip;

static_assert(sizeof(srsran_hip_phich_res_t) == sizeof(ctrl::PhichRow) && sizeof(srsran_hip_phich_res_t) == 44 &&
                  offsetof(srsran_hip_phich_res_t, bits) == offsetof(ctrl::PhichRow, bits) && offsetof(srsran_hip_phich_res_t, z) == offsetof(ctrl::PhichRow, z),
              "ctrl_kernel writes its PHICH rows in this layout");
static_assert(sizeof(srsran_hip_phich_resource_t) == 8, "phy_conv_abi.h layout");

namespace {

struct CtrlStage : call::Stage {};

CtrlStage& ctrl_stage() // of the calling thread, on the device it is bound to
{
  static thread_local StageRef<CtrlStage> r;
  return r.get();
}

// one call: the PCFICH (row != nullptr), or n PHICH resources
int run(const char* who, const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
        ctrl::PcfichRow* row, uint32_t n, const srsran_hip_phich_resource_t* r, srsran_hip_phich_res_t* res)
{
  TraceRange              trace_(who);
  const char*             why = nullptr;
  const pdcch_map::Table* t   = pdcch_map::table_of(sf, &why);
  if (!why && (!sf_symbols || !ce || (!row && (!r || !res)))) {
    why = "NULL argument";
  }
  if (!why) {
    why = pdcch_map::planes_invalid(*sf, sf_symbols, ce);
  }
  if (!why) {
    why = ctrl::phich_invalid(*t, *sf, n, r);
  }
  if (why) {
    return call::refused(who, why);
  }
  CtrlStage&    s = ctrl_stage();
  modem::Params mp;
  if (!s.ready()) {
    return call::no_device(who);
  }
  if (!modem::params_for(mp, modem::LLR_F32)) {
    return call::failed(who, "the sequence tables could not be placed on the device");
  }
  const uint32_t rows = row ? 1u : t->phich_rows, n_planes = sf->nof_rx * (1 + sf->cell_nof_ports);
  const size_t   pb = (size_t)rows * 12 * sf->cell_nof_prb * sizeof(cf_t), pstride = al256(pb);
  const size_t   o_planes = al256((size_t)n * sizeof(ctrl::PhichJob)), up = o_planes + n_planes * pstride;
  const size_t   o_phich = al256(up + (row ? sizeof(ctrl::PcfichRow) : 0)), end = o_phich + (size_t)n * sizeof(ctrl::PhichRow);
  if (!s.grow(end)) {
    return call::failed(who, "the staging allocation failed");
  }
  ctrl::phich_jobs(reinterpret_cast<ctrl::PhichJob*>(s.pin.get()), *t, *sf, n, r);
  pdcch_map::stage_planes(s.pin + o_planes, *sf, sf_symbols, ce, pb, pstride);
  ctrl::Params cp = {};
  cp.rx           = reinterpret_cast<const float2*>(s.dev + o_planes);
  cp.stride       = (uint32_t)(pstride / sizeof(cf_t));
  cp.ce           = cp.rx + (size_t)sf->nof_rx * cp.stride;
  cp.ports        = sf->cell_nof_ports;
  cp.nof_rx       = sf->nof_rx;
  cp.ext          = sf->cp_nsymb == 6;
  cp.noise        = noise_estimate; // pcfich.c:200, phich.c:251: not halved
  cp.seed         = ctrl::c_init(*sf);
  cp.qpsk_f       = mp.k.qpsk_f;
  cp.x1_bits      = mp.x1_bits;
  cp.x2_cols      = mp.x2_cols;
  cp.pcfich       = row ? 1 : 0;
  memcpy(cp.pcfich_idx, t->pcfich, sizeof(cp.pcfich_idx));
  cp.pcfich_out = reinterpret_cast<ctrl::PcfichRow*>(s.dev + up);
  cp.jobs       = reinterpret_cast<const ctrl::PhichJob*>(s.dev.get());
  cp.n_phich    = n;
  cp.phich_out  = reinterpret_cast<ctrl::PhichRow*>(s.dev + o_phich);
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, end - up, [&](hipStream_t st) { return ctrl::launch(cp, st); })) {
    return SRSRAN_ERROR;
  }
  if (row) {
    memcpy(row, s.pin + up, sizeof(*row));
  }
  if (n) {
    memcpy(res, s.pin + o_phich, (size_t)n * sizeof(*res));
  }
  return SRSRAN_SUCCESS;
}

int pcfich(const char* who, const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate, uint32_t* cfi,
           float* corr, float* data_f, cf_t* d, float* corr3)
{
  if (cfi) {
    *cfi = 0;
  }
  if (corr) {
    *corr = 0.f;
  }
  if (!cfi) {
    return call::refused(who, "NULL argument");
  }
  ctrl::PcfichRow row;
  const int       rc = run(who, sf, sf_symbols, ce, noise_estimate, &row, 0, nullptr, nullptr);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  *cfi = row.cfi;
  if (corr) {
    *corr = row.corr;
  }
  if (data_f) {
    memcpy(data_f, row.data_f, sizeof(row.data_f));
  }
  if (d) {
    memcpy(d, row.d, sizeof(row.d));
  }
  if (corr3) {
    memcpy(corr3, row.corr3, sizeof(row.corr3));
  }
  return 1; // as srsran_pcfich_decode
}

} // namespace

extern "C" int srsran_hip_regs_pcfich_table(const srsran_hip_pdcch_sf_t* sf, uint32_t re_idx[16])
{
  const char*             why;
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  if (!t || !re_idx) {
    return -1;
  }
  memcpy(re_idx, t->pcfich, sizeof(t->pcfich));
  return (int)ctrl::kPcfichRe;
}

extern "C" int srsran_hip_regs_phich_ngroups(const srsran_hip_pdcch_sf_t* sf)
{
  const char*             why;
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  return t ? (int)t->phich_groups : -1;
}

extern "C" int srsran_hip_regs_phich_table(const srsran_hip_pdcch_sf_t* sf, uint32_t ngroup, uint32_t re_idx[12])
{
  const char*             why;
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  if (!t || !re_idx || ngroup >= t->phich_groups) {
    return -1;
  }
  const uint32_t unit = sf->cp_nsymb == 6 ? ngroup / 2 : ngroup;
  memcpy(re_idx, &t->phich[(size_t)ctrl::kPhichRe * unit], ctrl::kPhichRe * sizeof(uint32_t));
  return (int)ctrl::kPhichRe;
}

extern "C" int srsran_hip_pcfich_decode(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                        uint32_t* cfi, float* corr)
{
  return pcfich("srsran_hip_pcfich_decode", sf, sf_symbols, ce, noise_estimate, cfi, corr, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pcfich_decode_dbg(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                            uint32_t* cfi, float* corr, float data_f[32], cf_t d[16], float corr3[3])
{
  return pcfich("srsran_hip_pcfich_decode_dbg", sf, sf_symbols, ce, noise_estimate, cfi, corr, data_f, d, corr3);
}

extern "C" int srsran_hip_phich_decode_multi(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                             uint32_t n, const srsran_hip_phich_resource_t* r, srsran_hip_phich_res_t* res)
{
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (res && n <= SRSRAN_HIP_PHICH_MAX_RESOURCES) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  return run("srsran_hip_phich_decode_multi", sf, sf_symbols, ce, noise_estimate, nullptr, n, r, res);
}
