// pdcch_host.cpp -- the PDCCH search of a subframe from the received grids (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pdcch_*,
// srsran_hip_pdcch_extract_llr, srsran_hip_pdcch_search_sf{,_dbg}).  The REG map is pdcch_map.h's; the front end is pdcch_kernels.hip; the decodes, with the mean
// rule on the device, are conv_kernels.hip's pdcch_dci_sf_kernel.  A search is one round trip (call_frame.h) with two launches on the calling thread's
// staging context.  One layout serves the pinned image and the device buffer:
//   [candidates | the region's rows of every plane || results | soft bits | _dbg: de-matched floats | symbols | equalised symbols | extracted planes]
// what is in front of || goes up; of what is behind, a search brings down the results, srsran_hip_pdcch_extract_llr the soft bits, _dbg everything.
// The search from the received grids alone (srsran_hip_pdcch_search_est{,_dbg}: run_est) puts the estimator and the PCFICH / PHICH kernel in front on the same
// stream: one round trip with four launches; its layout stands at the function.
// A description's table is built once per thread and uploaded once per staging context; both caches are small and start over when they are full.  That is
// safe because nothing of the thread's is in flight between two calls and because a call never holds an entry across an eviction: a call that takes one table
// looks up once, and run_est, which holds the tables of CFI 1, 2 and 3 at once, makes room for all that are missing BEFORE its first lookup (reserve_all_cfi),
// so none of its three lookups can empty the cache under the pointers it already has.
#include "call_frame.h"
#include "chest_dl_device.h"
#include "conv_device.h"
#include "ctrl_device.h"
#include "modem_device.h"
#include "pdcch_device.h"
#include "pdcch_map.h"
#include "srsran_amd/phy_conv_abi.h"

#include <algorithm>
#include <memory>

using namespace phyhip;

static_assert(sizeof(srsran_hip_pdcch_sf_t) == 44, "phy_conv_abi.h layout");
static_assert(sizeof(srsran_hip_pdcch_res_t) == conv::kDciResRow && offsetof(srsran_hip_pdcch_res_t, crc_rem) == conv::kDciBits &&
                  offsetof(srsran_hip_pdcch_res_t, decoded) == conv::kDciBits + 2 && offsetof(srsran_hip_pdcch_res_t, mean) == conv::kDciBits + 4,
              "pdcch_dci_sf_kernel writes its rows in this layout");

namespace {

constexpr size_t kMaxTables = 32;

struct HostTable {
  srsran_hip_pdcch_sf_t sf;
  pdcch_map::Table      t;
  bool                  ok;
};

// how many of the tables of sf with cfi = 1, 2, 3 a cache of entries with an `sf` member lacks; the cache starts over now if it has no room for them
template <class Cache>
void reserve_all_cfi(Cache& cache, const srsran_hip_pdcch_sf_t& sf)
{
  size_t missing = 0;
  for (uint32_t c = 1; c <= 3; c++) {
    srsran_hip_pdcch_sf_t one = sf;
    one.cfi                   = c;
    bool found                = false;
    for (const auto& e : cache) {
      found = found || pdcch_map::same_map(e->sf, one);
    }
    missing += found ? 0 : 1;
  }
  if (cache.size() + missing > kMaxTables) {
    cache.clear();
  }
}

std::vector<std::unique_ptr<HostTable>>& host_cache() // of the calling thread
{
  static thread_local std::vector<std::unique_ptr<HostTable>> cache;
  return cache;
}

// the table of a description that has passed pdcch_map::invalid(), built once per thread; nullptr: the rules are not defined on it
const pdcch_map::Table* host_table(const srsran_hip_pdcch_sf_t& sf)
{
  auto& cache = host_cache();
  for (const auto& e : cache) {
    if (pdcch_map::same_map(e->sf, sf)) {
      return e->ok ? &e->t : nullptr;
    }
  }
  if (cache.size() >= kMaxTables) {
    cache.clear();
  }
  auto e = std::make_unique<HostTable>();
  e->sf  = sf;
  e->ok  = pdcch_map::build(sf, e->t);
  cache.push_back(std::move(e));
  return cache.back()->ok ? &cache.back()->t : nullptr;
}

struct DeviceTable {
  srsran_hip_pdcch_sf_t      sf;
  StageBuf<StageMem::Device> d;
};

struct PdcchStage : call::Stage {
  std::vector<std::unique_ptr<DeviceTable>> tables;
  // the description's table in device memory: uploaded at its first use, resident from then on
  const uint32_t* table(const srsran_hip_pdcch_sf_t& sf, const pdcch_map::Table& t)
  {
    for (const auto& e : tables) {
      if (pdcch_map::same_map(e->sf, sf)) {
        return reinterpret_cast<const uint32_t*>(e->d.get());
      }
    }
    if (tables.size() >= kMaxTables) {
      tables.clear();
    }
    auto e = std::make_unique<DeviceTable>();
    e->sf  = sf;
    if (!e->d.grow(t.re_idx.size() * sizeof(uint32_t)) || upload(e->d.get(), t.re_idx.data(), t.re_idx.size() * sizeof(uint32_t)) != hipSuccess) {
      return nullptr;
    }
    tables.push_back(std::move(e));
    return reinterpret_cast<const uint32_t*>(tables.back()->d.get());
  }
};

PdcchStage& pdcch_stage() // of the calling thread, on the device it is bound to
{
  static thread_local StageRef<PdcchStage> r;
  return r.get();
}

struct Dbg {
  float*       llr_out;
  cf_t*        d_out;
  cf_t* const* sym_out;
  cf_t* const (*ce_out)[SRSRAN_MAX_PORTS];
  float*    rm_f;
  uint16_t* symbols;
};

size_t plane_bytes(const srsran_hip_pdcch_sf_t& sf) // the region's rows of one grid
{
  return (size_t)pdcch_map::nof_ctrl_symbols(sf) * 12 * sf.cell_nof_prb * sizeof(cf_t);
}

// the search, the stage by itself (n == 0, llr != nullptr) and their _dbg form
int run(const char* who, const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate, uint32_t n,
        const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, float* llr, const Dbg* dbg)
{
  TraceRange  trace_(who);
  const bool  search = llr == nullptr;
  const char* why    = nullptr;
  if (search && res && n <= SRSRAN_HIP_PDCCH_MAX_CANDIDATES) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  if (!why && (!sf_symbols || !ce || (search && (!cand || !res)))) {
    why = "NULL argument";
  }
  if (!why && n > SRSRAN_HIP_PDCCH_MAX_CANDIDATES) {
    why = "more than 256 candidates";
  }
  if (!why) {
    why = pdcch_map::planes_invalid(*sf, sf_symbols, ce);
  }
  const uint32_t nsym = t ? 4 * t->nregs : 0, nof_llr = 2 * nsym;
  for (uint32_t i = 0; i < n && !why; i++) {
    why = conv::dci_cand_invalid(cand[i], nof_llr);
  }
  if (why) {
    return call::refused(who, why);
  }
  PdcchStage&   s = pdcch_stage();
  modem::Params mp;
  const auto    zeroed = [&](int rc) { // a failed search leaves no result row behind
    if (search) {
      memset(res, 0, (size_t)n * sizeof(*res));
    }
    return rc;
  };
  if (!s.ready()) {
    return zeroed(call::no_device(who));
  }
  const uint32_t* d_tab = s.table(*sf, *t);
  if (!d_tab || !modem::params_for(mp, modem::LLR_F32)) {
    return zeroed(call::failed(who, "the REG table or the sequence tables could not be placed on the device"));
  }
  const uint32_t n_planes = sf->nof_rx * (1 + sf->cell_nof_ports);
  const size_t   pb = plane_bytes(*sf), pstride = al256(pb), xstride = al256((size_t)nsym * sizeof(cf_t));
  const bool     want_rm = dbg && dbg->rm_f, want_sym = dbg && dbg->symbols, want_d = dbg && dbg->d_out, want_x = dbg && (dbg->sym_out || dbg->ce_out);
  const size_t   o_planes = al256((size_t)n * sizeof(conv::DciJob)), up = o_planes + n_planes * pstride;
  const size_t   o_llr = al256(up + (size_t)n * conv::kDciResRow), o_rm = al256(o_llr + (size_t)nof_llr * sizeof(float));
  const size_t   o_sym = want_rm ? al256(o_rm + (size_t)n * conv::kDciSyms * sizeof(float)) : o_rm;
  const size_t   o_d   = want_sym ? al256(o_sym + (size_t)n * conv::kDciSyms * sizeof(uint16_t)) : o_sym;
  const size_t   o_x   = want_d ? o_d + xstride : o_d;
  const size_t   end   = want_x ? o_x + n_planes * xstride : o_x;
  const size_t   down  = dbg ? end : search ? o_llr : o_rm; // a search brings down the results alone
  if (!s.grow(end)) {
    return zeroed(call::failed(who, "the staging allocation failed"));
  }
  conv::DciJob* jobs = reinterpret_cast<conv::DciJob*>(s.pin.get());
  for (uint32_t i = 0; i < n; i++) {
    jobs[i] = conv::dci_job(cand[i]);
  }
  pdcch_map::stage_planes(s.pin + o_planes, *sf, sf_symbols, ce, pb, pstride);
  pdcch::FrontParams fp = {}; // (what only the search from the received grids alone sets stays null)
  fp.planes       = reinterpret_cast<const float2*>(s.dev + o_planes);
  fp.plane_stride = (uint32_t)(pstride / sizeof(cf_t));
  fp.tab          = d_tab;
  fp.nsym         = nsym;
  fp.ports        = sf->cell_nof_ports;
  fp.nof_rx       = sf->nof_rx;
  fp.noise        = noise_estimate / 2; // pdcch.c:471
  fp.seed         = sf->sf_idx * 512 + sf->cell_id;
  fp.qpsk_f       = mp.k.qpsk_f;
  fp.x1_bits      = mp.x1_bits;
  fp.x2_cols      = mp.x2_cols;
  fp.llr          = reinterpret_cast<float*>(s.dev + o_llr);
  fp.dbg_d        = want_d ? reinterpret_cast<float2*>(s.dev + o_d) : nullptr;
  fp.dbg_planes   = want_x ? reinterpret_cast<float2*>(s.dev + o_x) : nullptr;
  fp.dbg_stride   = (uint32_t)(xstride / sizeof(cf_t));
  const auto enqueue = [&](hipStream_t st) {
    hipError_t e = pdcch::launch_front(fp, st);
    if (e == hipSuccess) {
      e = conv::launch_pdcch_dci_sf(fp.llr, reinterpret_cast<const conv::DciJob*>(s.dev.get()), s.dev + up, want_rm ? reinterpret_cast<float*>(s.dev + o_rm) : nullptr,
                                    want_sym ? reinterpret_cast<uint16_t*>(s.dev + o_sym) : nullptr, n, st);
    }
    return e;
  };
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, down - up, enqueue)) {
    return zeroed(SRSRAN_ERROR);
  }
  if (search) {
    memcpy(res, s.pin + up, (size_t)n * sizeof(*res));
  } else {
    memcpy(llr, s.pin + o_llr, (size_t)nof_llr * sizeof(float));
  }
  if (dbg) {
    if (dbg->llr_out) {
      memcpy(dbg->llr_out, s.pin + o_llr, (size_t)nof_llr * sizeof(float));
    }
    if (want_rm) {
      memcpy(dbg->rm_f, s.pin + o_rm, (size_t)n * conv::kDciSyms * sizeof(float));
    }
    if (want_sym) {
      memcpy(dbg->symbols, s.pin + o_sym, (size_t)n * conv::kDciSyms * sizeof(uint16_t));
    }
    if (want_d) {
      memcpy(dbg->d_out, s.pin + o_d, (size_t)nsym * sizeof(cf_t));
    }
    for (uint32_t a = 0; want_x && a < sf->nof_rx; a++) {
      if (dbg->sym_out && dbg->sym_out[a]) {
        memcpy(dbg->sym_out[a], s.pin + o_x + a * xstride, (size_t)nsym * sizeof(cf_t));
      }
      for (uint32_t p = 0; dbg->ce_out && p < sf->cell_nof_ports; p++) {
        if (dbg->ce_out[p][a]) {
          memcpy(dbg->ce_out[p][a], s.pin + o_x + (sf->nof_rx + p * sf->nof_rx + a) * xstride, (size_t)nsym * sizeof(cf_t));
        }
      }
    }
  }
  return search ? SRSRAN_SUCCESS : (int)nof_llr;
}

struct EstDbg {
  float* llr_out;
  float* pcfich_data_f;
  cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS];
  float*    rm_f;
  uint16_t* symbols;
};

// The control side of a subframe from the received grids alone.  One layout serves the pinned image and the device buffer:
//   [the estimator's input: grids, pilot rows, PSS | its jobs | the three candidate lists | the PHICH jobs ||
//    the estimator's records | the PCFICH's row | the CFI word | the PHICH rows | max(n_cand) result rows |
//    _dbg: soft bits (CFI 3's size) | de-matched floats | symbols ||| device only: the pairs' noise estimates | the ce grids [port][rx] (_dbg: brought down too)]
// what is in front of || goes up in one copy; what lies between || and ||| comes down in one copy, as far as the call needs it.
int run_est(const char* who, const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
            const srsran_hip_pdcch_est_t* opt, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* phich,
            srsran_hip_phich_res_t* phich_res, uint32_t* cfi, float* cfi_corr, srsran_hip_chest_dl_res_t* est_out, const EstDbg* dbg)
{
  TraceRange     trace_(who);
  const uint32_t kMax = SRSRAN_HIP_PDCCH_MAX_CANDIDATES;
  const bool     counts = opt && opt->n_cand[0] <= kMax && opt->n_cand[1] <= kMax && opt->n_cand[2] <= kMax && opt->n_phich <= SRSRAN_HIP_PHICH_MAX_RESOURCES;
  const uint32_t max_n  = counts ? std::max(opt->n_cand[0], std::max(opt->n_cand[1], opt->n_cand[2])) : 0, n_ph = counts ? opt->n_phich : 0;
  const auto     zero   = [&]() {
    if (res && max_n) {
      memset(res, 0, (size_t)max_n * sizeof(*res));
    }
    if (phich_res && n_ph) {
      memset(phich_res, 0, (size_t)n_ph * sizeof(*phich_res));
    }
    if (cfi) {
      *cfi = 0;
    }
    if (cfi_corr) {
      *cfi_corr = 0.f;
    }
    if (est_out) {
      *est_out = {};
    }
  };
  zero();
  const char*             why = nullptr;
  const pdcch_map::Table* t[3] = {nullptr, nullptr, nullptr};
  if (!sf || !est || !state_in || !sf_symbols || !opt || !res || !cfi || !est_out || (opt->n_phich && (!phich || !phich_res)) ||
      ((opt->n_cand[0] || opt->n_cand[1] || opt->n_cand[2]) && !cand)) {
    why = "NULL argument";
  } else if (!counts) {
    why = "more than 256 candidates in a list or more than 16 PHICH resources";
  } else if (opt->cfi3_to_2 > 1) {
    why = "cfi3_to_2 is not 0 or 1";
  } else if (!(why = pdcch_map::invalid(*sf)) && !(why = chest_dl::invalid(est, state_in))) {
    if (est->nof_prb != sf->cell_nof_prb || est->nof_ports != sf->cell_nof_ports || est->id != sf->cell_id || est->cp_nsymb != sf->cp_nsymb || est->sf_idx != sf->sf_idx) {
      why = "the estimator's cell or subframe is not sf's";
    } else if (est->nof_rx != sf->nof_rx) {
      why = "the estimator's nof_rx is not sf's";
    }
  }
  for (uint32_t a = 0; !why && a < sf->nof_rx; a++) {
    why = !sf_symbols[a] ? "a received grid is NULL" : nullptr;
  }
  if (!why) {
    reserve_all_cfi(host_cache(), *sf); // the three pointers below stay good: none of the lookups evicts
  }
  for (uint32_t c = 0; !why && c < 3; c++) { // all three regions: the CFI is not known yet
    srsran_hip_pdcch_sf_t one = *sf;
    one.cfi                   = c + 1;
    t[c]                      = pdcch_map::table_of(&one, &why);
  }
  if (!why) {
    why = ctrl::phich_invalid(*t[0], *sf, n_ph, phich);
  }
  uint32_t first[3] = {0, 0, 0}, n_jobs = 0;
  for (uint32_t c = 0; !why && c < 3; c++) {
    first[c] = n_jobs;
    for (uint32_t i = 0; i < opt->n_cand[c] && !why; i++) {
      why = conv::dci_cand_invalid(cand[n_jobs + i], 8ull * t[c]->nregs, "a location past the end of the control region of its list's CFI");
    }
    n_jobs += opt->n_cand[c];
  }
  if (why) {
    return call::refused(who, why);
  }
  PdcchStage&   s = pdcch_stage();
  modem::Params mp;
  const auto    zeroed = [&](int rc) {
    zero();
    return rc;
  };
  if (!s.ready()) {
    return zeroed(call::no_device(who));
  }
  const uint32_t* d_tab[3];
  reserve_all_cfi(s.tables, *sf);
  for (uint32_t c = 0; c < 3; c++) {
    srsran_hip_pdcch_sf_t one = *sf;
    one.cfi                   = c + 1;
    d_tab[c]                  = s.table(one, *t[c]);
  }
  if (!d_tab[0] || !d_tab[1] || !d_tab[2] || !modem::params_for(mp, modem::LLR_F32)) {
    return zeroed(call::failed(who, "the REG tables or the sequence tables could not be placed on the device"));
  }
  const chest_dl::Layout l       = chest_dl::layout_of(*est);
  const uint32_t         n_pairs = est->nof_rx * est->nof_ports, nsym3 = 4 * t[2]->nregs;
  const bool             want_llr = dbg && dbg->llr_out, want_rm = dbg && dbg->rm_f, want_sym = dbg && dbg->symbols;
  bool                   want_g   = false;
  for (uint32_t i = 0; dbg && dbg->ce_grid_out && i < n_pairs; i++) {
    want_g = want_g || dbg->ce_grid_out[i % est->nof_ports][i / est->nof_ports];
  }
  const size_t gb = (size_t)l.grid_points * sizeof(cf_t);
  const size_t o_ej = al256((size_t)l.in_points * sizeof(cf_t)), o_jobs = al256(o_ej + n_pairs * sizeof(chest_dl::Job));
  const size_t o_pj = al256(o_jobs + (size_t)n_jobs * sizeof(conv::DciJob)), up = al256(o_pj + (size_t)n_ph * sizeof(ctrl::PhichJob));
  const size_t o_pc = al256(up + n_pairs * sizeof(chest_dl::Record)), o_cfi = al256(o_pc + sizeof(ctrl::PcfichRow)), o_ph = o_cfi + 256;
  const size_t o_res = al256(o_ph + (size_t)n_ph * sizeof(ctrl::PhichRow)), o_llr = al256(o_res + (size_t)max_n * conv::kDciResRow);
  const size_t o_rm  = al256(o_llr + (size_t)2 * nsym3 * sizeof(float));
  const size_t o_sym = want_rm ? al256(o_rm + (size_t)max_n * conv::kDciSyms * sizeof(float)) : o_rm;
  const size_t o_dn  = want_sym ? al256(o_sym + (size_t)max_n * conv::kDciSyms * sizeof(uint16_t)) : o_sym;
  const size_t o_dg = o_dn + 256, end = o_dg + n_pairs * gb;
  const size_t down = want_g ? end : (want_rm || want_sym) ? o_dn : want_llr ? o_rm : o_llr;
  if (!s.grow(end)) {
    return zeroed(call::failed(who, "the staging allocation failed"));
  }
  chest_dl::stage_input(reinterpret_cast<cf_t*>(s.pin.get()), *est, l, sf_symbols);
  auto* ejobs = reinterpret_cast<chest_dl::Job*>(s.pin + o_ej);
  chest_dl::make_jobs(ejobs, *est, *state_in, l);
  const uint32_t gstride = l.grid_points; // of the received grids in the estimator's input and of the ce grids alike
  for (uint32_t i = 0; i < n_pairs; i++) { // the ce grids in the order of the planes: [port][rx]
    ejobs[i].o_ce = ((i % est->nof_ports) * est->nof_rx + i / est->nof_ports) * gstride;
  }
  conv::DciJob* jobs = reinterpret_cast<conv::DciJob*>(s.pin + o_jobs);
  for (uint32_t i = 0; i < n_jobs; i++) {
    jobs[i] = conv::dci_job(cand[i]);
  }
  ctrl::phich_jobs(reinterpret_cast<ctrl::PhichJob*>(s.pin + o_pj), *t[0], *sf, n_ph, phich);
  const modem::NoiseAvg  noise = {reinterpret_cast<const float*>(s.dev + o_dn), est->nof_rx, est->nof_ports};
  uint32_t*              d_cfi = reinterpret_cast<uint32_t*>(s.dev + o_cfi);
  const chest_dl::Params ep    = {reinterpret_cast<const float2*>(s.dev.get()), reinterpret_cast<float2*>(s.dev + o_dg), reinterpret_cast<const chest_dl::Job*>(s.dev + o_ej),
                                  reinterpret_cast<chest_dl::Record*>(s.dev + up), reinterpret_cast<float*>(s.dev + o_dn), n_pairs, l.in_points, n_pairs * gstride};
  ctrl::Params           cp    = {};
  cp.rx                        = reinterpret_cast<const float2*>(s.dev.get());
  cp.ce                        = reinterpret_cast<const float2*>(s.dev + o_dg);
  cp.stride                    = gstride;
  cp.ports                     = sf->cell_nof_ports;
  cp.nof_rx                    = sf->nof_rx;
  cp.ext                       = sf->cp_nsymb == 6;
  cp.noise_dev                 = noise;
  cp.seed                      = ctrl::c_init(*sf);
  cp.qpsk_f                    = mp.k.qpsk_f;
  cp.x1_bits                   = mp.x1_bits;
  cp.x2_cols                   = mp.x2_cols;
  cp.pcfich                    = 1;
  memcpy(cp.pcfich_idx, t[0]->pcfich, sizeof(cp.pcfich_idx));
  cp.pcfich_out = reinterpret_cast<ctrl::PcfichRow*>(s.dev + o_pc);
  cp.jobs       = reinterpret_cast<const ctrl::PhichJob*>(s.dev + o_pj);
  cp.n_phich    = n_ph;
  cp.phich_out  = reinterpret_cast<ctrl::PhichRow*>(s.dev + o_ph);
  cp.cfi3_to_2  = opt->cfi3_to_2;
  cp.cfi_word   = d_cfi;
  pdcch::FrontParams fp = {};
  fp.planes             = cp.rx;
  fp.ce                 = cp.ce;
  fp.plane_stride       = gstride;
  fp.tab                = d_tab[2];
  fp.nsym               = nsym3;
  fp.ports              = sf->cell_nof_ports;
  fp.nof_rx             = sf->nof_rx;
  fp.noise_dev          = noise;
  fp.seed               = sf->sf_idx * 512 + sf->cell_id;
  fp.qpsk_f             = mp.k.qpsk_f;
  fp.x1_bits            = mp.x1_bits;
  fp.x2_cols            = mp.x2_cols;
  fp.llr                = reinterpret_cast<float*>(s.dev + o_llr);
  fp.cfi_dev            = d_cfi;
  conv::DciSel sel      = {d_cfi, {first[0], first[1], first[2]}, {opt->n_cand[0], opt->n_cand[1], opt->n_cand[2]}};
  for (uint32_t c = 0; c < 3; c++) {
    fp.tab3[c]  = d_tab[c];
    fp.nsym3[c] = 4 * t[c]->nregs;
  }
  const auto enqueue = [&](hipStream_t st) {
    hipError_t e = chest_dl::launch(ep, st);
    if (e == hipSuccess) {
      e = ctrl::launch(cp, st);
    }
    if (e == hipSuccess) {
      e = pdcch::launch_front(fp, st);
    }
    if (e == hipSuccess) {
      e = conv::launch_pdcch_dci_sf(fp.llr, reinterpret_cast<const conv::DciJob*>(s.dev + o_jobs), s.dev + o_res, want_rm ? reinterpret_cast<float*>(s.dev + o_rm) : nullptr,
                                    want_sym ? reinterpret_cast<uint16_t*>(s.dev + o_sym) : nullptr, max_n, st, &sel);
    }
    return e;
  };
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, down - up, enqueue)) {
    return zeroed(SRSRAN_ERROR);
  }
  const ctrl::PcfichRow* row = reinterpret_cast<const ctrl::PcfichRow*>(s.pin + o_pc);
  const uint32_t         c   = *reinterpret_cast<const uint32_t*>(s.pin + o_cfi) - 1;
  if (c > 2) {
    return zeroed(call::failed(who, "the CFI word left by the device is not 1 .. 3"));
  }
  const uint32_t n = opt->n_cand[c];
  *cfi             = c + 1;
  if (cfi_corr) {
    *cfi_corr = row->corr;
  }
  memcpy(res, s.pin + o_res, (size_t)n * sizeof(*res)); // the rows past the chosen list's length stay zero
  if (n_ph) {
    memcpy(phich_res, s.pin + o_ph, (size_t)n_ph * sizeof(*phich_res));
  }
  chest_dl::finish(*est, *state_in, reinterpret_cast<const chest_dl::Record*>(s.pin + up), srsran_symbol_sz(est->nof_prb), est_out);
  if (dbg) {
    if (want_llr) {
      memcpy(dbg->llr_out, s.pin + o_llr, (size_t)8 * t[c]->nregs * sizeof(float));
    }
    if (dbg->pcfich_data_f) {
      memcpy(dbg->pcfich_data_f, row->data_f, sizeof(row->data_f));
    }
    if (want_rm) {
      memset(dbg->rm_f, 0, (size_t)max_n * conv::kDciSyms * sizeof(float));
      memcpy(dbg->rm_f, s.pin + o_rm, (size_t)n * conv::kDciSyms * sizeof(float));
    }
    if (want_sym) {
      memset(dbg->symbols, 0, (size_t)max_n * conv::kDciSyms * sizeof(uint16_t));
      memcpy(dbg->symbols, s.pin + o_sym, (size_t)n * conv::kDciSyms * sizeof(uint16_t));
    }
    for (uint32_t i = 0; want_g && i < n_pairs; i++) {
      if (cf_t* g = dbg->ce_grid_out[i % est->nof_ports][i / est->nof_ports]) {
        memcpy(g, s.pin + o_dg + (size_t)ejobs[i].o_ce * sizeof(cf_t), gb);
      }
    }
  }
  return SRSRAN_SUCCESS;
}

} // namespace

const pdcch_map::Table* pdcch_map::table_of(const srsran_hip_pdcch_sf_t* sf, const char** why)
{
  if (!sf) {
    *why = "NULL argument";
    return nullptr;
  }
  *why = pdcch_map::invalid(*sf);
  if (*why) {
    return nullptr;
  }
  const pdcch_map::Table* t = host_table(*sf);
  if (!t) {
    *why = "the PCFICH and PHICH of this description leave the PDCCH of some cfi without REGs";
  }
  return t;
}

extern "C" int srsran_hip_regs_pdcch_nregs(const srsran_hip_pdcch_sf_t* sf)
{
  const char*             why;
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  return t ? (int)t->nregs : -1;
}

extern "C" int srsran_hip_regs_pdcch_table(const srsran_hip_pdcch_sf_t* sf, uint32_t* re_idx)
{
  const char*             why;
  const pdcch_map::Table* t = pdcch_map::table_of(sf, &why);
  if (!t || !re_idx) {
    return -1;
  }
  memcpy(re_idx, t->re_idx.data(), t->re_idx.size() * sizeof(uint32_t));
  return (int)t->nregs;
}

extern "C" int srsran_hip_regs_pdcch_get(const srsran_hip_pdcch_sf_t* sf, uint32_t n_planes, const cf_t* const* grids, cf_t* const* d)
{
  const char*             who = "srsran_hip_regs_pdcch_get";
  TraceRange              trace_(who);
  const char*             why = nullptr;
  const pdcch_map::Table* t   = pdcch_map::table_of(sf, &why);
  if (!why && (!grids || !d || n_planes == 0 || n_planes > pdcch::kMaxPlanes)) {
    why = "NULL argument, or not 1 .. 10 planes";
  }
  for (uint32_t p = 0; !why && p < n_planes; p++) {
    why = (!grids[p] || !d[p]) ? "a plane is NULL" : nullptr;
  }
  if (why) {
    call::refused(who, why);
    return -1;
  }
  PdcchStage& s = pdcch_stage();
  if (!s.ready()) {
    call::no_device(who);
    return -1;
  }
  const uint32_t  nsym  = 4 * t->nregs;
  const size_t    pb = plane_bytes(*sf), pstride = al256(pb), xstride = al256((size_t)nsym * sizeof(cf_t)), up = n_planes * pstride, end = up + n_planes * xstride;
  const uint32_t* d_tab = s.table(*sf, *t);
  if (!d_tab || !s.grow(end)) {
    call::failed(who, "the REG table or the staging images could not be allocated");
    return -1;
  }
  for (uint32_t p = 0; p < n_planes; p++) {
    memcpy(s.pin + p * pstride, grids[p], pb);
  }
  const auto enqueue = [&](hipStream_t st) {
    return pdcch::launch_gather(reinterpret_cast<const float2*>(s.dev.get()), (uint32_t)(pstride / sizeof(cf_t)), d_tab, nsym, n_planes,
                                reinterpret_cast<float2*>(s.dev + up), (uint32_t)(xstride / sizeof(cf_t)), st);
  };
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, end - up, enqueue)) {
    return -1;
  }
  for (uint32_t p = 0; p < n_planes; p++) {
    memcpy(d[p], s.pin + up + p * xstride, (size_t)nsym * sizeof(cf_t));
  }
  return (int)nsym;
}

extern "C" int srsran_hip_pdcch_extract_llr(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                            float* llr)
{
  if (!llr) {
    return call::refused("srsran_hip_pdcch_extract_llr", "NULL argument");
  }
  return run("srsran_hip_pdcch_extract_llr", sf, sf_symbols, ce, noise_estimate, 0, nullptr, nullptr, llr, nullptr);
}

extern "C" int srsran_hip_pdcch_search_sf(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                          uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res)
{
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  return run("srsran_hip_pdcch_search_sf", sf, sf_symbols, ce, noise_estimate, n, cand, res, nullptr, nullptr);
}

extern "C" int srsran_hip_pdcch_search_sf_dbg(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                              uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, float* llr_out, cf_t* d_out,
                                              cf_t* const* sym_out, cf_t* const (*ce_out)[SRSRAN_MAX_PORTS], float* rm_f, uint16_t* symbols)
{
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  const Dbg dbg = {llr_out, d_out, sym_out, ce_out, rm_f, symbols};
  return run("srsran_hip_pdcch_search_sf_dbg", sf, sf_symbols, ce, noise_estimate, n, cand, res, nullptr, &dbg);
}

extern "C" int srsran_hip_pdcch_search_est(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
                                           cf_t* const sf_symbols[], const srsran_hip_pdcch_est_t* opt, const srsran_hip_pdcch_cand_t* cand,
                                           srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* phich, srsran_hip_phich_res_t* phich_res, uint32_t* cfi,
                                           float* cfi_corr, srsran_hip_chest_dl_res_t* est_out)
{
  return run_est("srsran_hip_pdcch_search_est", sf, est, state_in, sf_symbols, opt, cand, res, phich, phich_res, cfi, cfi_corr, est_out, nullptr);
}

extern "C" int srsran_hip_pdcch_search_est_dbg(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
                                               cf_t* const sf_symbols[], const srsran_hip_pdcch_est_t* opt, const srsran_hip_pdcch_cand_t* cand,
                                               srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* phich, srsran_hip_phich_res_t* phich_res,
                                               uint32_t* cfi, float* cfi_corr, srsran_hip_chest_dl_res_t* est_out, float* llr_out, float pcfich_data_f[32],
                                               cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS], float* rm_f, uint16_t* symbols)
{
  const EstDbg dbg = {llr_out, pcfich_data_f, ce_grid_out, rm_f, symbols};
  return run_est("srsran_hip_pdcch_search_est_dbg", sf, est, state_in, sf_symbols, opt, cand, res, phich, phich_res, cfi, cfi_corr, est_out, &dbg);
}
