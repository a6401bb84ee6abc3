// pdcch_host.cpp -- the PDCCH search of a subframe from the received grids (include/srsran_amd/phy_conv_abi.h: srsran_hip_regs_pdcch_*,
// srsran_hip_pdcch_extract_llr, srsran_hip_pdcch_search_sf{,_dbg}).  The REG map is pdcch_map.h's; the front end is pdcch_kernels.hip; the decodes, with the mean
// rule on the device, are conv_kernels.hip's pdcch_dci_sf_kernel.  A search is one upload, two launches, one download and one host wait on the calling
// thread's staging context (stage.h).  One layout serves the pinned image and the device buffer:
//   [candidates | the region's rows of every plane || results | soft bits | _dbg: de-matched floats | symbols | equalised symbols | extracted planes]
// what is in front of || goes up; of what is behind, a search brings down the results, srsran_hip_pdcch_extract_llr the soft bits, _dbg everything.
// A description's table is built once per thread and uploaded once per staging context; both caches are small and start over when they are full (nothing
// of the thread's is in flight between two calls).
#include "conv_device.h"
#include "modem_device.h"
#include "pdcch_device.h"
#include "pdcch_map.h"
#include "stage.h"
#include "srsran_amd/phy_conv_abi.h"

#include <memory>
#include <string>

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

// the table of a description that has passed pdcch_map::invalid(), built once per thread; nullptr: the rules are not defined on it
const pdcch_map::Table* host_table(const srsran_hip_pdcch_sf_t& sf)
{
  static thread_local std::vector<std::unique_ptr<HostTable>> cache;
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

struct PdcchStage {
  StageStream                               st;
  HostImage                                 pin;
  DeviceBuf                                 dev;
  std::vector<std::unique_ptr<DeviceTable>> tables;
  bool                                      ready() { return st.open(); }
  bool                                      grow(size_t need) { return pin.grow(need, need / 2) && dev.grow(need, need / 2); }
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

int refuse(const char* who, const char* why)
{
  fprintf(stderr, "[srsran_phy_hip] %s: %s\n", who, why);
  return SRSRAN_ERROR_INVALID_INPUTS;
}

// a description the calls take: in range, and one the reference's own initialisation succeeds on
const pdcch_map::Table* table_of(const srsran_hip_pdcch_sf_t* sf, const char** why)
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
  const pdcch_map::Table* t = table_of(sf, &why);
  if (!why && (!sf_symbols || !ce || (search && (!cand || !res)))) {
    why = "NULL argument";
  }
  if (!why && n > SRSRAN_HIP_PDCCH_MAX_CANDIDATES) {
    why = "more than 256 candidates";
  }
  for (uint32_t a = 0; !why && a < sf->nof_rx; a++) {
    why = !sf_symbols[a] ? "a received grid is NULL" : nullptr;
    for (uint32_t p = 0; !why && p < sf->cell_nof_ports; p++) {
      why = !ce[p][a] ? "an estimate grid is NULL" : nullptr;
    }
  }
  const uint32_t nsym = t ? 4 * t->nregs : 0, nof_llr = 2 * nsym;
  for (uint32_t i = 0; i < n && !why; i++) {
    if (cand[i].L > 3) {
      why = "aggregation level above 3";
    } else if ((uint64_t)cand[i].ncce * 72 + (72u << cand[i].L) > nof_llr) {
      why = "a location past the end of the control region";
    } else if (cand[i].nof_bits == 0 || cand[i].nof_bits > SRSRAN_HIP_DCI_MAX_BITS) {
      why = "nof_bits outside 1 .. 128";
    }
  }
  if (why) {
    return refuse(who, why);
  }
  PdcchStage&   s = pdcch_stage();
  modem::Params mp;
  const auto    fail = [&](const char* what) {
    fprintf(stderr, "[srsran_phy_hip] %s: %s\n", who, what);
    if (search) {
      memset(res, 0, (size_t)n * sizeof(*res));
    }
    return SRSRAN_ERROR;
  };
  if (!s.ready()) {
    const std::string text = std::string(get_error()) + " (there is no CPU fallback)";
    return fail(text.c_str());
  }
  const uint32_t* d_tab = s.table(*sf, *t);
  if (!d_tab || !modem::params_for(mp, modem::LLR_F32)) {
    return fail("the REG table or the sequence tables could not be placed on the device");
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
    return fail("the staging allocation failed");
  }
  conv::DciJob* jobs = reinterpret_cast<conv::DciJob*>(s.pin.get());
  for (uint32_t i = 0; i < n; i++) {
    jobs[i] = conv::DciJob{cand[i].ncce * 72, 72u << cand[i].L, cand[i].nof_bits};
  }
  for (uint32_t a = 0; a < sf->nof_rx; a++) {
    memcpy(s.pin + o_planes + a * pstride, sf_symbols[a], pb);
    for (uint32_t p = 0; p < sf->cell_nof_ports; p++) {
      memcpy(s.pin + o_planes + (sf->nof_rx + p * sf->nof_rx + a) * pstride, ce[p][a], pb);
    }
  }
  pdcch::FrontParams fp;
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
  hipError_t e    = hipMemcpyAsync(s.dev, s.pin, up, hipMemcpyHostToDevice, s.st);
  if (e == hipSuccess) {
    e = pdcch::launch_front(fp, s.st);
  }
  if (e == hipSuccess) {
    e = conv::launch_pdcch_dci_sf(fp.llr, reinterpret_cast<const conv::DciJob*>(s.dev.get()), s.dev + up, want_rm ? reinterpret_cast<float*>(s.dev + o_rm) : nullptr,
                                  want_sym ? reinterpret_cast<uint16_t*>(s.dev + o_sym) : nullptr, n, s.st);
  }
  if (e == hipSuccess && down > up) {
    e = hipMemcpyAsync(s.pin + up, s.dev + up, down - up, hipMemcpyDeviceToHost, s.st);
  }
  const hipError_t w = hipStreamSynchronize(s.st);
  e                  = e != hipSuccess ? e : w;
  if (e != hipSuccess) {
    set_error("%s: %s", who, hipGetErrorString(e));
    return fail(get_error());
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

} // namespace

extern "C" int srsran_hip_regs_pdcch_nregs(const srsran_hip_pdcch_sf_t* sf)
{
  const char*             why;
  const pdcch_map::Table* t = table_of(sf, &why);
  return t ? (int)t->nregs : -1;
}

extern "C" int srsran_hip_regs_pdcch_table(const srsran_hip_pdcch_sf_t* sf, uint32_t* re_idx)
{
  const char*             why;
  const pdcch_map::Table* t = table_of(sf, &why);
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
  const pdcch_map::Table* t   = table_of(sf, &why);
  if (!why && (!grids || !d || n_planes == 0 || n_planes > pdcch::kMaxPlanes)) {
    why = "NULL argument, or not 1 .. 10 planes";
  }
  for (uint32_t p = 0; !why && p < n_planes; p++) {
    why = (!grids[p] || !d[p]) ? "a plane is NULL" : nullptr;
  }
  if (why) {
    refuse(who, why);
    return -1;
  }
  PdcchStage& s = pdcch_stage();
  if (!s.ready()) {
    fprintf(stderr, "[srsran_phy_hip] %s: %s (there is no CPU fallback)\n", who, get_error());
    return -1;
  }
  const uint32_t  nsym  = 4 * t->nregs;
  const size_t    pb = plane_bytes(*sf), pstride = al256(pb), xstride = al256((size_t)nsym * sizeof(cf_t)), up = n_planes * pstride, end = up + n_planes * xstride;
  const uint32_t* d_tab = s.table(*sf, *t);
  if (!d_tab || !s.grow(end)) {
    fprintf(stderr, "[srsran_phy_hip] %s: the REG table or the staging images could not be allocated\n", who);
    return -1;
  }
  for (uint32_t p = 0; p < n_planes; p++) {
    memcpy(s.pin + p * pstride, grids[p], pb);
  }
  hipError_t e = hipMemcpyAsync(s.dev, s.pin, up, hipMemcpyHostToDevice, s.st);
  if (e == hipSuccess) {
    e = pdcch::launch_gather(reinterpret_cast<const float2*>(s.dev.get()), (uint32_t)(pstride / sizeof(cf_t)), d_tab, nsym, n_planes,
                             reinterpret_cast<float2*>(s.dev + up), (uint32_t)(xstride / sizeof(cf_t)), s.st);
  }
  if (e == hipSuccess) {
    e = hipMemcpyAsync(s.pin + up, s.dev + up, end - up, hipMemcpyDeviceToHost, s.st);
  }
  const hipError_t w = hipStreamSynchronize(s.st);
  e                  = e != hipSuccess ? e : w;
  if (e != hipSuccess) {
    set_error("%s: %s", who, hipGetErrorString(e));
    fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
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
    return refuse("srsran_hip_pdcch_extract_llr", "NULL argument");
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
