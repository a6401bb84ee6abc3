// pbch_host.cpp -- PBCH / MIB decoding (include/srsran_amd/phy_pbch_abi.h).  The rules are pbch_map.h's, the kernel is pbch_kernels.hip.  Every call is one
// round trip (call_frame.h) on the calling thread's staging context: srsran_hip_pbch_try_frames, _decode and _decode_multi with ONE launch,
// srsran_hip_pbch_decode_est with TWO (chest_dl::launch, then pbch::launch, chained in one enqueue: no host wait between them).  The host picks the first hit
// in the reference's order from the job rows that came down and advances the caller's state.
// One layout serves the pinned image and the device buffer; what is in front of || goes up, what is behind comes down:
//   [decode_est: the estimator's input | its jobs] [cells | jobs | sequences | the cells' four soft-bit rows | decode: the 4 x 72 rows of every plane ||
//    decode_est: the estimator's records] [job rows | newest rows | _dbg: de-matched floats | symbols | equalised symbols | newest rows per hypothesis
//    ||| decode_est, device only: the pairs' noise estimates | the ce grids [port][rx]]
#include "call_frame.h"
#include "chest_dl_device.h"
#include "pbch_device.h"
#include "srsran_amd/phy_pbch_abi.h"

#include <cmath>
#include <vector>

using namespace phyhip;

static_assert(sizeof(srsran_hip_pbch_cell_t) == 16 && sizeof(srsran_hip_pbch_state_t) == 7684 && sizeof(srsran_hip_pbch_res_t) == 48, "phy_pbch_abi.h layout");
static_assert(sizeof(srsran_hip_pbch_row_t) == pbch::kOutRow && offsetof(srsran_hip_pbch_row_t, crc_rem) == pbch::kBits &&
                  offsetof(srsran_hip_pbch_row_t, ones) == pbch::kBits + 2,
              "pbch_kernel writes its rows in this layout");
static_assert(SRSRAN_HIP_PBCH_MAX_RE == pbch_map::kMaxRe && SRSRAN_HIP_PBCH_MAX_BITS == pbch_map::kMaxBits && SRSRAN_HIP_PBCH_MAX_COMBOS == pbch_map::kMaxCombos &&
                  SRSRAN_HIP_PBCH_MAX_CELLS == pbch::kMaxCells && SRSRAN_HIP_PBCH_PAYLOAD_LEN == pbch_map::kPayload,
              "limits");

namespace {

struct PbchStage : call::Stage {};

PbchStage& pbch_stage() // of the calling thread, on the device it is bound to
{
  static thread_local StageRef<PbchStage> r;
  return r.get();
}

constexpr uint32_t kPlanePoints = pbch_map::kRows * pbch_map::kCols; // what is staged of a plane

const char* cell_invalid(const srsran_hip_pbch_cell_t& c)
{
  if (c.nof_prb < 6 || c.nof_prb > 110 || c.id > 503 || (c.cp_nsymb != 7 && c.cp_nsymb != 6) || c.nof_ports > 4) {
    return "a cell field is out of range";
  }
  if (c.nof_ports == 3) {
    return "3 ports are not a PBCH hypothesis";
  }
  return nullptr;
}

struct Dbg {
  cf_t*                  d;
  float*                 llr_new;
  srsran_hip_pbch_row_t* rows;
  uint32_t*              n_rows;
};

// the jobs of a call and where its regions lie, from `base` on
struct Plan {
  uint32_t               n_cells = 0, n_slots = 0;
  pbch::Cell             cells[pbch::kMaxCells];
  uint32_t               first_job[pbch::kMaxCells + 1] = {0};
  std::vector<pbch::Job> jobs;
  size_t                 o_cells, o_jobs, o_seq, o_hist, o_planes, up, o_rows, o_new, o_rm, o_sym, o_d, o_llr, end;

  // nant 0 in `stage_only`: the combinations once, on the caller's rows
  void add(const srsran_hip_pbch_cell_t& c, uint32_t f, float noise, bool stage_only)
  {
    const uint32_t i = n_cells++;
    uint32_t       nant[3], nl = stage_only ? 1 : pbch_map::nant_list(c.nof_ports, nant);
    pbch::Cell&    k = cells[i];
    k                = {};
    k.id             = c.id;
    k.cp_nsymb       = c.cp_nsymb;
    k.f              = f;
    k.last_nant      = stage_only ? 0xFFu : nant[nl - 1];
    k.noise          = noise;
    k.o_hist         = i * 4 * pbch_map::kMaxBits;
    k.o_seq          = i * pbch_map::kSeqWords;
    k.o_new          = i * pbch_map::kMaxBits;
    k.first_slot     = n_slots;
    for (uint32_t h = 0; h < nl; h++) {
      for (uint32_t cmb = 0; cmb < pbch_map::nof_combos(f); cmb++) {
        jobs.push_back(pbch::Job{(uint8_t)i, (uint8_t)(stage_only ? 0 : nant[h]), (uint8_t)cmb, (uint8_t)h});
      }
    }
    n_slots += nl;
    first_job[n_cells] = (uint32_t)jobs.size();
  }
  void lay_out(size_t base, size_t plane_bytes, size_t between, bool dbg)
  {
    const size_t nj = jobs.size();
    o_cells  = base;
    o_jobs   = al256(o_cells + sizeof(cells));
    o_seq    = al256(o_jobs + nj * sizeof(pbch::Job));
    o_hist   = al256(o_seq + (size_t)n_cells * pbch_map::kSeqWords * 4);
    o_planes = al256(o_hist + (size_t)n_cells * 4 * pbch_map::kMaxBits * sizeof(float));
    up       = al256(o_planes + plane_bytes);
    o_rows   = al256(up + between);
    o_new    = al256(o_rows + nj * pbch::kOutRow);
    o_rm     = al256(o_new + (size_t)n_cells * pbch_map::kMaxBits * sizeof(float));
    o_sym    = dbg ? al256(o_rm + nj * pbch_map::kCoded * sizeof(float)) : o_rm;
    o_d      = dbg ? al256(o_sym + nj * pbch_map::kCoded * sizeof(uint16_t)) : o_rm;
    o_llr    = dbg ? al256(o_d + (size_t)n_slots * pbch_map::kMaxRe * sizeof(cf_t)) : o_rm;
    end      = dbg ? al256(o_llr + (size_t)n_slots * pbch_map::kMaxBits * sizeof(float)) : o_rm;
  }
  // cells, jobs, sequences and history rows into the image
  void stage(uint8_t* pin, const float* const* hist, const uint32_t* rows_of) const
  {
    memcpy(pin + o_cells, cells, sizeof(cells));
    memcpy(pin + o_jobs, jobs.data(), jobs.size() * sizeof(pbch::Job));
    for (uint32_t i = 0; i < n_cells; i++) {
      pbch_map::sequence(cells[i].id, reinterpret_cast<uint32_t*>(pin + o_seq) + cells[i].o_seq);
      float*       h = reinterpret_cast<float*>(pin + o_hist) + cells[i].o_hist;
      const size_t n = (size_t)rows_of[i] * 2 * pbch_map::nof_re(cells[i].cp_nsymb);
      memcpy(h, hist[i], n * sizeof(float));
      memset(h + n, 0, (4 * pbch_map::kMaxBits - n) * sizeof(float));
    }
  }
  pbch::Params params(uint8_t* dev, bool dbg, float qpsk_f) const
  {
    pbch::Params p = {};
    p.planes       = reinterpret_cast<const float2*>(dev);
    p.cells        = reinterpret_cast<const pbch::Cell*>(dev + o_cells);
    p.jobs         = reinterpret_cast<const pbch::Job*>(dev + o_jobs);
    p.hist         = reinterpret_cast<const float*>(dev + o_hist);
    p.seq          = reinterpret_cast<const uint32_t*>(dev + o_seq);
    p.rows         = dev + o_rows;
    p.newest       = reinterpret_cast<float*>(dev + o_new);
    p.dbg_rm       = dbg ? reinterpret_cast<float*>(dev + o_rm) : nullptr;
    p.dbg_sym      = dbg ? reinterpret_cast<uint16_t*>(dev + o_sym) : nullptr;
    p.dbg_d        = dbg ? reinterpret_cast<float2*>(dev + o_d) : nullptr;
    p.dbg_llr      = dbg ? reinterpret_cast<float*>(dev + o_llr) : nullptr;
    p.qpsk_f       = qpsk_f;
    p.n_jobs       = (uint32_t)jobs.size();
    return p;
  }
  // what came down for cell i -> *res, *state (pbch.c:489-556) and the _dbg outputs
  void finish(const uint8_t* pin, uint32_t i, srsran_hip_pbch_state_t* state, srsran_hip_pbch_res_t* res, const Dbg* dbg) const
  {
    const pbch::Cell& k        = cells[i];
    const uint32_t    nof_bits = 2 * pbch_map::nof_re(k.cp_nsymb), f = k.f;
    const auto*       rows     = reinterpret_cast<const srsran_hip_pbch_row_t*>(pin + o_rows);
    *res                       = {};
    memcpy(state->llr + (size_t)(f - 1) * nof_bits, reinterpret_cast<const float*>(pin + o_new) + k.o_new, nof_bits * sizeof(float));
    state->frame_idx = f;
    for (uint32_t j = first_job[i]; j < first_job[i + 1]; j++) {
      if (pbch_map::verdict(rows[j].crc_rem, rows[j].ones, jobs[j].nant)) {
        uint32_t nb, dst, src;
        pbch_map::combo(f, jobs[j].combo, &nb, &dst, &src);
        res->ret          = 1;
        res->nof_tx_ports = jobs[j].nant;
        res->sfn_offset   = (int32_t)dst - (int32_t)src + (int32_t)f - 1;
        res->src = src, res->dst = dst, res->nb = nb;
        memcpy(res->payload, rows[j].bits, pbch_map::kPayload);
        state->frame_idx = 0;
        break;
      }
    }
    if (state->frame_idx == 4) { // make room for the next frame
      memmove(state->llr, state->llr + nof_bits, (size_t)3 * nof_bits * sizeof(float));
      state->frame_idx = 3;
    }
    if (dbg) {
      const uint32_t nj = first_job[i + 1] - first_job[i], nl = nj / pbch_map::nof_combos(f);
      if (dbg->rows) {
        memcpy(dbg->rows, rows + first_job[i], (size_t)nj * sizeof(*rows));
      }
      if (dbg->n_rows) {
        *dbg->n_rows = nj;
      }
      if (dbg->d) {
        memset(dbg->d, 0, (size_t)3 * pbch_map::kMaxRe * sizeof(cf_t));
        memcpy(dbg->d, pin + o_d + (size_t)k.first_slot * pbch_map::kMaxRe * sizeof(cf_t), (size_t)nl * pbch_map::kMaxRe * sizeof(cf_t));
      }
      if (dbg->llr_new) {
        memset(dbg->llr_new, 0, (size_t)3 * pbch_map::kMaxBits * sizeof(float));
        memcpy(dbg->llr_new, pin + o_llr + (size_t)k.first_slot * pbch_map::kMaxBits * sizeof(float), (size_t)nl * pbch_map::kMaxBits * sizeof(float));
      }
    }
  }
};

void zero_dbg(const Dbg* dbg)
{
  if (dbg && dbg->n_rows) {
    *dbg->n_rows = 0;
  }
}

uint32_t ports_tried(const srsran_hip_pbch_cell_t& c)
{
  return c.nof_ports ? c.nof_ports : 4;
}

// srsran_hip_pbch_decode{,_dbg} (n == 1) and _multi
int run(const char* who, uint32_t n, const srsran_hip_pbch_cell_t* cells, srsran_hip_pbch_state_t* const* states, const cf_t* const* rx,
        const cf_t* const (*ce)[SRSRAN_MAX_PORTS], const float* noise, srsran_hip_pbch_res_t* res, const Dbg* dbg)
{
  TraceRange  trace_(who);
  const char* why = nullptr;
  zero_dbg(dbg);
  if (res && n <= pbch::kMaxCells) {
    memset(res, 0, (size_t)n * sizeof(*res));
  }
  if (n > pbch::kMaxCells) {
    why = "more than 8 cells";
  } else if (!cells || !states || !rx || !ce || !noise || !res) {
    why = "NULL argument";
  }
  for (uint32_t i = 0; !why && i < n; i++) {
    if (!states[i]) {
      why = "NULL argument";
    } else if (!(why = cell_invalid(cells[i]))) {
      if (states[i]->frame_idx > 3) {
        why = "frame_idx is above 3";
      } else if (!std::isfinite(noise[i])) {
        why = "noise_estimate is not finite";
      } else if (!rx[i]) {
        why = "a plane is NULL";
      }
      for (uint32_t p = 0; !why && p < ports_tried(cells[i]); p++) {
        why = !ce[i][p] ? "a plane is NULL" : nullptr;
      }
    }
  }
  if (why) {
    return call::refused(who, why);
  }
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  PbchStage&    s = pbch_stage();
  modem::Params mp;
  if (!s.ready()) {
    return call::no_device(who);
  }
  if (!modem::params_for(mp, modem::LLR_F32)) {
    return call::failed(who, "the demodulator's constants could not be placed on the device");
  }
  Plan         pl;
  const float* hist[pbch::kMaxCells];
  uint32_t     rows_of[pbch::kMaxCells];
  for (uint32_t i = 0; i < n; i++) {
    pl.add(cells[i], states[i]->frame_idx + 1, noise[i], false);
    hist[i]    = states[i]->llr;
    rows_of[i] = states[i]->frame_idx; // the rows below the newest
  }
  pl.lay_out(0, (size_t)n * 5 * kPlanePoints * sizeof(cf_t), 0, dbg != nullptr);
  if (!s.grow(pl.end)) {
    return call::failed(who, "the staging allocation failed");
  }
  pl.stage(s.pin, hist, rows_of);
  for (uint32_t i = 0; i < n; i++) { // slot 1's first four symbols, the 72 centre sub-carriers, of the received grid and of every estimate tried
    const uint32_t row = 12 * cells[i].nof_prb, o = cells[i].cp_nsymb * row + pbch_map::first_col(cells[i].nof_prb);
    cf_t*          at  = reinterpret_cast<cf_t*>(s.pin + pl.o_planes) + (size_t)i * 5 * kPlanePoints;
    for (uint32_t p = 0; p <= ports_tried(cells[i]); p++) {
      const cf_t* g = p == 0 ? rx[i] : ce[i][p - 1];
      for (uint32_t r = 0; r < pbch_map::kRows; r++) {
        memcpy(at + p * kPlanePoints + r * pbch_map::kCols, g + o + (size_t)r * row, pbch_map::kCols * sizeof(cf_t));
      }
    }
    pbch::Cell& k = pl.cells[i];
    k.o_rx        = (uint32_t)(pl.o_planes / sizeof(cf_t)) + i * 5 * kPlanePoints;
    k.o_ce        = k.o_rx + kPlanePoints;
    k.ce_stride   = kPlanePoints;
    k.row_stride  = pbch_map::kCols;
  }
  memcpy(s.pin + pl.o_cells, pl.cells, sizeof(pl.cells));
  const pbch::Params kp      = pl.params(s.dev, dbg != nullptr, mp.k.qpsk_f);
  const auto         enqueue = [&](hipStream_t st) { return pbch::launch(kp, st); };
  if (!call::round_trip(who, s.st, s.pin, s.dev, pl.up, pl.up, pl.end - pl.up, enqueue)) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < n; i++) {
    pl.finish(s.pin, i, states[i], &res[i], dbg);
  }
  return SRSRAN_SUCCESS;
}

int run_try(const char* who, const srsran_hip_pbch_cell_t* cell, const float* llr, uint32_t frame_idx, srsran_hip_pbch_row_t* rows, float* rm_f, uint16_t* symbols)
{
  TraceRange  trace_(who);
  const char* why = nullptr;
  if (!cell || !llr || !rows) {
    why = "NULL argument";
  } else if (!(why = cell_invalid(*cell)) && (frame_idx < 1 || frame_idx > 4)) {
    why = "frame_idx is outside 1 .. 4";
  }
  if (why) {
    return call::refused(who, why);
  }
  const uint32_t nj = pbch_map::nof_combos(frame_idx);
  memset(rows, 0, (size_t)nj * sizeof(*rows));
  PbchStage& s = pbch_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  Plan pl;
  pl.add(*cell, frame_idx, 0.f, true);
  const bool dbg = rm_f || symbols;
  pl.lay_out(0, 0, 0, dbg);
  if (!s.grow(pl.end)) {
    return call::failed(who, "the staging allocation failed");
  }
  pl.stage(s.pin, &llr, &frame_idx);
  pbch::Params kp = pl.params(s.dev, dbg, 0.f);
  kp.dbg_d        = nullptr;
  kp.dbg_llr      = nullptr;
  const auto enqueue = [&](hipStream_t st) { return pbch::launch(kp, st); };
  if (!call::round_trip(who, s.st, s.pin, s.dev, pl.up, pl.up, pl.end - pl.up, enqueue)) {
    return SRSRAN_ERROR;
  }
  memcpy(rows, s.pin + pl.o_rows, (size_t)nj * sizeof(*rows));
  if (rm_f) {
    memcpy(rm_f, s.pin + pl.o_rm, (size_t)nj * pbch_map::kCoded * sizeof(float));
  }
  if (symbols) {
    memcpy(symbols, s.pin + pl.o_sym, (size_t)nj * pbch_map::kCoded * sizeof(uint16_t));
  }
  return (int)nj;
}

int run_est(const char* who, const srsran_hip_pbch_cell_t* cell, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
            srsran_hip_pbch_state_t* state, cf_t* const sf_symbols[], srsran_hip_pbch_res_t* res, srsran_hip_chest_dl_res_t* est_out, const Dbg* dbg)
{
  TraceRange  trace_(who);
  const char* why = nullptr;
  zero_dbg(dbg);
  if (res) {
    *res = {};
  }
  if (est_out) {
    *est_out = {};
  }
  if (!cell || !est || !state_in || !state || !sf_symbols || !res || !est_out) {
    why = "NULL argument";
  } else if (!(why = cell_invalid(*cell)) && !(why = chest_dl::invalid(est, state_in))) {
    if (est->nof_prb != cell->nof_prb || est->id != cell->id || est->cp_nsymb != cell->cp_nsymb || est->nof_ports != ports_tried(*cell)) {
      why = "the estimator's cell is not the PBCH cell's";
    } else if (est->sf_idx != 0) {
      why = "the estimator's sf_idx is not 0";
    } else if (state->frame_idx > 3) {
      why = "frame_idx is above 3";
    }
  }
  for (uint32_t a = 0; !why && a < est->nof_rx; a++) {
    why = !sf_symbols[a] ? "a plane is NULL" : nullptr;
  }
  if (why) {
    return call::refused(who, why);
  }
  PbchStage&    s = pbch_stage();
  modem::Params mp;
  if (!s.ready()) {
    return call::no_device(who);
  }
  if (!modem::params_for(mp, modem::LLR_F32)) {
    return call::failed(who, "the demodulator's constants could not be placed on the device");
  }
  const chest_dl::Layout l       = chest_dl::layout_of(*est);
  const uint32_t         n_pairs = est->nof_rx * est->nof_ports, gstride = l.grid_points;
  const size_t           o_ej = al256((size_t)l.in_points * sizeof(cf_t)), base = al256(o_ej + n_pairs * sizeof(chest_dl::Job));
  Plan                   pl;
  pl.add(*cell, state->frame_idx + 1, 0.f, false);
  pl.lay_out(base, 0, n_pairs * sizeof(chest_dl::Record), dbg != nullptr);
  const size_t o_rec = pl.up, o_dn = pl.end, o_dg = o_dn + 256, end = o_dg + (size_t)n_pairs * gstride * sizeof(cf_t);
  if (!s.grow(end)) {
    return call::failed(who, "the staging allocation failed");
  }
  chest_dl::stage_input(reinterpret_cast<cf_t*>(s.pin.get()), *est, l, sf_symbols);
  auto* ejobs = reinterpret_cast<chest_dl::Job*>(s.pin + o_ej);
  chest_dl::make_jobs(ejobs, *est, *state_in, l);
  for (uint32_t i = 0; i < n_pairs; i++) { // the ce grids [port][rx]
    ejobs[i].o_ce = ((i % est->nof_ports) * est->nof_rx + i / est->nof_ports) * gstride;
  }
  pbch::Cell& k = pl.cells[0];
  k.o_rx        = cell->cp_nsymb * 12 * cell->nof_prb + pbch_map::first_col(cell->nof_prb); // the first antenna's grid lies at the image's start
  k.o_ce        = (uint32_t)(o_dg / sizeof(cf_t)) + k.o_rx;
  k.ce_stride   = est->nof_rx * gstride;
  k.row_stride  = 12 * cell->nof_prb;
  const float*   hist    = state->llr;
  const uint32_t rows_of = state->frame_idx;
  pl.stage(s.pin, &hist, &rows_of);
  const chest_dl::Params ep = {reinterpret_cast<const float2*>(s.dev.get()), reinterpret_cast<float2*>(s.dev + o_dg), reinterpret_cast<const chest_dl::Job*>(s.dev + o_ej),
                               reinterpret_cast<chest_dl::Record*>(s.dev + o_rec), reinterpret_cast<float*>(s.dev + o_dn), n_pairs, l.in_points, n_pairs * gstride};
  pbch::Params           kp = pl.params(s.dev, dbg != nullptr, mp.k.qpsk_f);
  kp.noise_dev              = modem::NoiseAvg{reinterpret_cast<const float*>(s.dev + o_dn), est->nof_rx, est->nof_ports};
  const auto enqueue        = [&](hipStream_t st) {
    hipError_t e = chest_dl::launch(ep, st);
    if (e == hipSuccess) {
      e = pbch::launch(kp, st);
    }
    return e;
  };
  if (!call::round_trip(who, s.st, s.pin, s.dev, pl.up, pl.up, pl.end - pl.up, enqueue)) {
    return SRSRAN_ERROR;
  }
  chest_dl::finish(*est, *state_in, reinterpret_cast<const chest_dl::Record*>(s.pin + o_rec), srsran_symbol_sz(est->nof_prb), est_out);
  pl.finish(s.pin, 0, state, res, dbg);
  return SRSRAN_SUCCESS;
}

} // namespace

extern "C" int srsran_hip_pbch_nof_re(const srsran_hip_pbch_cell_t* cell)
{
  return (!cell || cell_invalid(*cell)) ? -1 : (int)pbch_map::nof_re(cell->cp_nsymb);
}

extern "C" int srsran_hip_pbch_table(const srsran_hip_pbch_cell_t* cell, uint32_t* re_idx)
{
  if (!cell || !re_idx || cell_invalid(*cell)) {
    return -1;
  }
  const uint32_t n = pbch_map::nof_re(cell->cp_nsymb);
  for (uint32_t i = 0; i < n; i++) {
    re_idx[i] = pbch_map::re_index(i, cell->nof_prb, cell->id, cell->cp_nsymb);
  }
  return (int)n;
}

extern "C" void srsran_hip_pbch_mib_unpack(const uint8_t* payload, uint32_t* nof_prb, uint32_t* phich_length, uint32_t* phich_resources, uint32_t* sfn)
{
  uint32_t v[4] = {0, 0, 0, 0};
  if (payload) {
    pbch_map::mib_unpack(payload, &v[0], &v[1], &v[2], &v[3]);
  }
  uint32_t* const out[4] = {nof_prb, phich_length, phich_resources, sfn};
  for (int i = 0; i < 4; i++) {
    if (out[i]) {
      *out[i] = v[i];
    }
  }
}

extern "C" int srsran_hip_pbch_try_frames(const srsran_hip_pbch_cell_t* cell, const float* llr, uint32_t frame_idx, srsran_hip_pbch_row_t* rows)
{
  return run_try("srsran_hip_pbch_try_frames", cell, llr, frame_idx, rows, nullptr, nullptr);
}

extern "C" int srsran_hip_pbch_try_frames_dbg(const srsran_hip_pbch_cell_t* cell, const float* llr, uint32_t frame_idx, srsran_hip_pbch_row_t* rows, float* rm_f,
                                              uint16_t* symbols)
{
  return run_try("srsran_hip_pbch_try_frames_dbg", cell, llr, frame_idx, rows, rm_f, symbols);
}

extern "C" int srsran_hip_pbch_decode(const srsran_hip_pbch_cell_t* cell, srsran_hip_pbch_state_t* state, const cf_t* sf_symbols0, const cf_t* const ce[SRSRAN_MAX_PORTS],
                                      float noise_estimate, srsran_hip_pbch_res_t* res)
{
  return run("srsran_hip_pbch_decode", 1, cell, &state, &sf_symbols0, reinterpret_cast<const cf_t* const(*)[SRSRAN_MAX_PORTS]>(ce), &noise_estimate, res, nullptr);
}

extern "C" int srsran_hip_pbch_decode_dbg(const srsran_hip_pbch_cell_t* cell, srsran_hip_pbch_state_t* state, const cf_t* sf_symbols0,
                                          const cf_t* const ce[SRSRAN_MAX_PORTS], float noise_estimate, srsran_hip_pbch_res_t* res, cf_t* d, float* llr_new,
                                          srsran_hip_pbch_row_t* rows, uint32_t* n_rows)
{
  const Dbg dbg = {d, llr_new, rows, n_rows};
  return run("srsran_hip_pbch_decode_dbg", 1, cell, &state, &sf_symbols0, reinterpret_cast<const cf_t* const(*)[SRSRAN_MAX_PORTS]>(ce), &noise_estimate, res, &dbg);
}

extern "C" int srsran_hip_pbch_decode_multi(uint32_t n, const srsran_hip_pbch_cell_t* cells, srsran_hip_pbch_state_t* const* states, const cf_t* const* sf_symbols0,
                                            const cf_t* const (*ce)[SRSRAN_MAX_PORTS], const float* noise_estimate, srsran_hip_pbch_res_t* res)
{
  return run("srsran_hip_pbch_decode_multi", n, cells, states, sf_symbols0, ce, noise_estimate, res, nullptr);
}

extern "C" int srsran_hip_pbch_decode_est(const srsran_hip_pbch_cell_t* cell, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* est_state_in,
                                          srsran_hip_pbch_state_t* state, cf_t* const sf_symbols[], srsran_hip_pbch_res_t* res, srsran_hip_chest_dl_res_t* est_out)
{
  return run_est("srsran_hip_pbch_decode_est", cell, est, est_state_in, state, sf_symbols, res, est_out, nullptr);
}

extern "C" int srsran_hip_pbch_decode_est_dbg(const srsran_hip_pbch_cell_t* cell, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* est_state_in,
                                              srsran_hip_pbch_state_t* state, cf_t* const sf_symbols[], srsran_hip_pbch_res_t* res,
                                              srsran_hip_chest_dl_res_t* est_out, cf_t* d, float* llr_new, srsran_hip_pbch_row_t* rows, uint32_t* n_rows)
{
  const Dbg dbg = {d, llr_new, rows, n_rows};
  return run_est("srsran_hip_pbch_decode_est_dbg", cell, est, est_state_in, state, sf_symbols, res, est_out, &dbg);
}
