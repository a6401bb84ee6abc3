// pbch_device.h -- what pbch_host.cpp and pbch_kernels.hip share: the cells and jobs of a PBCH call and its launch.
#pragma once
#include "hip_common.h"
#include "modem_device.h"
#include "pbch_map.h"

namespace phyhip {
namespace pbch {

constexpr uint32_t kBits   = 40;        // SRSRAN_BCH_PAYLOADCRC_LEN
constexpr uint32_t kOutRow = kBits + 8; // the 40 bits, the 16-bit remainder, the 16-bit count of payload ones, four zero bytes
constexpr uint32_t kMaxCells = 8;
constexpr uint32_t kMaxJobs  = kMaxCells * 3 * pbch_map::kMaxCombos;

struct Cell {          // offsets in points (float2) from Params::planes, in floats from Params::hist / newest, in words from Params::seq
  uint32_t o_rx;       // the received plane's RE at symbol 0 of slot 1, first of the 72 sub-carriers
  uint32_t o_ce;       // the same RE of port 0's estimate
  uint32_t ce_stride;  // from a port's estimate plane to the next port's
  uint32_t row_stride; // from a symbol to the next
  uint32_t id, cp_nsymb;
  uint32_t f;          // frame_idx behind its increment: 1 .. 4
  uint32_t last_nant;  // the last antenna hypothesis of the cell: its combination 0 stores the newest row
  float    noise;      // noise_estimate, when Params::noise_dev.v is null
  uint32_t o_hist;     // the caller's four rows of nof_bits soft bits (rows < f - 1 are read; with Job::nant 0 rows < f)
  uint32_t o_seq;      // the cell's pbch_map::kSeqWords words
  uint32_t o_new;      // where the newest row goes (kMaxBits floats)
  uint32_t first_slot; // _dbg: the cell's first (cell, hypothesis) slot of Params::dbg_d / dbg_llr
};

struct Job { // one wave
  uint8_t cell, nant, combo, slot; // nant 0: the decode stage by itself on the caller's rows; slot: the hypothesis's number in the cell's list (0 .. 2)
};

struct Params {
  const float2*   planes;
  const Cell*     cells;
  const Job*      jobs;
  const float*    hist;
  const uint32_t* seq;
  uint8_t*        rows;   // n_jobs x kOutRow
  float*          newest; // per cell
  float*          dbg_rm; // nullptr, or n_jobs x 120
  uint16_t*       dbg_sym;
  float2*         dbg_d;   // nullptr, or per slot kMaxRe points
  float*          dbg_llr; // nullptr, or per slot kMaxBits floats
  modem::NoiseAvg noise_dev; // v != nullptr: the one-port equaliser's noise estimate is get_noise() of the estimator ahead on the stream
  float           qpsk_f;
  uint32_t        n_jobs;
};
hipError_t launch(const Params& p, hipStream_t st);

} // namespace pbch
} // namespace phyhip
