// ctrl_device.h -- what ctrl_host.cpp and ctrl_kernels.hip share: the tables of the PCFICH and PHICH receivers as data, the parameter block, the rows the
// kernel leaves and the launch.
#pragma once
#include "hip_common.h"
#include "modem_device.h"
#include "pdcch_map.h"

namespace phyhip {
namespace ctrl {

constexpr uint32_t kPcfichRe = 16, kPhichRe = 12, kMaxPhich = 16;

// TS 36.212 Table 5.3.4-1 (pcfich.c:39-44 without the reserved row): the receiver correlates against 2 b - 1
constexpr uint8_t kCfiTable[3][32] = {{0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1},
                                      {1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0},
                                      {1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1}};
// TS 36.211 Table 6.9.1-2 (phich.c:40-48): w[nseq][j] as {re, im}
constexpr int8_t kPhichWNormal[8][4][2] = {{{1, 0}, {1, 0}, {1, 0}, {1, 0}},   {{1, 0}, {-1, 0}, {1, 0}, {-1, 0}}, {{1, 0}, {1, 0}, {-1, 0}, {-1, 0}},
                                           {{1, 0}, {-1, 0}, {-1, 0}, {1, 0}}, {{0, 1}, {0, 1}, {0, 1}, {0, 1}},   {{0, 1}, {0, -1}, {0, 1}, {0, -1}},
                                           {{0, 1}, {0, 1}, {0, -1}, {0, -1}}, {{0, 1}, {0, -1}, {0, -1}, {0, 1}}};
constexpr int8_t kPhichWExt[4][2][2]    = {{{1, 0}, {1, 0}}, {{1, 0}, {-1, 0}}, {{0, 1}, {0, 1}}, {{0, 1}, {0, -1}}};

struct PhichJob { // one resource: the group's REs (pdcch_map.h; each below the staged rows, checked when the table is built) and what to take of them
  uint32_t idx[kPhichRe];
  uint32_t ngroup, nseq;
};
struct PcfichRow { // what workgroup 0 leaves
  uint32_t cfi;
  float    corr;
  float    corr3[3];
  float    data_f[32];
  float    d[kPcfichRe][2]; // re, im
};
struct PhichRow { // srsran_hip_phich_res_t
  uint32_t ack_value;
  float    distance;
  float    bits[3];
  float    z[3][2]; // re, im (no 8-byte alignment: the row is 44 bytes)
};

// rx: the received grids, antenna a at rx + a * stride; ce: the estimate grids, [port][rx] at ce + (port * nof_rx + a) * stride.  Each holds at least the
// rows the indices reach.
struct Params {
  const float2*   rx;
  const float2*   ce;
  uint32_t        stride; // points
  uint32_t        ports, nof_rx;
  uint32_t        ext;   // extended cyclic prefix
  float           noise; // one port: added to the gain when above 0 (not halved)
  modem::NoiseAvg noise_dev; // v != nullptr: the estimate a kernel ahead on the stream left, instead of `noise`
  uint32_t        seed;      // c_init of both channels
  float           qpsk_f;    // (float)-M_SQRT2
  const uint32_t* x1_bits;   // modem::Params: the sequence tables
  const uint32_t* x2_cols;
  uint32_t        pcfich; // 1: workgroup 0 is the PCFICH and the PHICH resources follow; 0: resources only
  uint32_t        pcfich_idx[kPcfichRe];
  PcfichRow*      pcfich_out;
  const PhichJob* jobs; // n_phich
  uint32_t        n_phich;
  PhichRow*       phich_out;
  uint32_t        cfi3_to_2; // the TDD rule of ue_dl.c:331 for the word below: a decoded 3 becomes 2
  uint32_t*       cfi_word;  // nullptr, or one word of device memory for the kernels behind on the stream: the CFI after that rule
};
hipError_t launch(const Params& p, hipStream_t st);

// host side: nullptr, or why the n resources are refused on the description of table t
inline const char* phich_invalid(const pdcch_map::Table& t, const srsran_hip_pdcch_sf_t& sf, uint32_t n, const srsran_hip_phich_resource_t* r)
{
  if (n > kMaxPhich) {
    return "more than 16 resources";
  }
  for (uint32_t i = 0; i < n; i++) {
    if (r[i].ngroup >= t.phich_groups) {
      return "ngroup is not below the number of PHICH groups";
    }
    if (r[i].nseq >= (sf.cp_nsymb == 6 ? 4u : 8u)) {
      return "nseq is not below 8 (4 with the extended cyclic prefix)";
    }
  }
  return nullptr;
}
// the jobs of n resources that have passed phich_invalid (group g reads mapping unit g / 2 with the extended prefix)
inline void phich_jobs(PhichJob* jobs, const pdcch_map::Table& t, const srsran_hip_pdcch_sf_t& sf, uint32_t n, const srsran_hip_phich_resource_t* r)
{
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t unit = sf.cp_nsymb == 6 ? r[i].ngroup / 2 : r[i].ngroup;
    memcpy(jobs[i].idx, &t.phich[(size_t)kPhichRe * unit], sizeof(jobs[i].idx));
    jobs[i].ngroup = r[i].ngroup;
    jobs[i].nseq   = r[i].nseq;
  }
}
// c_init of both channels' sequences (sequences.c:38-49)
inline uint32_t c_init(const srsran_hip_pdcch_sf_t& sf)
{
  return (sf.sf_idx + 1) * (2 * sf.cell_id + 1) * 512 + sf.cell_id;
}

} // namespace ctrl
} // namespace phyhip
