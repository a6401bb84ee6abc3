// pdcch_map.h -- which REs of a subframe grid the PDCCH's control region takes, in the order srsran_regs_pdcch_get reads them: srsran_regs_init_opts and
// what it calls (phch/regs.c:692-781), restated as written and with its quirks.  ONE restatement, plain C++ (no device code): srsran_hip_regs_pdcch_nregs /
// _table, the table the front-end kernel reads through (pdcch_kernels.hip) and the REs of the PCFICH and the PHICH groups (srsran_hip_regs_pcfich_table /
// _phich_ngroups / _phich_table, ctrl_host.cpp) all come from build().
//
// The rules.  The region's symbols are l = 0 .. max_ctrl - 1, max_ctrl = 4 on a cell of at most 10 PRB and 3 otherwise.  Symbol l has n[l] REGs per PRB
// (regs_num_x_symbol, :590): 2 on symbol 0, 2 on symbol 1 of a 4-port cell, 2 on symbol 3 with the extended cyclic prefix, else 3.
//   - A REG of a 3-REG symbol is four neighbouring REs; one of a 2-REG symbol is six REs less the two at vo = cell_id % 3 and vo + 3 -- on a ONE-port cell too
//     (regs_reg_init, :625: "two references in the middle").
//   - The REGs are numbered PRB by PRB; inside a PRB in three rounds over the symbols, a 2-REG symbol sitting out the middle round (:730-755).
//   - PCFICH (:492) takes four REGs of symbol 0 at k = 6 (id % (2 nof_prb)) + 6 (i nof_prb / 2), modulo the row.
//   - PHICH (:249), when phich_mi > 0: phich_mi ceilf(Ng (nof_prb / 8)) mapping units (Ng a float) of three REGs each, taken among the REGs of symbols
//     0 .. 2 that the PCFICH left, numbered per symbol; unit mi's REG i lies on symbol li = 0 (normal length), i (extended) or (mi / 2 + i + 1) % 2
//     (extended with mbsfn_or_sf1_6_tdd), at number (id n[li] / n[d] + mi + i n[li] / 3) % n[li] with d = 1 in the last case and 0 otherwise -- integer
//     arithmetic in that order.  A REG may be hit twice.
//   - PDCCH (:66-146) for the cfi: the REGs left on the symbols l < cfi (+ 1 when nof_prb <= 10), N of them, through the 32-column interleaver
//     (nrows = (N - 1) / 32 + 1, ndummy = 32 nrows - N, columns in the order PERM) and the cyclic shift by the cell id in its two forms:
//     position k of the interleaver's output reads REG (N + k - id % N) % N when k < id, else (k - id) % N.  Then N is cut to a multiple of 9.
// Grid index of RE i of a REG: k[i] + l 12 nof_prb (REG_IDX, :31).
#pragma once
#include "srsran_amd/phy_conv_abi.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace phyhip {
namespace pdcch_map {

// nullptr for a description the rules are defined on, else what is wrong with it
inline const char* invalid(const srsran_hip_pdcch_sf_t& sf)
{
  if (sf.cell_nof_prb < 6 || sf.cell_nof_prb > 110) {
    return "cell_nof_prb is not 6 .. 110";
  }
  if (sf.cell_nof_ports != 1 && sf.cell_nof_ports != 2 && sf.cell_nof_ports != 4) {
    return "cell_nof_ports is not 1, 2 or 4";
  }
  if (sf.cell_id > 503) {
    return "cell_id is above 503";
  }
  if (sf.cp_nsymb != 7 && sf.cp_nsymb != 6) {
    return "cp_nsymb is not 7 or 6";
  }
  if (sf.phich_length > 1) {
    return "phich_length is not 0 (normal) or 1 (extended)";
  }
  if (sf.phich_resources > 3) {
    return "phich_resources is above 3";
  }
  if (sf.phich_mi > 3) {
    return "phich_mi is above 3";
  }
  if (sf.mbsfn_or_sf1_6_tdd > 1) {
    return "mbsfn_or_sf1_6_tdd is not 0 or 1";
  }
  if (sf.cfi < 1 || sf.cfi > 3) {
    return "cfi is not 1 .. 3";
  }
  if (sf.sf_idx > 9) {
    return "sf_idx is above 9";
  }
  if (sf.nof_rx != 1 && sf.nof_rx != 2) {
    return "nof_rx is not 1 or 2";
  }
  return nullptr;
}

inline uint32_t nof_ctrl_symbols(const srsran_hip_pdcch_sf_t& sf) // the rows of a grid the region reads
{
  return sf.cfi + (sf.cell_nof_prb <= 10 ? 1u : 0u);
}

struct Table {
  uint32_t              nregs = 0; // a multiple of 9
  std::vector<uint32_t> re_idx;    // 4 nregs grid indices, each below nof_ctrl_symbols 12 nof_prb (checked by build)
  // the two small channels (they do not depend on the cfi): what srsran_regs_pcfich_get and srsran_regs_phich_get read, in their order
  uint32_t              pcfich[16] = {}; // on symbol 0: each below 12 nof_prb
  uint32_t              phich_units = 0; // mapping units (ngroups_phich before the doubling): phich_mi ceilf(Ng (nof_prb / 8)), 0 without PHICH
  uint32_t              phich_groups = 0; // srsran_regs_phich_ngroups: the units, twice that with the extended prefix (group g reads unit g / 2)
  uint32_t              phich_rows = 0;   // the grid rows the units reach: 1 .. 3, 0 without PHICH
  std::vector<uint32_t> phich;            // 12 grid indices per unit, each below phich_rows 12 nof_prb
};

// the fields the table depends on (sf_idx and nof_rx do not enter)
inline bool same_map(const srsran_hip_pdcch_sf_t& a, const srsran_hip_pdcch_sf_t& b)
{
  return a.cell_nof_prb == b.cell_nof_prb && a.cell_nof_ports == b.cell_nof_ports && a.cell_id == b.cell_id && a.cp_nsymb == b.cp_nsymb &&
         a.phich_length == b.phich_length && a.phich_resources == b.phich_resources && a.phich_mi == b.phich_mi &&
         a.mbsfn_or_sf1_6_tdd == b.mbsfn_or_sf1_6_tdd && a.cfi == b.cfi;
}

// `sf` has passed invalid().  false when the reference's own initialisation fails (a PCFICH REG hit twice; a PHICH so large that the region of some cfi -- not
// only this one -- keeps no REG, on which regs_pdcch_init divides by zero) or an index leaves the region's rows.
inline bool build(const srsran_hip_pdcch_sf_t& sf, Table& out)
{
  struct Reg {
    uint32_t l, k0, k[4];
    bool     assigned;
  };
  static const uint8_t PERM[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
  const uint32_t nof_prb = sf.cell_nof_prb, id = sf.cell_id, vo = id % 3, max_ctrl = nof_prb <= 10 ? 4 : 3;
  uint32_t       n[4] = {0, 0, 0, 0}, total = 0;
  for (uint32_t l = 0; l < max_ctrl; l++) {
    n[l] = l == 0 ? 2 : l == 1 ? (sf.cell_nof_ports == 4 ? 2 : 3) : l == 2 ? 3 : (sf.cp_nsymb == 7 ? 3 : 2);
    total += nof_prb * n[l];
  }
  std::vector<Reg> regs(total);
  // the ordering loop (:730-755)
  uint32_t j[4] = {0, 0, 0, 0}, k = 0, i = 0, prb = 0, jmax = 0;
  while (k < total) {
    if (n[i] == 3 || (n[i] == 2 && jmax != 1)) {
      Reg&           r    = regs[k];
      const uint32_t base = prb * 12;
      r.l        = i;
      r.assigned = false;
      if (n[i] == 2) { // regs_reg_init, maxreg 2
        r.k0       = base + j[i] * 6;
        uint32_t m = 0;
        for (uint32_t t = 0; t < vo; t++) {
          r.k[m++] = r.k0 + t;
        }
        for (uint32_t t = 0; t < 2; t++) {
          r.k[m++] = r.k0 + t + vo + 1;
        }
        const uint32_t z = m;
        for (uint32_t t = 0; t < 4 - z; t++) {
          r.k[m++] = r.k0 + vo + 3 + t + 1;
        }
      } else {
        r.k0 = base + j[i] * 4;
        for (uint32_t t = 0; t < 4; t++) {
          r.k[t] = r.k0 + t;
        }
      }
      j[i]++;
      k++;
    }
    i++;
    if (i == max_ctrl) {
      i = 0;
      jmax++;
    }
    if (jmax == 3) {
      prb++;
      j[0] = j[1] = j[2] = j[3] = 0;
      jmax = 0;
    }
  }
  // PCFICH (:492)
  const uint32_t k_hat = 6 * (id % (2 * nof_prb));
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t kk = (k_hat + (q * nof_prb / 2) * 6) % (nof_prb * 12);
    Reg*           f  = nullptr;
    for (Reg& r : regs) {
      if (r.l == 0 && r.k0 == kk) {
        f = &r;
        break;
      }
    }
    if (!f || f->assigned) {
      return false;
    }
    f->assigned = true;
    for (uint32_t t = 0; t < 4; t++) {
      out.pcfich[4 * q + t] = f->k[t]; // symbol 0
    }
  }
  out.phich_units = out.phich_groups = out.phich_rows = 0;
  out.phich.clear();
  // PHICH (:249)
  if (sf.phich_mi > 0) {
    const float    ng     = sf.phich_resources == 0 ? (float)1 / 6 : sf.phich_resources == 1 ? (float)1 / 2 : sf.phich_resources == 2 ? 1.f : 2.f;
    const uint32_t units  = sf.phich_mi * (uint32_t)(int)ceilf(ng * ((float)nof_prb / 8));
    std::vector<Reg*> per[3];
    for (Reg& r : regs) {
      if (r.l < 3 && !r.assigned) {
        per[r.l].push_back(&r);
      }
    }
    const uint32_t c[3] = {(uint32_t)per[0].size(), (uint32_t)per[1].size(), (uint32_t)per[2].size()};
    const bool     ext = sf.phich_length == 1, alt = ext && sf.mbsfn_or_sf1_6_tdd;
    for (uint32_t mi = 0; mi < units; mi++) {
      for (uint32_t q = 0; q < 3; q++) {
        const uint32_t li = !ext ? 0 : alt ? (mi / 2 + q + 1) % 2 : q;
        if (c[li] == 0 || c[alt ? 1 : 0] == 0) {
          return false;
        }
        const uint32_t ni = ((id * c[li] / c[alt ? 1 : 0]) + mi + q * c[li] / 3) % c[li];
        per[li][ni]->assigned = true;
        for (uint32_t t = 0; t < 4; t++) {
          out.phich.push_back(per[li][ni]->k[t] + li * nof_prb * 12);
        }
        out.phich_rows = li + 1 > out.phich_rows ? li + 1 : out.phich_rows;
      }
    }
    out.phich_units  = units;
    out.phich_groups = sf.cp_nsymb == 6 ? 2 * units : units;
  }
  // PDCCH (:66-146)
  const uint32_t    nctrl = nof_ctrl_symbols(sf);
  std::vector<Reg*> tmp;
  for (Reg& r : regs) {
    if (r.l < nctrl && !r.assigned) {
      tmp.push_back(&r);
    }
  }
  const uint32_t N = (uint32_t)tmp.size();
  for (uint32_t c = 1; c <= 3; c++) { // the reference lays out all three regions whatever the cfi, and divides by each one's REG count
    uint32_t left = 0;
    for (const Reg& r : regs) {
      left += (r.l < c + (nof_prb <= 10 ? 1u : 0u) && !r.assigned) ? 1u : 0u;
    }
    if (left == 0) {
      return false;
    }
  }
  std::vector<Reg*> order(N, nullptr);
  const uint32_t    nrows = (N - 1) / 32 + 1, ndummy = 32 * nrows - N;
  k                       = 0;
  for (uint32_t col = 0; col < 32; col++) {
    for (uint32_t row = 0; row < nrows; row++) {
      if (row * 32 + PERM[col] >= ndummy) {
        const uint32_t m  = row * 32 + PERM[col] - ndummy;
        const uint32_t kp = k < id ? (N + k - (id % N)) % N : (k - id) % N;
        order[m]          = tmp[kp];
        k++;
      }
    }
  }
  out.nregs = (N / 9) * 9;
  out.re_idx.resize((size_t)4 * out.nregs);
  const uint32_t limit = nctrl * 12 * nof_prb;
  for (uint32_t r = 0; r < out.nregs; r++) {
    for (uint32_t t = 0; t < 4; t++) {
      const uint32_t idx = order[r]->k[t] + order[r]->l * nof_prb * 12;
      if (idx >= limit) {
        return false;
      }
      out.re_idx[(size_t)4 * r + t] = idx;
    }
  }
  return true;
}

// the table of a description the calls take -- in range, and one the reference's own initialisation succeeds on -- built once per thread (pdcch_host.cpp);
// nullptr with *why set for any other
const Table* table_of(const srsran_hip_pdcch_sf_t* sf, const char** why);

// the grids a call on sf's planes takes -- a received grid per antenna, an estimate grid per (port, antenna): nullptr, or which one is missing
inline const char* planes_invalid(const srsran_hip_pdcch_sf_t& sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS])
{
  for (uint32_t a = 0; a < sf.nof_rx; a++) {
    if (!sf_symbols[a]) {
      return "a received grid is NULL";
    }
    for (uint32_t p = 0; p < sf.cell_nof_ports; p++) {
      if (!ce[p][a]) {
        return "an estimate grid is NULL";
      }
    }
  }
  return nullptr;
}
// the first pb bytes of each of them into planes of stride pstride from `at`, in the order the kernels index: [rx | port-major estimates]
inline void stage_planes(uint8_t* at, const srsran_hip_pdcch_sf_t& sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], size_t pb, size_t pstride)
{
  for (uint32_t a = 0; a < sf.nof_rx; a++) {
    memcpy(at + a * pstride, sf_symbols[a], pb);
    for (uint32_t p = 0; p < sf.cell_nof_ports; p++) {
      memcpy(at + (sf.nof_rx + p * sf.nof_rx + a) * pstride, ce[p][a], pb);
    }
  }
}

} // namespace pdcch_map
} // namespace phyhip
