// pdsch_map.h -- which REs of a subframe grid a PDSCH grant takes, in the order srsran_pdsch_get leaves them (srsran_pdsch_cp, pdsch.c:136-220, with
// pdsch_cp_skip_symbol :83-114, pdsch_cp_crs_offset :116-134 and prb_cp_ref / prb_cp / prb_cp_half of prb_dl.c).  ONE restatement, plain C++ (no device
// code): srsran_hip_pdsch_nof_re, the checks of the _sf grant calls and the de-mapping kernel's segment table (pdsch_map_kernels.hip) all walk for_each_prb.
//
// The rules.  Slot s takes its symbols l = (s == 0 ? lstart : 0) .. nof_symb_slot[s] - 1; symbol l of slot s is row l + s * nof_symb_slot[0] of the grid.
// In such a row every allocated PRB n (prb_idx[s][n]) gives its 12 REs but
//   - the cell-specific reference signals: on the symbols that carry them (l == 0, l == cp_nsymb - 3, and l == 1 on 4 ports) the REs k with
//     k % 6 == (l == 0 ? id % 6 : (id + 3) % 6) on one port, k % 3 == id % 3 on 2 and 4 ports;
//   - the synchronisation signals and the PBCH: in the centre PRBs (nof_prb / 2 - 3 <= n < nof_prb / 2 + 3 + nof_prb % 2) of
//       FDD  slot 0 of subframes 0 and 5, the slot's last two symbols            (PSS / SSS)
//       TDD  slot 1 of subframes 0 and 5, the slot's last symbol                 (SSS)
//       TDD  slot 0 of subframes 1 and 6, symbol 2                               (PSS)
//       both slot 1 of subframe 0, symbols 0 .. 3                                (PBCH)
//     nothing is taken -- except on a cell with an odd PRB count, where those signals cover only half of the first and of the last of the seven centre PRBs:
//     PRB nof_prb / 2 - 3 gives its lower six REs, PRB nof_prb / 2 + 3 its upper six (less the reference signals, as everywhere).
// "The slot's last symbols" are counted from grant->nof_symb_slot[s], as the reference does.
#pragma once
#include "srsran_amd/phy_chan_abi.h"

#include <cstdint>

namespace phyhip {
namespace pdsch_map {

// one allocated PRB of one grid row: where its 12 REs start in the grid (points), where its taken REs go in the plane, which of the 12 are taken
struct Seg {
  uint32_t grid_off;
  uint32_t out_off;
  uint32_t mask;
  uint32_t reserved;
};

// nullptr for a description the rules are defined on, else what is wrong with it
inline const char* invalid(const srsran_hip_pdsch_sf_t& sf)
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
  if (sf.frame_type > 1) {
    return "frame_type is not 0 (FDD) or 1 (TDD)";
  }
  if (sf.sf_idx > 9) {
    return "sf_idx is above 9";
  }
  if (sf.nof_symb_slot[0] > sf.cp_nsymb || sf.nof_symb_slot[1] > sf.cp_nsymb) {
    return "nof_symb_slot is above cp_nsymb";
  }
  if (sf.lstart >= sf.nof_symb_slot[0]) {
    return "lstart leaves no symbol in slot 0";
  }
  if (sf.csi_enable > 1) {
    return "csi_enable is not 0 or 1";
  }
  bool any = false;
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t n = 0; n < 110; n++) {
      if (sf.prb_idx[s][n] > 1) {
        return "a prb_idx byte is above 1";
      }
      any = any || (n < sf.cell_nof_prb && sf.prb_idx[s][n] && (s == 0 || sf.nof_symb_slot[1] > 0));
    }
  }
  return any ? nullptr : "the allocation is empty";
}

// the REs of a PRB that do not carry a reference signal on symbol l of a slot
inline uint32_t crs_free(const srsran_hip_pdsch_sf_t& sf, uint32_t l)
{
  const bool has_crs = (l == 1 && sf.cell_nof_ports == 4) || l == 0 || l == sf.cp_nsymb - 3;
  if (!has_crs) {
    return 0xfffu;
  }
  if (sf.cell_nof_ports == 1) {
    return 0xfffu & ~(0x041u << (l == 0 ? sf.cell_id % 6 : (sf.cell_id + 3) % 6));
  }
  return 0xfffu & ~(0x249u << (sf.cell_id % 3));
}

// PRB n on symbol l of slot s lies under PSS / SSS / PBCH
inline bool under_sync(const srsran_hip_pdsch_sf_t& sf, uint32_t s, uint32_t l, uint32_t n)
{
  const uint32_t half = sf.cell_nof_prb / 2;
  if (n < half - 3 || n >= half + 3 + sf.cell_nof_prb % 2) {
    return false;
  }
  if (sf.frame_type == 0) {
    if (s == 0 && (sf.sf_idx == 0 || sf.sf_idx == 5) && l >= sf.nof_symb_slot[s] - 2u) { // (unsigned, as there: a slot of one symbol has no such symbols)
      return true;
    }
  } else {
    if (s == 1 && (sf.sf_idx == 0 || sf.sf_idx == 5) && l >= sf.nof_symb_slot[s] - 1u) {
      return true;
    }
    if (s == 0 && (sf.sf_idx == 1 || sf.sf_idx == 6) && l == 2) {
      return true;
    }
  }
  return s == 1 && sf.sf_idx == 0 && l < 4;
}

// fn(row of the grid, PRB, 12-bit mask of the REs taken) for every allocated PRB that gives at least one RE, in the order of srsran_pdsch_get.
// `sf` has passed invalid().
template <class Fn>
inline void for_each_prb(const srsran_hip_pdsch_sf_t& sf, Fn fn)
{
  const uint32_t half = sf.cell_nof_prb / 2;
  const bool     odd  = sf.cell_nof_prb % 2 != 0;
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t l = s == 0 ? sf.lstart : 0; l < sf.nof_symb_slot[s]; l++) {
      const uint32_t keep = crs_free(sf, l);
      for (uint32_t n = 0; n < sf.cell_nof_prb; n++) {
        if (!sf.prb_idx[s][n]) {
          continue;
        }
        uint32_t mask = keep;
        if (under_sync(sf, s, l, n)) {
          mask = !odd ? 0u : n == half - 3 ? keep & 0x03fu : n == half + 3 ? keep & 0xfc0u : 0u;
        }
        if (mask) {
          fn(l + s * sf.nof_symb_slot[0], n, mask);
        }
      }
    }
  }
}

inline uint32_t nof_re(const srsran_hip_pdsch_sf_t& sf)
{
  uint32_t n = 0;
  for_each_prb(sf, [&](uint32_t, uint32_t, uint32_t mask) { n += (uint32_t)__builtin_popcount(mask); });
  return n;
}

// What the host stages of a grid and the table over it.  Rows row0 .. row0 + rows - 1 of the grid are used (symbol lstart to the grant's last symbol), and of
// each row the PRBs prb0 .. prb0 + prbs - 1 (the lowest to the highest allocated one in either slot): the staged image of a plane is rows x 12 prbs points,
// and Seg::grid_off counts in it.
struct Window {
  uint32_t row0, rows, prb0, prbs;
  uint32_t n_seg, nof_re;
  uint32_t staged_points() const { return rows * prbs * 12; }
};
constexpr uint32_t MAX_SEG = 14 * 110;

inline Window window(const srsran_hip_pdsch_sf_t& sf)
{
  uint32_t lo = sf.cell_nof_prb, hi = 0, last = 0;
  Window   w = {sf.lstart, 0, 0, 0, 0, 0};
  for_each_prb(sf, [&](uint32_t row, uint32_t n, uint32_t mask) {
    lo   = n < lo ? n : lo;
    hi   = n > hi ? n : hi;
    last = row;
    w.n_seg++;
    w.nof_re += (uint32_t)__builtin_popcount(mask);
  });
  if (w.n_seg) {
    w.rows = last - w.row0 + 1;
    w.prb0 = lo;
    w.prbs = hi - lo + 1;
  }
  return w;
}

// the table (w.n_seg entries, at most MAX_SEG) over the staged image of window w
inline void fill_table(const srsran_hip_pdsch_sf_t& sf, const Window& w, Seg* tab)
{
  uint32_t i = 0, out = 0;
  for_each_prb(sf, [&](uint32_t row, uint32_t n, uint32_t mask) {
    tab[i++] = {((row - w.row0) * w.prbs + (n - w.prb0)) * 12, out, mask, 0};
    out += (uint32_t)__builtin_popcount(mask);
  });
}

} // namespace pdsch_map
} // namespace phyhip
