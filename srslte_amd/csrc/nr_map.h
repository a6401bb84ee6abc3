// nr_map.h -- which REs of an NR slot grid a shared-channel grant takes and where its DMRS lie: the one restatement, plain C++ (no device code), of
//   srsran_dmrs_sch_get_symbols_idx           dmrs_sch.c:262-435   mapping type A, single and double length (38.211 tables 7.4.1.1.2-3 / -4); type B refused
//   srsran_dmrs_sch_rvd_re_pattern            dmrs_sch.c:437-487   the subcarriers the DMRS CDM groups without data reserve on the DMRS symbols
//   srsran_re_pattern_{,list_}to_symbol_mask  re_pattern.c:60-109  the caller's reserved patterns (at most SRSRAN_RE_PATTERN_LIST_SIZE = 4)
//   srsran_pdsch_nr_cp                        pdsch_nr.c:225-270   (= pusch_nr_cp, pusch_nr.c:274-318) symbols S .. S + L - 1, carrier PRBs in ascending order
//                                                                  where prb_idx[] is set, the 12 subcarriers minus the mask
//   srsran_dmrs_sch_seed                      dmrs_sch.c:511-532   c_init of a DMRS symbol
//   srsran_dmrs_sch_get_symbol                dmrs_sch.c:677-761   the sequence advances prb_skip * nof_pilots_x_prb * 2 bits over unused PRBs and two bits per
//                                                                  pilot over used ones: pilot j of carrier PRB p reads bits 2 (p nof_pilots_x_prb + j), + 1
//   srsran_dmrs_get_pilots_type1 / _type2     dmrs_sch.c:71-101    at delta = 0: pilot j of PRB p is subcarrier 2 j (type 1), 6 (j / 2) + j % 2 (type 2)
//   srsran_symbol_distance_s                  phy_common_nr.c:164-188, as written ((N << numerology) * SRSRAN_LTE_TS)
// srsran_hip_nr_sch_nof_re, the checks of the grid calls, the de-mapping table and the estimator's job (nr_chest_device.h) all come from here.
#pragma once
#include "srsran_amd/phy_nr_chan_abi.h"

#include <cmath>
#include <cstdint>

namespace phyhip {
namespace nr_map {

constexpr uint32_t MAX_PRB      = SRSRAN_HIP_NR_MAX_PRB;
constexpr uint32_t MAX_DMRS_SYM = 4;            // SRSRAN_DMRS_SCH_MAX_SYMBOLS
constexpr uint32_t NSYMB        = 14;           // SRSRAN_NSYMB_PER_SLOT_NR
constexpr uint32_t MAX_PILOTS   = 6 * MAX_PRB;  // per DMRS symbol (type 1)
constexpr uint32_t MAX_SEG      = NSYMB * MAX_PRB;

// dmrs_sch.c:262-435.  The count of DMRS symbols, or -1 where the reference returns an error.
inline int dmrs_symbols(const srsran_hip_nr_grid_t& g, uint32_t sym[MAX_DMRS_SYM])
{
  if (g.mapping != 0) {
    return -1; // :429-431
  }
  const uint32_t ld = g.S + g.L, ap = g.additional_pos;
  if (g.typeA_pos != 2 && ap == 3) {
    return -1; // :411-415
  }
  if ((ld == 3 || ld == 4) && g.typeA_pos != 2) {
    return -1; // :419-423
  }
  const uint32_t l0 = g.typeA_pos == 3 ? 3 : 2;
  int            n  = 0;
  if (g.length == 1) { // :262-349 (l1 = 11)
    if (ld < 3) {
      return -1;
    }
    sym[n++] = l0;
    if (ld < 8 || ap == 0) {
      return n;
    }
    if (ld < 10) {
      sym[n++] = 7;
    } else if (ld < 12) {
      if (ap == 1 || ap == 3) { // as written, :298: "additional_pos > srsran_dmrs_sch_add_pos_2" compares enumerators declared in the order 2, 0, 1, 3
        sym[n++] = 6;
      }
      sym[n++] = 9;
    } else if (ld == 12) {
      if (ap == 1) {
        sym[n++] = 9;
      } else if (ap == 2) {
        sym[n++] = 6, sym[n++] = 9;
      } else {
        sym[n++] = 5, sym[n++] = 8, sym[n++] = 11;
      }
    } else {
      if (ap == 1) {
        sym[n++] = 11;
      } else if (ap == 2) {
        sym[n++] = 7, sym[n++] = 11;
      } else {
        sym[n++] = 5, sym[n++] = 8, sym[n++] = 11;
      }
    }
    return n;
  }
  // :352-393
  if (ld < 4 || ap == 3) {
    return -1;
  }
  sym[n++] = l0, sym[n++] = l0 + 1;
  if (ld < 10 || ap == 0) {
    return n;
  }
  const uint32_t l = ld < 13 ? 8 : 10;
  sym[n++] = l, sym[n++] = l + 1;
  return n;
}

// nullptr for a description the rules are defined on, else what is wrong with it
inline const char* invalid(const srsran_hip_nr_grid_t& g)
{
  if (g.nof_prb == 0 || g.nof_prb > MAX_PRB) {
    return "nof_prb is not 1 .. 275";
  }
  if (g.scs > 4) {
    return "scs is above 4";
  }
  if (g.mapping != 0) {
    return "mapping type B is not supported";
  }
  if (g.dmrs_type > 1 || (g.typeA_pos != 2 && g.typeA_pos != 3) || g.additional_pos > 3 || (g.length != 1 && g.length != 2) || g.n_scid > 1) {
    return "dmrs_type, typeA_pos, additional_pos, length or n_scid out of range";
  }
  if (g.L == 0 || g.S + g.L > NSYMB || g.S >= NSYMB) {
    return "S + L is above 14, or L is 0";
  }
  if (g.typeA_pos != 2 && g.additional_pos == 3) {
    return "additional_pos 3 needs typeA_pos 2";
  }
  if ((g.S + g.L == 3 || g.S + g.L == 4) && g.typeA_pos != 2) {
    return "S + L of 3 or 4 needs typeA_pos 2";
  }
  uint32_t sym[MAX_DMRS_SYM];
  if (dmrs_symbols(g, sym) <= 0) {
    return "no DMRS symbols for this duration, length and additional_pos";
  }
  if (g.nof_dmrs_cdm_groups_without_data < 1 || g.nof_dmrs_cdm_groups_without_data > 3) {
    return "nof_dmrs_cdm_groups_without_data is not 1 .. 3";
  }
  if (g.nof_rvd > SRSRAN_HIP_NR_MAX_RVD_PATTERNS) {
    return "more than 4 reserved patterns";
  }
  for (uint32_t i = 0; i < g.nof_rvd; i++) {
    if (g.rvd[i].rb_end > MAX_PRB || g.rvd[i].rb_stride == 0) {
      return "a reserved pattern has rb_end above 275 or rb_stride 0";
    }
  }
  bool any = false;
  for (uint32_t n = 0; n < g.nof_prb; n++) {
    if (g.prb_idx[n] > 1) {
      return "a prb_idx byte is above 1";
    }
    any = any || g.prb_idx[n];
  }
  return any ? nullptr : "no PRB is set";
}

inline uint32_t pilots_x_prb(const srsran_hip_nr_grid_t& g) { return g.dmrs_type == 0 ? 6u : 4u; }
inline uint32_t dmrs_stride(const srsran_hip_nr_grid_t& g) { return g.dmrs_type == 0 ? 2u : 3u; }

// dmrs_sch.c:454-470: the 12-bit subcarrier mask of the DMRS pattern
inline uint32_t dmrs_sc_mask(const srsran_hip_nr_grid_t& g)
{
  uint32_t m = 0;
  for (uint32_t n = 0; n < (g.dmrs_type == 0 ? 3u : 2u); n++) {
    for (uint32_t kp = 0; kp < 2; kp++) {
      for (uint32_t d = 0; d < g.nof_dmrs_cdm_groups_without_data; d++) {
        m |= 1u << ((g.dmrs_type == 0 ? 4 * n + 2 * kp + d : 6 * n + kp + 2 * d) % 12);
      }
    }
  }
  return m;
}

// the 14-bit mask of the DMRS symbols (`g` has passed invalid())
inline uint32_t dmrs_symbol_mask(const srsran_hip_nr_grid_t& g)
{
  uint32_t  sym[MAX_DMRS_SYM], m = 0;
  const int n = dmrs_symbols(g, sym);
  for (int i = 0; i < n; i++) {
    m |= 1u << (sym[i] % NSYMB);
  }
  return m;
}

// re_pattern.c:60-109: the subcarriers of PRB rb the caller's patterns reserve on symbol l
inline uint32_t rvd_sc_mask(const srsran_hip_nr_grid_t& g, uint32_t l, uint32_t rb)
{
  uint32_t m = 0;
  for (uint32_t i = 0; i < g.nof_rvd; i++) {
    const srsran_hip_nr_re_pattern_t& p = g.rvd[i];
    if (((p.symbol >> l) & 1u) && rb >= p.rb_begin && rb < p.rb_end && (rb - p.rb_begin) % p.rb_stride == 0) {
      m |= p.sc & 0xfffu;
    }
  }
  return m;
}

// fn(symbol l, carrier PRB, ordinal of the PRB among the granted ones, 12-bit mask of the REs taken) for every granted PRB that gives at least one RE, in
// the order of srsran_pdsch_nr_cp.  `g` has passed invalid().
template <class Fn>
inline void for_each_prb(const srsran_hip_nr_grid_t& g, Fn fn)
{
  const uint32_t dsc = dmrs_sc_mask(g), dsym = dmrs_symbol_mask(g);
  for (uint32_t l = g.S; l < g.S + g.L; l++) {
    const uint32_t dm = ((dsym >> l) & 1u) ? dsc : 0u;
    uint32_t       ord = 0;
    for (uint32_t rb = 0; rb < g.nof_prb; rb++) {
      if (!g.prb_idx[rb]) {
        continue;
      }
      const uint32_t mask = 0xfffu & ~(dm | rvd_sc_mask(g, l, rb));
      if (mask) {
        fn(l, rb, ord, mask);
      }
      ord++;
    }
  }
}

inline uint32_t nof_re(const srsran_hip_nr_grid_t& g)
{
  uint32_t n = 0;
  for_each_prb(g, [&](uint32_t, uint32_t, uint32_t, uint32_t mask) { n += (uint32_t)__builtin_popcount(mask); });
  return n;
}

inline uint32_t granted_prbs(const srsran_hip_nr_grid_t& g)
{
  uint32_t n = 0;
  for (uint32_t rb = 0; rb < g.nof_prb; rb++) {
    n += g.prb_idx[rb] ? 1u : 0u;
  }
  return n;
}

// one granted PRB of one symbol: where its 12 REs start in the grid (points), where its taken REs go in the codeword, which of the 12 are taken, and
// where its 12 estimates start in the interpolated row (12 x ordinal) with the symbol in the upper half
struct Seg {
  uint32_t grid_off;
  uint32_t out_off;
  uint32_t mask;
  uint32_t ce_sym; // ce offset | symbol << 16
};

// the table (at most MAX_SEG entries); returns the count of entries
inline uint32_t fill_table(const srsran_hip_nr_grid_t& g, Seg* tab)
{
  uint32_t i = 0, out = 0;
  for_each_prb(g, [&](uint32_t l, uint32_t rb, uint32_t ord, uint32_t mask) {
    tab[i++] = {(l * g.nof_prb + rb) * 12, out, mask, (ord * 12) | (l << 16)};
    out += (uint32_t)__builtin_popcount(mask);
  });
  return i;
}
inline uint32_t nof_seg(const srsran_hip_nr_grid_t& g)
{
  uint32_t n = 0;
  for_each_prb(g, [&](uint32_t, uint32_t, uint32_t, uint32_t) { n++; });
  return n;
}

// dmrs_sch.c:530-531
inline uint32_t dmrs_seed(const srsran_hip_nr_grid_t& g, uint32_t l)
{
  const uint64_t n_id = g.n_id, n_scid = g.n_scid ? 1 : 0;
  return (uint32_t)(((((uint64_t)NSYMB * g.slot_idx + l + 1) * (2 * n_id + 1)) << 17) + (2 * n_id + n_scid)) & 0x7fffffffu;
}

// phy_common_nr.c:164-188
inline float symbol_distance_s(uint32_t l0, uint32_t l1, uint32_t numerology)
{
  if (l0 >= l1) {
    return 0.0f;
  }
  const uint32_t count = l1 - l0, cp_boundary = 7u << numerology;
  const uint32_t extra = (l0 < cp_boundary && l1 >= cp_boundary) ? 16u : 0u;
  const uint32_t N     = (2048 + 144) * count + extra;
  return (float)(N << numerology) * (1.0f / (15000.0f * 2048.0f));
}

// srsran_chest_set_smooth_filter_gauss(filter, 4, 2) (chest_common.c:70-95; dmrs_sch.c:604)
inline void smooth_filter(float f[5])
{
  float norm = 0.f;
  for (int i = 0; i < 5; i++) {
    f[i] = expf(-powf((float)(i - 2), 2) / (2.0f * powf(2.f, 2)));
    norm += f[i];
  }
  for (int i = 0; i < 5; i++) {
    f[i] *= 1.0f / norm;
  }
}

} // namespace nr_map
} // namespace phyhip
