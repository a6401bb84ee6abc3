// lte_prach_tables.h -- the small PRACH tables of TS 36.211 section 5.7 (preamble formats 0 .. 3), written out from the standard's values:
//
//   kPrachTcp / kPrachTseq : Table 5.7.1-1, in units of T_s
//   kPrachNcsUnrestricted / kPrachNcsRestricted : Table 5.7.2-2
//
// Table 5.7.2-4, the order of the 838 physical roots by logical index, is NOT in the library: no copy of the standard was at hand when this was written,
// and the table cannot be derived.  The application hands it in once (srsran_hip_prach_set_root_order, phy_prach_abi.h); an srsRAN build has it as
// prach_zc_roots[838].  The tests take it from the record of the reference's run (tests/golden/prach_ref.npz: root_order).
#pragma once
#include <cstdint>

namespace phyhip {
namespace prach {

constexpr uint32_t kPrachTcp[4]  = {3168, 21024, 6240, 21024};
constexpr uint32_t kPrachTseq[4] = {24576, 24576, 2 * 24576, 2 * 24576};
constexpr uint32_t kPrachNcsUnrestricted[16] = {0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419};
constexpr uint32_t kPrachNcsRestricted[15]   = {15, 18, 22, 26, 32, 38, 46, 55, 68, 82, 100, 128, 158, 202, 237};

} // namespace prach
} // namespace phyhip
