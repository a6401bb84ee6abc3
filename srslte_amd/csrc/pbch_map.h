// pbch_map.h -- the PBCH rules, restated once: which REs of slot 1 srsran_pbch_get reads (phch/pbch.c:54-102 on prb_cp_ref / prb_cp, phch/prb_dl.c:46-85),
// the hypothesis list of srsran_pbch_decode (pbch.c:501-548), the CRC masks (srsran_crc_mask), the verdict of srsran_pbch_crc_check (pbch.c:378-397), the
// scrambling sequence (srsran_sequence_pbch: c_init = cell_id, 1920 or 1728 bits) and srsran_pbch_mib_unpack (pbch.c:271-312).  Host and device.
//
// The REs.  The channel lies on the first four symbols of slot 1, on the 72 sub-carriers that start at nof_prb * 12 / 2 - 36 (mid-PRB for 15 and 25 PRB).  On
// symbols 0 and 1 -- and on symbol 3 with the extended prefix -- the sub-carriers j of those 72 with j % 3 == cell_id % 3 are skipped WHATEVER the port count
// (the places of the CRS of four ports): 48 REs.  That is the index set prb_cp_ref(offset = id % 3, 4, 24) walks: `offset` REs, 23 times (skip one, take two),
// and, when offset < 2, skip one and take 2 - offset; with offset 2 the walk ends one RE short of the row, which is why pbch.c:73/75 adds 1 there.  The other
// symbols are taken whole.  Normal prefix: 48 + 48 + 72 + 72 = 240 REs; extended: 48 + 48 + 72 + 48 = 216.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PBCH_HD __host__ __device__
#else
#define PBCH_HD
#endif

namespace phyhip {
namespace pbch_map {

constexpr uint32_t kRows       = 4;   // symbols of slot 1 the channel lies on
constexpr uint32_t kCols       = 72;  // its sub-carriers
constexpr uint32_t kMaxRe      = 240; // PBCH_RE_CP_NORM
constexpr uint32_t kMaxBits    = 480; // soft bits of one frame
constexpr uint32_t kPayload    = 24;  // SRSRAN_BCH_PAYLOAD_LEN
constexpr uint32_t kCoded      = 120; // SRSRAN_BCH_ENCODED_LEN
constexpr uint32_t kMaxCombos  = 30;  // (nb, dst, src) combinations with four frames
constexpr uint32_t kSeqWords   = 60;  // 1920 chips, 32 a word

PBCH_HD inline uint32_t nof_re(uint32_t cp_nsymb)
{
  return cp_nsymb == 7 ? 240u : 216u;
}

PBCH_HD inline uint32_t first_col(uint32_t nof_prb)
{
  return nof_prb * 6 - 36;
}

PBCH_HD inline bool row_skips(uint32_t row, uint32_t cp_nsymb)
{
  return row < 2 || (cp_nsymb == 6 && row == 3);
}

// RE number i of srsran_pbch_get's output (i < nof_re) -> its symbol of slot 1 (0 .. 3) and its sub-carrier among the 72 (0 .. 71)
PBCH_HD inline void re_pos(uint32_t i, uint32_t id, uint32_t cp_nsymb, uint32_t* row, uint32_t* col)
{
  const uint32_t o = id % 3;
  uint32_t       r = 0;
  for (; r < 3; r++) {
    const uint32_t len = row_skips(r, cp_nsymb) ? 48u : 72u;
    if (i < len) {
      break;
    }
    i -= len;
  }
  *row = r;
  if (row_skips(r, cp_nsymb)) { // the two of every three that are not o, in increasing order
    const uint32_t t = i >> 1, u = i & 1u;
    *col             = 3 * t + u + (u >= o ? 1u : 0u);
  } else {
    *col = i;
  }
}

// the index of RE i in the grid of slot 1 (rows of 12 nof_prb)
PBCH_HD inline uint32_t re_index(uint32_t i, uint32_t nof_prb, uint32_t id, uint32_t cp_nsymb)
{
  uint32_t row, col;
  re_pos(i, id, cp_nsymb, &row, &col);
  return row * 12 * nof_prb + first_col(nof_prb) + col;
}

// combinations of frame_idx f (1 .. 4): for nb < f / for dst < 4 - nb / for src < f - nb.  4, 11, 20, 30.
PBCH_HD inline uint32_t nof_combos(uint32_t f)
{
  uint32_t n = 0;
  for (uint32_t nb = 0; nb < f; nb++) {
    n += (4 - nb) * (f - nb);
  }
  return n;
}

PBCH_HD inline void combo(uint32_t f, uint32_t c, uint32_t* nb, uint32_t* dst, uint32_t* src)
{
  for (uint32_t b = 0; b < f; b++) {
    const uint32_t per = f - b, n = (4 - b) * per;
    if (c < n) {
      *nb  = b;
      *dst = c / per;
      *src = c % per;
      return;
    }
    c -= n;
  }
  *nb = *dst = *src = 0;
}

// the antenna hypotheses of a cell: nof_ports 0 -> 1, 2, 4; else that one.  Returns how many.
PBCH_HD inline uint32_t nant_list(uint32_t nof_ports, uint32_t nant[3])
{
  if (nof_ports == 0) {
    nant[0] = 1, nant[1] = 2, nant[2] = 4;
    return 3;
  }
  nant[0] = nof_ports;
  return 1;
}

// srsran_crc_mask[nant - 1] as the 16-bit word the parity bits are xored with, first bit highest
PBCH_HD inline uint32_t crc_mask(uint32_t nant)
{
  return nant == 1 ? 0x0000u : nant == 2 ? 0xFFFFu : nant == 4 ? 0x5555u : 0x0000u;
}

// srsran_pbch_crc_check: rem is the 16 parity bits xor the CRC of the payload, ones the count of payload ones
PBCH_HD inline bool verdict(uint32_t rem, uint32_t ones, uint32_t nant)
{
  return rem == crc_mask(nant) && ones != 0;
}

// TS 36.211 7.2 with c_init = cell_id, packed 32 chips a word (chip k is bit k % 32 of word k / 32); kSeqWords words, every chip of them computed
inline void sequence(uint32_t cell_id, uint32_t* words)
{
  static_assert(kSeqWords * 32 == 1920, "one word per 32 chips");
  uint32_t x1 = 1, x2 = cell_id; // bit i = x(n + i), i < 31
  for (uint32_t n = 0; n < 1600 + kSeqWords * 32; n++) {
    if (n >= 1600) {
      const uint32_t k = n - 1600;
      if ((k & 31u) == 0) {
        words[k >> 5] = 0;
      }
      words[k >> 5] |= ((x1 ^ x2) & 1u) << (k & 31u);
    }
    const uint32_t n1 = ((x1 >> 3) ^ x1) & 1u, n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
    x1                = (x1 >> 1) | (n1 << 30);
    x2                = (x2 >> 1) | (n2 << 30);
  }
}

// srsran_pbch_mib_unpack on the 24 payload bits
inline void mib_unpack(const uint8_t* msg, uint32_t* nof_prb, uint32_t* phich_length, uint32_t* phich_resources, uint32_t* sfn)
{
  const uint32_t bw = (msg[0] & 1u) << 2 | (msg[1] & 1u) << 1 | (msg[2] & 1u);
  *nof_prb          = bw == 0 ? 6 : bw == 1 ? 15 : (bw - 1) * 25;
  *phich_length     = msg[3] ? 1 : 0;
  *phich_resources  = (msg[4] & 1u) << 1 | (msg[5] & 1u);
  uint32_t s        = 0;
  for (uint32_t i = 0; i < 8; i++) {
    s = (s << 1) | (msg[6 + i] & 1u);
  }
  *sfn = s << 2;
}

} // namespace pbch_map
} // namespace phyhip
