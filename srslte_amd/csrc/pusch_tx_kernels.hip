// pusch_tx_kernels.hip -- PUSCH transmit with control information (gfx950): the multiplexer / channel interleaver of TS 36.212 5.2.2.8, the scrambler, the
// placeholder / repetition fix-up and the modulator in one pass -- the transmit mirror of uci_tile (modem_kernels.hip).
//
// Reference behaviour: srsran_ulsch_encode (sch.c:1194-1337: the CQI code word in front of the transport block's bits, ulsch_interleave around the RI positions,
// the RI and ACK bits written at their positions) and what srsran_pusch_encode does with its q (pusch.c:299-334: srsran_sequence_pusch_apply_pack, the fix-up
// loop, srsran_mod_modulate_bytes).  The reference writes q, reads and writes it twice more and reads it again; here one lane per modulation symbol decides
// from (row, column) and the three counts where its Qm bits come from, scrambles them with the wave's chips and stores one constellation point.  q never
// reaches memory unless the caller asks for it.
//
// Tiling as mod_tile: one workgroup = MODEM_TILE_SYMS symbols, a quarter per wave (lane l takes l, l + 64, ...: a wave's stores are contiguous 512 B), the
// wave's <= 4096 chips made by its first lanes into LDS.  The gathers -- Qm bits of the coder's image (at most 86,400 bits: 10.8 KB), Qm bytes of the control
// image -- are byte loads from arrays that fit L2 many times over; a wave's 64 lanes read neighbouring ranks of a row or ranks `cols` apart, a few cache lines.
#include "hip_common.h"
#include "modem_arith.h"
#include "pusch_tx_device.h"

namespace phyhip {
namespace pusch_tx {

namespace {

enum { KIND_DATA = 0, KIND_RI = 1, KIND_ACK = 2 };
enum { TYPE_ONE = 1, TYPE_REPETITION = 2, TYPE_PLACEHOLDER = 3 }; // srsran_uci_bit_type_t

// what symbol s holds before scrambling: v = its Qm bits, bit k of the symbol in bit k; types = the type of bit k in bits 2 k, 2 k + 1 (0 for data); its kind
// and, for a control symbol, its number in the reference's list
template <int QM>
struct Symbol {
  uint32_t v, types, kind, num;
};

template <int QM>
__device__ __forceinline__ uint32_t typed_bits(const uint8_t* t, uint32_t& types)
{
  uint32_t v = 0;
  types      = 0;
#pragma unroll
  for (int k = 0; k < QM; k++) {
    const uint32_t ty = t[k];
    types |= ty << (2 * k);
    v |= (ty == TYPE_ONE ? 1u : 0u) << k; // sch.c:1321-1332: UCI_BIT_1 is written as 1, every other type as 0
  }
  return v;
}

template <int QM>
__device__ __forceinline__ Symbol<QM> symbol_source(const Params& p, uint32_t s)
{
  // the four columns of each kind, one per nibble (index j); the symbol number inside a row of four is {0,3,2,1}[j], the inverse of (3 n) % 4
  const uint32_t ri_cols = p.cols > 10 ? 0xA741u : 0x8530u, ack_cols = p.cols > 10 ? 0x9832u : 0x7621u, n_of_j = 0x1230u;
  const uint32_t rows = p.rows, q_ack = p.q_ack, q_ri = p.q_ri, q_cqi = p.q_cqi;
  const uint32_t col = s / rows, row = s - col * rows, b = rows - 1 - row; // b: rows below this one
  const int      m   = (int)q_ri - 4 * (int)b;                            // RI symbols of this row: those whose number in the row is < m
  int            n_ri = -1, n_ack = -1;
  uint32_t       inrow = 0; // RI symbols of this row left of this column
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t rc = (ri_cols >> (4 * j)) & 15u, ac = (ack_cols >> (4 * j)) & 15u, t = (n_of_j >> (4 * j)) & 15u;
    n_ri  = rc == col ? (int)(4 * b + t) : n_ri;
    n_ack = ac == col ? (int)(4 * b + t) : n_ack;
    inrow += (rc < col && (int)t < m) ? 1u : 0u;
  }
  Symbol<QM> y;
  if (n_ri >= 0 && (uint32_t)n_ri < q_ri) {
    y.kind = KIND_RI;
    y.num  = (uint32_t)n_ri;
    y.v    = typed_bits<QM>(p.ctl + (size_t)(q_ack + y.num) * QM, y.types);
    return y;
  }
  if (n_ack >= 0 && (uint32_t)n_ack < q_ack) { // punctures the data stream: the symbol keeps its rank, its bits are the ACK's
    y.kind = KIND_ACK;
    y.num  = (uint32_t)n_ack;
    y.v    = typed_bits<QM>(p.ctl + (size_t)y.num * QM, y.types);
    return y;
  }
  const uint32_t above = q_ri - min(q_ri, 4 * (b + 1)); // RI symbols in the rows above
  const uint32_t rank  = row * p.cols + col - above - inrow;
  y.kind = KIND_DATA;
  y.num = y.types = 0;
  if (rank < q_cqi) {
    const uint8_t* c = p.ctl + (size_t)(q_ack + q_ri + rank) * QM;
    y.v              = 0;
#pragma unroll
    for (int k = 0; k < QM; k++) {
      y.v |= (uint32_t)(c[k] & 1u) << k;
    }
  } else { // the coder's image keeps its own layout: the CQI offset is applied here
    const uint32_t e = (rank - q_cqi) * QM, by = e >> 3;
    const uint32_t hi = by < p.e_bytes ? p.e_bits[by] : 0u, lo = by + 1 < p.e_bytes ? p.e_bits[by + 1] : 0u;
    const uint32_t msb = (((hi << 8) | lo) >> (16 - QM - (e & 7u))) & ((1u << QM) - 1u); // bit 0 of the symbol = MSB
    y.v                = __brev(msb) >> (32 - QM);
  }
  return y;
}

// one chip of the sequence at an arbitrary bit (make_chips' jump to the 128-chip boundary, then the shift register up to the bit)
__device__ __forceinline__ uint32_t chip_single(const Params& p, uint32_t bit)
{
  const uint32_t  j = bit / MODEM_SEQ_CHUNK, o = bit % MODEM_SEQ_CHUNK;
  const uint32_t* col = p.x2_cols + (size_t)j * 31;
  uint32_t        s2  = 0;
  for (int i = 0; i < 31; i++) {
    s2 ^= ((p.seed >> i) & 1u) ? col[i] : 0u;
  }
  for (uint32_t k = 0; k < o / 16; k++) {
    s2 = modem::step16_x2(s2);
  }
  const uint32_t c1 = p.x1_bits[(size_t)j * (MODEM_SEQ_CHUNK / 32) + (o >> 5)] >> (o & 31u);
  return ((s2 >> (o & 15u)) ^ c1) & 1u;
}

// pusch.c:315-331 on the scrambled bits x of symbol s, bit by bit in list order: a placeholder becomes 1, a repetition at position p > 1 takes bit p - 1 as
// the loop finds it -- bit k - 1 of this symbol, already fixed, or `prev` (bit s Qm - 1) for k = 0; at p <= 1 it is left as it is
template <int QM>
__device__ __forceinline__ uint32_t fix_symbol(uint32_t x, uint32_t types, uint32_t s, uint32_t prev)
{
#pragma unroll
  for (int k = 0; k < QM; k++) {
    const uint32_t t = (types >> (2 * k)) & 3u;
    if (t == TYPE_PLACEHOLDER) {
      x |= 1u << k;
    } else if (t == TYPE_REPETITION && s * QM + k > 1) {
      const uint32_t bit = k ? (x >> (k - 1)) & 1u : prev;
      x                  = (x & ~(1u << k)) | (bit << k);
    }
  }
  return x;
}

// The value of bit s Qm - 1 -- the last bit of symbol s - 1 -- when the fix-up loop reaches a repetition type in bit 0 of control symbol s (kind, num).  The
// reference's encoders never put one there (encode_ri_ack: a repetition follows its bit inside a symbol); a caller's list may.  The loop runs over the RI
// list, then the ACK list: symbol s - 1 has been fixed before only when s is an ACK symbol and s - 1 is an RI symbol or an ACK symbol of a lower number (the
// one in the bottom row of the column to the left, reached from row 0).  Its own bit 0 then saw the unfixed last bit of the symbol before it, which is data
// or a control symbol of a higher number.
template <int QM>
__device__ __noinline__ uint32_t bit_before(const Params& p, uint32_t s, uint32_t kind, uint32_t num)
{
  const uint32_t   sy = s - 1;
  const Symbol<QM> y  = symbol_source<QM>(p, sy);
  uint32_t         x  = y.v;
  const bool       fixed = kind == KIND_ACK && (y.kind == KIND_RI || (y.kind == KIND_ACK && y.num < num));
  if (!fixed || y.types == 0) {
    return ((x >> (QM - 1)) ^ chip_single(p, sy * QM + QM - 1)) & 1u;
  }
  for (int k = 0; k < QM; k++) {
    x ^= chip_single(p, sy * QM + k) << k;
  }
  uint32_t prev = 0;
  if ((y.types & 3u) == TYPE_REPETITION && sy * QM > 1) {
    const Symbol<QM> w = symbol_source<QM>(p, sy - 1);
    prev               = ((w.v >> (QM - 1)) ^ chip_single(p, sy * QM - 1)) & 1u;
  }
  return (fix_symbol<QM>(x, y.types, sy, prev) >> (QM - 1)) & 1u;
}

template <int MOD>
__device__ __forceinline__ void mux_mod_tile(const Params& p, uint32_t tile, uint32_t* cbw)
{
  constexpr int  QM   = 2 * MOD;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = tile * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4); // first symbol of this wave
  if (w0 >= p.n) {
    return;
  }
  if (p.scramble) {
    modem::make_chips(p.x1_bits, p.x2_cols, p.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (p.n - w0) * QM), cbw);
  }
  const float2* tab = p.table + modem::mod_table_offset(MOD);
#pragma unroll
  for (int r = 0; r < (int)(MODEM_TILE_SYMS / 256); r++) {
    const uint32_t s = w0 + r * 64u + lane;
    if (s >= p.n) {
      continue;
    }
    const Symbol<QM> y = symbol_source<QM>(p, s);
    uint32_t         x = y.v;
    if (p.scramble) {
      x ^= modem::chips_at(cbw, (r * 64u + lane) * QM) & ((1u << QM) - 1u); // chip i of the symbol in bit i
      if (y.types) {
        uint32_t prev = 0;
        if ((y.types & 3u) == TYPE_REPETITION && s * QM > 1) {
          prev = bit_before<QM>(p, s, y.kind, y.num);
        }
        x = fix_symbol<QM>(x, y.types, s, prev);
      }
    }
    const uint32_t msb = __brev(x) >> (32 - QM); // bit 0 of the symbol = MSB: the table's index and the packed order
    if (p.d) {
      p.d[s] = tab[msb];
    }
    if (p.q_words) {
      const uint32_t at = s * QM, by = at >> 3, w16 = msb << (16 - QM - (at & 7u));
      atomicOr(p.q_words + (by >> 2), (w16 >> 8) << (8 * (by & 3u)));
      if ((at & 7u) + QM > 8) {
        atomicOr(p.q_words + ((by + 1) >> 2), (w16 & 0xffu) << (8 * ((by + 1) & 3u)));
      }
    }
  }
}

__global__ __launch_bounds__(256) void pusch_mux_mod_kernel(const Params p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][MODEM_TILE_BITS / 128 + 4];
  if ((threadIdx.x & 63u) == 0) {
    cb[threadIdx.x >> 6][MODEM_TILE_BITS / 128] = 0; // chips_at reads one word past the last one
  }
  __syncthreads();
  uint32_t* cbw = cb[threadIdx.x >> 6];
  switch (p.mod) {
    case 1:
      mux_mod_tile<1>(p, blockIdx.x, cbw);
      break;
    case 2:
      mux_mod_tile<2>(p, blockIdx.x, cbw);
      break;
    case 3:
      mux_mod_tile<3>(p, blockIdx.x, cbw);
      break;
    default:
      break;
  }
}

} // namespace

hipError_t launch_mux_mod(const Params& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if (p.mod < 1 || p.mod > 3 || p.rows == 0 || p.cols == 0 || p.n != p.rows * p.cols || !p.e_bits || !p.table || (!p.ctl && (p.q_ack | p.q_ri | p.q_cqi))) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(pusch_mux_mod_kernel, dim3(ceil_div(p.n, MODEM_TILE_SYMS)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

} // namespace pusch_tx
} // namespace phyhip
