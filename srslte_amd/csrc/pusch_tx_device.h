// pusch_tx_device.h -- parameter block and launcher of pusch_tx_kernels.hip: the PUSCH transmit multiplexer (TS 36.212 5.2.2.8) fused with the scrambler, the
// placeholder / repetition fix-up of pusch.c:315-331 and the modulator
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace phyhip {
namespace pusch_tx {

// The grant's H' = n modulation symbols are a matrix of `cols` SC-FDMA symbols x `rows` sub-carriers; symbol s = col rows + row holds bits s Qm .. s Qm + Qm - 1
// of the reference's q.  RI symbol n sits in row rows - 1 - n / 4, column {1,4,7,10}[(3 n) % 4] (cols > 10) or {0,3,5,8}; ACK symbol n in the same row, column
// {2,3,8,9} or {1,2,6,7} (uci.c:364-416).  Every symbol that is not an RI symbol has a rank in the data stream g, row by row (ulsch_interleave, sch.c:932-990);
// an ACK symbol keeps its rank and its bits replace the data's.  Rank < q_cqi: the CQI code word; behind it the coder's e bits, from bit (rank - q_cqi) Qm.
struct Params {
  const uint8_t*  e_bits;  // the coder's image: (n - q_ri - q_cqi) Qm bits, byte packed, MSB first (device memory)
  uint32_t        e_bytes; // bytes of it that may be read
  const uint8_t*  ctl;     // control image, device-readable: [ACK types q_ack Qm | RI types q_ri Qm | CQI bits q_cqi Qm], one byte per bit
  float2*         d;       // n constellation points in the order the transform reads (point s), or nullptr
  uint32_t*       q_words; // or nullptr: the packed bits of q are ORed into this ZEROED array (whole 32-bit words, MSB first inside every byte)
  const float2*   table;   // constellation tables of all modulations (modem::mod_table_offset)
  uint32_t        mod;     // QPSK, 16-QAM, 64-QAM
  uint32_t        n, rows, cols;
  uint32_t        q_ack, q_ri, q_cqi;
  uint32_t        seed;     // c_init
  uint32_t        scramble; // 1: scrambled bits with the fix-up (what pusch.c modulates); 0: srsran_ulsch_encode's bits -- types 2 and 3 written as 0
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
};
inline uint32_t ctl_bytes(uint32_t q_ack, uint32_t q_ri, uint32_t q_cqi, uint32_t Qm)
{
  return (q_ack + q_ri + q_cqi) * Qm;
}
hipError_t launch_mux_mod(const Params& p, hipStream_t stream);

} // namespace pusch_tx
} // namespace phyhip
