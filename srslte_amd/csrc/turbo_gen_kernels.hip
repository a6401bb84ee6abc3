// turbo_gen_kernels.hip -- the scalar LTE turbo decoder (turbodecoder_gen.c) for gfx950: what srsran_tdec_run_all() dispatches to where no
// window decoder takes the block size (turbo_kernels.hip has the window decoders).
#include "hip_common.h"
#include "turbo_arith.h"
#include "turbo_device.h"

namespace phyhip {
namespace turbo {

__device__ __forceinline__ short wrap16(int v)
{
  return (short)v;
}

// ------------------------------------------------------------------------------------------------
// Scalar decoder (turbodecoder_gen.c): one lane per code block, wrapping int16, beta kept in HBM.
// Used for K <= 400 (AUTO) or SRSRAN_TDEC_GENERIC.  Vectors are stored lane-interleaved
// [index][64 lanes] so that a wave's accesses coalesce.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gen_acs_beta(short (&old)[8], short x, short y)
{
  short xy = wrap16(x + y);
  short m_b[8], nw[8];
  m_b[0] = wrap16(old[4] + xy);
  m_b[1] = old[4];
  m_b[2] = wrap16(old[5] + y);
  m_b[3] = wrap16(old[5] + x);
  m_b[4] = wrap16(old[6] + x);
  m_b[5] = wrap16(old[6] + y);
  m_b[6] = old[7];
  m_b[7] = wrap16(old[7] + xy);
  nw[0] = old[0];
  nw[1] = wrap16(old[0] + xy);
  nw[2] = wrap16(old[1] + x);
  nw[3] = wrap16(old[1] + y);
  nw[4] = wrap16(old[2] + y);
  nw[5] = wrap16(old[2] + x);
  nw[6] = wrap16(old[3] + xy);
  nw[7] = old[3];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    old[i] = m_b[i] > nw[i] ? m_b[i] : nw[i];
  }
}

__global__ __launch_bounds__(64) void tdec_gen_kernel(const GenParams p)
{
  const int lane = threadIdx.x;
  const int cb   = blockIdx.x * 64 + lane;
  if (cb >= p.n_cb) {
    return;
  }
  const uint32_t K  = p.K;
  const uint32_t L  = K + 4; // K + 3 tail (+1 for the beta terminal state)
  // per-wave slab, element (array, index, lane): ((array_base + index) * 64 + lane)
  short* ws = p.ws + (size_t)blockIdx.x * p.ws_stride;
#define GV(base, idx) ws[((size_t)(base) + (idx)) * 64 + lane]
  const uint32_t oS = 0, oP0 = L, oP1 = 2 * L, oA1 = 3 * L, oA2 = 4 * L, oE1 = 5 * L, oE2 = 6 * L, oB = 7 * L;
  // beta: 8 * (K+4) from oB

  if (p.n_begin == 0) {
    // int8 input: the 8-bit API widens to int16 when no 8-bit decoder takes this K (turbodecoder.c:455-478)
    const size_t       in_off = p.desc ? (size_t)p.desc[cb].in_off : (size_t)cb * p.in_stride;
    const short*       in16 = p.input + in_off;
    const signed char* in8  = reinterpret_cast<const signed char*>(p.input) + in_off;
    auto               in   = [&](uint32_t i) -> short { return p.in_is8 ? (short)in8[i] : in16[i]; };
    for (uint32_t i = 0; i < K; i++) { // turbodecoder_gen.c:238-258
      GV(oS, i)  = in(3 * i);
      GV(oP0, i) = in(3 * i + 1);
      GV(oP1, i) = in(3 * i + 2);
    }
    for (uint32_t i = K; i < K + 3; i++) {
      GV(oS, i)  = in(3 * K + 2 * (i - K));
      GV(oP0, i) = in(3 * K + 2 * (i - K) + 1);
      GV(oA2, i) = in(3 * K + 6 + 2 * (i - K));
      GV(oP1, i) = in(3 * K + 6 + 2 * (i - K) + 1);
    }
  }
  const uint16_t* inter   = p.inter;
  const uint16_t* deinter = p.deinter;
  uint32_t        n_run    = p.n_end; // half iterations completed when the loop is left
  bool            crc_good = false;

  for (uint32_t n = p.n_begin; n < p.n_end; n++) {
    const bool     dec1    = !(n & 1);
    const bool     has_app = dec1 && n > 0;
    const uint32_t oX = dec1 ? oS : oA2, oY = dec1 ? oP0 : oP1, oOut = dec1 ? oE1 : oE2;
    if (dec1) {
      if (n) {
        for (uint32_t i = 0; i < K; i++) {
          GV(oA1, i) = wrap16(GV(oA1, i) - GV(oE1, i));
        }
      }
    } else {
      for (uint32_t i = 0; i < K; i++) {
        short e = GV(oE1, i);
        if (n > 1) {
          e          = wrap16(e - GV(oA1, i));
          GV(oE1, i) = e;
        }
        GV(oA2, deinter[i]) = e;
      }
    }
    // map_gen_beta (turbodecoder_gen.c:58-112)
    short old[8];
    old[0] = 0;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      old[i] = -TD_INF;
    }
    const uint32_t end = K + 3;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      GV(oB + 8 * end, i) = old[i];
    }
    for (int k = (int)end - 1; k >= 0; k--) {
      short x = GV(oX, k);
      if (has_app && (uint32_t)k < K) {
        x = wrap16(x + GV(oA1, k));
      }
      short y = GV(oY, k);
      gen_acs_beta(old, x, y);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        GV(oB + 8 * k, i) = old[i];
      }
      if ((k % 4) == 0 && (uint32_t)k < K) {
#pragma unroll
        for (int i = 1; i < 8; i++) {
          old[i] = wrap16(old[i] - old[0]);
        }
        old[0] = 0;
      }
    }
    // map_gen_alpha (turbodecoder_gen.c:114-198)
    old[0] = 0;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      old[i] = -TD_INF;
    }
    for (uint32_t k = 1; k < K + 1; k++) {
      short x = GV(oX, k - 1);
      if (has_app) {
        x = wrap16(x + GV(oA1, k - 1));
      }
      short y  = GV(oY, k - 1);
      short xy = wrap16(x + y);
      short m_b[8], nw[8];
      m_b[0] = old[0];
      m_b[1] = wrap16(old[3] + y);
      m_b[2] = wrap16(old[4] + y);
      m_b[3] = old[7];
      m_b[4] = old[1];
      m_b[5] = wrap16(old[2] + y);
      m_b[6] = wrap16(old[5] + y);
      m_b[7] = old[6];
      nw[0] = wrap16(old[1] + xy);
      nw[1] = wrap16(old[2] + x);
      nw[2] = wrap16(old[5] + x);
      nw[3] = wrap16(old[6] + xy);
      nw[4] = wrap16(old[0] + xy);
      nw[5] = wrap16(old[3] + x);
      nw[6] = wrap16(old[4] + x);
      nw[7] = wrap16(old[7] + xy);
      short m1 = 0, m0 = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        short bq = GV(oB + 8 * k, i);
        short v0 = wrap16(m_b[i] + bq);
        short v1 = wrap16(nw[i] + bq);
        m0 = (i == 0) ? v0 : (v0 > m0 ? v0 : m0);
        m1 = (i == 0) ? v1 : (v1 > m1 ? v1 : m1);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        old[i] = m_b[i] > nw[i] ? m_b[i] : nw[i];
      }
      if ((k % 4) == 0) {
#pragma unroll
        for (int i = 1; i < 8; i++) {
          old[i] = wrap16(old[i] - old[0]);
        }
        old[0] = 0;
      }
      GV(oOut, k - 1) = wrap16(m1 - m0);
    }
    if (!dec1) {
      for (uint32_t i = 0; i < K; i++) {
        GV(oA1, inter[i]) = GV(oE2, i);
      }
    }
    n_run = n + 1;
    if (p.crc_poly) {
      // decode_tb_cb (sch.c:420-454): the checksum of the K hard bits after every half iteration (crc.c:92-140: MSB first,
      // zero initial state; zero = the block is good); this lane's block stops at its first match
      const uint32_t oC = (n_run & 1) ? oE1 : oA1;
      const uint32_t g  = p.crc_poly & 0xffffffu;
      uint32_t       c  = 0;
      for (uint32_t i = 0; i < K; i++) {
        const uint32_t x = GV(oC, i) > 0 ? 1u : 0u;
        c = ((c << 1) & 0xffffffu) ^ ((((c >> 23) ^ x) & 1u) ? g : 0u);
      }
      if (c == 0) {
        crc_good = true;
        break;
      }
    }
  }
  if (p.noi) {
    p.noi[cb] = (int)(n_run - p.n_begin);
  }
  if (p.crc_ok) {
    p.crc_ok[cb] = crc_good ? 1 : 0;
  }
  // decision (turbodecoder.c:370-378, turbodecoder_gen.c:260-277)
  const uint32_t oD        = (n_run & 1) ? oE1 : oA1;
  uint8_t*       out       = p.output + (p.desc ? (size_t)p.desc[cb].out_off : (size_t)cb * p.out_stride);
  const uint32_t out_bytes = p.desc ? p.desc[cb].out_bytes : K / 8;
  for (uint32_t jb = 0; jb < out_bytes; jb++) {
    uint32_t byte = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
      byte |= (GV(oD, jb * 8 + t) > 0 ? 0x80u : 0u) >> t;
    }
    out[jb] = (uint8_t)byte;
  }
  if (p.dec_llr) {
    short* o16 = p.dec_llr + (size_t)cb * K;
    for (uint32_t i = 0; i < K; i++) {
      o16[i] = GV(oD, i);
    }
  }
#undef GV
}

hipError_t launch_gen(const GenParams& p, hipStream_t stream)
{
  dim3 grid(ceil_div(p.n_cb, 64));
  hipLaunchKernelGGL(tdec_gen_kernel, grid, dim3(64), 0, stream, p);
  return hipGetLastError();
}

} // namespace turbo
} // namespace phyhip
