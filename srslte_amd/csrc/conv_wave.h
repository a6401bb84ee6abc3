// conv_wave.h -- the device code one wave runs on one frame of the LTE convolutional code, shared by conv_kernels.hip (Viterbi frames, PDCCH candidates) and
// pbch_kernels.hip (PBCH hypotheses): the rate de-matcher srsran_rm_conv_rx on a soft-bit source, the quantiser of srsran_viterbi_decode_f, the reference's
// 16-bit 64-state decoder with one lane per trellis state (the layout is described at the head of conv_kernels.hip) and the 16-bit CRC.  Device code only.
#pragma once
#include "conv_device.h"

#include <climits>

namespace phyhip {
namespace conv {
namespace {

constexpr uint32_t kPoly[3] = {0x6D, 0x4F, 0x57};

__device__ __forceinline__ uint32_t uniform(uint32_t v) // a value every lane holds alike, made known as such
{
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t sign_of(uint32_t butterfly, uint32_t poly) // Branchtab37_sse2[k].c[i]
{
  return (__builtin_popcount((2u * butterfly) & poly) & 1) ? 0xFFFFu : 0u;
}

// the branch metric of butterfly (sg0, sg1, sg2) on the three symbols at sym[p]: avg(avg(t0 ^ s0, t1 ^ s1), t2 ^ s2) >> 3, avg = (a + b + 1) >> 1
__device__ __forceinline__ uint32_t branch_metric(const uint16_t* sym, uint32_t p, uint32_t sg0, uint32_t sg1, uint32_t sg2)
{
  const uint32_t x0 = sg0 ^ sym[p], x1 = sg1 ^ sym[p + 1], x2 = sg2 ^ sym[p + 2];
  return ((((x0 + x1 + 1) >> 1) + x2 + 1) >> 1) >> 3;
}

// One frame on the calling wave (all 64 lanes, block of 64; L and tail wave-uniform).  sym: LDS, 3 L symbols (tail biting: laid out three times by
// wrapping) or 3 (L + 6); words: LDS, nof_words(L, tail) of them; out: L bits, one per byte (global); bits: nullptr or an LDS copy of them.
__device__ __forceinline__ void viterbi_wave(const uint16_t* sym, uint32_t L, bool tail, uint64_t* words, uint8_t* out, uint8_t* bits)
{
  const uint32_t lane = threadIdx.x, bf = lane >> 1, odd = lane & 1;
  const uint32_t sg0 = sign_of(bf, kPoly[0]), sg1 = sign_of(bf, kPoly[1]), sg2 = sign_of(bf, kPoly[2]);
  const int      a0 = (int)(bf * 4), a1 = (int)((bf + 32) * 4);
  const uint32_t nsteps = tail ? 3 * L : L + 6, t_lo = (tail ? L : 0) + 6, n3 = 3 * L;
  uint32_t       m = 0, p = 0;
  uint32_t       metric = branch_metric(sym, 0, sg0, sg1, sg2);
  for (uint32_t t = 0; t < nsteps; t++) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute(a0, (int)m), c = (uint32_t)__builtin_amdgcn_ds_bpermute(a1, (int)m);
    // the next step's branch metric does not wait for the exchange
    p += 3;
    if (tail && p == n3) {
      p = 0;
    }
    const uint32_t next     = t + 1 < nsteps ? branch_metric(sym, p, sg0, sg1, sg2) : 0u;
    const uint32_t m_metric = 8191u - metric;
    const uint32_t x = (a + (odd ? m_metric : metric)) & 0xFFFFu, y = (c + (odd ? metric : m_metric)) & 0xFFFFu;
    const bool     dec = (int16_t)(uint16_t)(x - y) > 0;
    m                  = dec ? y : x;
    metric             = next;
    const uint64_t w   = __ballot(dec);
    if (t >= t_lo && lane == 0) {
      words[t - t_lo] = w;
    }
  }
  __syncthreads();
  const uint32_t nw = nsteps > t_lo ? nsteps - t_lo : 0, span = nw > L ? nw : L;
  uint32_t       state = 0;
  for (int blk = (int)((span + 63) / 64) - 1; blk >= 0; blk--) {
    const uint32_t idx = (uint32_t)blk * 64 + lane;
    const uint64_t w   = idx < nw ? words[idx] : 0; // past the steps that ran: the zeros the reference's clear left
    const int      wlo = (int)(uint32_t)w, whi = (int)(uint32_t)(w >> 32);
    uint64_t       km  = 0;
#pragma unroll
    for (int j = 63; j >= 0; j--) {
      const uint64_t ww = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(whi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane(wlo, j);
      const uint32_t k  = (uint32_t)(ww >> state) & 1u;
      state             = (state >> 1) | (k << 5);
      km |= (uint64_t)k << j;
    }
    if (idx < L) {
      const uint8_t bit = (uint8_t)((km >> lane) & 1u);
      out[idx]          = bit;
      if (bits) {
        bits[idx] = bit;
      }
    }
  }
}

// srsran_vec_quant_fus as the reference's compiler left it: one fused multiply-add, truncation, clamps.  cvttss2si gives INT_MIN outside int32 (and on NaN).
__device__ __forceinline__ uint16_t quant_fus(float gain, float x)
{
  const float v = __builtin_fmaf(gain, x, 32767.5f);
  int         q = (v > -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN;
  q             = q < 0 ? 0 : q;
  q             = q > 65535 ? 65535 : q;
  return (uint16_t)q;
}

__device__ __forceinline__ float wave_max(float v)
{
  for (int o = 32; o > 0; o >>= 1) {
    v = fmaxf(v, __shfl_xor(v, o));
  }
  return v;
}

__constant__ uint8_t kPermCC[32]    = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
__constant__ uint8_t kPermCCInv[32] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14, 17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};

// srsran_rm_conv_rx of E soft bits e(0) .. e(E - 1) onto the 3 L outputs rm[] (LDS): the lane that owns an output position walks the inputs that land on it
// in increasing k -- the sum order of the reference's one pass over the input.  The position's first input is its rank among the non-dummy places of the
// circular buffer; the others follow every 3 L inputs.  Returns the lane's max(1e-9, |rm|) of its positions (the quantiser's start value).
template <class SoftBit>
__device__ __forceinline__ float rm_conv_wave(SoftBit&& e, uint32_t E, uint32_t L, float* rm)
{
  const uint32_t lane = threadIdx.x, n3 = 3 * L;
  const uint32_t nrows = (L - 1) / 32 + 1, K_p = nrows * 32, ndummy = K_p - L; // ndummy < 32: the dummies are the first ndummy places of row 0
  uint32_t       dmask = 0;                                                    // columns (after the permutation) whose row 0 is a dummy
  for (uint32_t c = 0; c < 32; c++) {
    dmask |= (kPermCC[c] < ndummy ? 1u : 0u) << c;
  }
  float mx = 1e-9f;
  for (uint32_t o = lane; o < n3; o += 64) {
    const uint32_t i = o / 3, s = o - 3 * i, row = (i + ndummy) >> 5, col = kPermCCInv[(i + ndummy) & 31];
    const uint32_t dummies = s * ndummy + __builtin_popcount(dmask & ((1u << col) - 1u)) + ((row > 0 && ((dmask >> col) & 1u)) ? 1u : 0u);
    float          t       = 10000.f; // SRSRAN_RX_NULL, and its comparisons as written
    for (uint32_t k = K_p * s + col * nrows + row - dummies; k < E; k += n3) {
      const float v = e(k);
      if (t == 10000.f) {
        t = v;
      } else if (v != 10000.f) {
        t += v;
      }
    }
    t     = t == 10000.f ? 0.f : t;
    rm[o] = t;
    mx    = fmaxf(mx, fabsf(t));
  }
  return mx;
}

// the 16 bits behind the n payload bits at bits[] (one per byte), first bit highest, xor the CRC (0x11021) of the payload
__device__ __forceinline__ uint32_t crc_rem(const uint8_t* bits, uint32_t n)
{
  uint32_t crc = 0, p_bits = 0;
  for (uint32_t i = 0; i < n; i++) {
    crc = ((crc << 1) ^ ((((crc >> 15) ^ bits[i]) & 1u) ? 0x1021u : 0u)) & 0xFFFFu;
  }
  for (uint32_t i = 0; i < 16; i++) {
    p_bits = (p_bits << 1) | bits[n + i];
  }
  return p_bits ^ crc;
}

} // namespace
} // namespace conv
} // namespace phyhip
