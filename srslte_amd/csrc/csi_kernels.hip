// csi_kernels.hip -- CSI weighting of a PDSCH codeword's soft bits (cfg->csi_enable) (gfx950).
//
// Reference behaviour: csi_correction (lib/src/phy/phch/pdsch.c:523-618), called between the descrambler and srsran_dlsch_decode2 (:735).  With c[] the
// codeword's CSI row (one float per modulation symbol) and c_max its largest entry:
//   8-bit soft bits      e = (int8_t)((float)e * (c[s] / c_max))                                             float quotient, float product, truncation
//   16-bit, vector body  w = saturate_int16(round_to_nearest_even(c[t] * ((float)INT16_MAX / c_max))), e = (e * w) >> 16      (_mm_cvtps_pi16, _mm_mulhi_pi16)
//   16-bit, left over    e = (int16_t)((float)e * (c[s] / c_max))                                            as the 8-bit rule: truncated, NOT halved
// The vector body (the LV_HAVE_SSE build) covers 16-QAM and 256-QAM whole and QPSK / 64-QAM in pairs of symbols (a, b); what it leaves over -- the last
// symbol of an odd QPSK / 64-QAM codeword, every symbol of BPSK -- takes the left-over rule.  Whose weight a bit takes (t above) is not always its own
// symbol's: the two symbols of a QPSK pair take each other's (_mm_blend_ps(_csi1, _csi2, 3)); of a 64-QAM pair's 12 bits, 0-3 take a's, 4-5 b's, 6-7 a's,
// 8-11 b's.  The library reproduces this, quirks included.  (QPSK / 64-QAM with ONE symbol overrun in the reference -- its loop bound is unsigned --: the
// symbol takes the left-over rule here.  A NaN product converts to 0 here and to INT16_MIN there; the host refuses a caller's row that is not finite.)
//
// One launch weights the call's codewords in place.  Launch shape: a workgroup of 256 lanes covers CSI_TILE_SYMS symbols of one codeword (a quarter of
// the demodulator's tile), a lane 16 bytes of soft bits per step (one dwordx4 load and store).  Every workgroup first reduces the WHOLE row to its maximum:
// a row is at most 62 KB (15.6 k REs) and sits in L2 behind the front end that wrote it, so the <= 31 workgroups of a codeword re-reading it costs less than
// a second launch, there is no atomic and no word to zero, and the result does not depend on scheduling (a maximum is exact in any order).  The quotient
// and the scale are IEEE divisions, every product is rounded by itself (rn_mul / rn_div of modem_arith.h: nothing contracts).
#include "csi_device.h"
#include "hip_common.h"
#include "modem_arith.h"

#include <cmath>

namespace phyhip {
namespace csi {

using namespace modem;

namespace {

// soft bit `b` of the codeword (n symbols)
template <typename T, int MOD>
__device__ __forceinline__ T weigh(T e, uint32_t b, const float* c, uint32_t n, float c_max, float scale)
{
  constexpr uint32_t QM = MOD == 0 ? 1 : 2 * MOD;
  const uint32_t     s  = b / QM;
  bool               vec = false;
  uint32_t           t   = s; // the symbol whose weight the bit takes
  if (sizeof(T) == 2) {
    if (MOD == 1) {
      vec = (s | 1u) < n;
      t   = s ^ 1u;
    } else if (MOD == 3) {
      const uint32_t a = s & ~1u, q = b - a * QM; // bit 0 .. 11 of the pair
      vec              = (s | 1u) < n;
      t                = a + (((q >= 4 && q < 6) || q >= 8) ? 1u : 0u);
    } else {
      vec = MOD != 0;
    }
  }
  if (vec) {
    const int w = min(max(__float2int_rn(rn_mul(c[t], scale)), -32768), 32767);
    return (T)(((int)e * w) >> 16);
  }
  return (T)(int)rn_mul((float)e, rn_div(c[s], c_max));
}

template <typename T, int MOD>
__device__ __forceinline__ void weigh_tile(const WeightJob& job, uint32_t tile, float c_max)
{
  constexpr uint32_t QM = MOD == 0 ? 1 : 2 * MOD, PER = 16 / sizeof(T);
  const uint32_t     b0 = tile * CSI_TILE_SYMS * QM, b1 = min(job.n, (tile + 1) * CSI_TILE_SYMS) * QM; // the tile's soft bits
  const float        scale = rn_div(32767.0f, c_max);
  T*                 e  = (T*)job.e;
  const bool         al = (((uintptr_t)e) & 15u) == 0;
  for (uint32_t u = b0 + threadIdx.x * PER; u < b1; u += 256u * PER) {
    if (al && u + PER <= b1) {
      union {
        uint4 q;
        T     v[PER];
      } x;
      x.q = *(const uint4*)(e + u);
#pragma unroll
      for (uint32_t k = 0; k < PER; k++) {
        x.v[k] = weigh<T, MOD>(x.v[k], u + k, job.csi, job.n, c_max, scale);
      }
      *(uint4*)(e + u) = x.q;
    } else {
      for (uint32_t k = 0; k < PER && u + k < b1; k++) {
        e[u + k] = weigh<T, MOD>(e[u + k], u + k, job.csi, job.n, c_max, scale);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void csi_weight_kernel(const WeightParams p)
{
  __shared__ float part[4];
  const bool       second = p.n_jobs == 2 && blockIdx.x >= p.tile1; // workgroup-uniform
  const WeightJob  job    = second ? p.job[1] : p.job[0];
  const uint32_t   tile   = blockIdx.x - (second ? p.tile1 : 0u);
  // the row's maximum (srsran_vec_max_fi, pdsch.c:530-534)
  float        m = -INFINITY;
  const float* c = job.csi;
  uint32_t     i = threadIdx.x;
  if ((((uintptr_t)c) & 15u) == 0) {
    const uint32_t n4 = job.n / 4;
    for (; i < n4; i += 256u) {
      const float4 v = ((const float4*)c)[i];
      m              = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    i = 4 * n4 + threadIdx.x;
  }
  for (; i < job.n; i += 256u) {
    m = fmaxf(m, c[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
  }
  if ((threadIdx.x & 63u) == 0) {
    part[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  const float c_max = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  switch (job.mod) {
    case 0:
      weigh_tile<T, 0>(job, tile, c_max);
      break;
    case 1:
      weigh_tile<T, 1>(job, tile, c_max);
      break;
    case 2:
      weigh_tile<T, 2>(job, tile, c_max);
      break;
    case 3:
      weigh_tile<T, 3>(job, tile, c_max);
      break;
    default:
      weigh_tile<T, 4>(job, tile, c_max);
      break;
  }
}

} // namespace

hipError_t launch_weight(const WeightParams& p, bool llr8, hipStream_t stream)
{
  if (p.n_jobs == 0 || p.n_jobs > 2) {
    return p.n_jobs ? hipErrorInvalidValue : hipSuccess;
  }
  uint32_t tiles = 0;
  for (uint32_t j = 0; j < p.n_jobs; j++) {
    if (!p.job[j].e || !p.job[j].csi || p.job[j].mod > 4 || p.job[j].n == 0 || (j == 1 && p.tile1 != tiles)) {
      return hipErrorInvalidValue;
    }
    tiles += ceil_div(p.job[j].n, CSI_TILE_SYMS);
  }
  if (llr8) {
    hipLaunchKernelGGL(csi_weight_kernel<int8_t>, dim3(tiles), dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL(csi_weight_kernel<int16_t>, dim3(tiles), dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

} // namespace csi
} // namespace phyhip
