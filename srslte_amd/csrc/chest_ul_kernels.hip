// chest_ul_kernels.hip -- the PUSCH channel estimator, srsran_chest_ul_estimate_pusch (chest_ul.c:370-404), for the grants of a call in ONE launch:
// one workgroup of four waves per grant.
//   pass one   lanes stride over the grant's 2 n references (at most 11 per lane, all loaded before the first is used: the rows are read across the bus):
//              ls = rx conj(r) (srsran_vec_prod_conj_ccc) into LDS, |rx|^2 into the lane's sum
//   barrier
//   pass two   the same lanes, the same points: sm = the 3-tap filter over the LDS neighbours with srsran_conv_same_cf's end rule (convolution.c:181-218:
//              the virtual neighbour in front of element 0 is 3 ls[1] - 2 ls[0], the one behind the last 3 ls[N-1] - 2 ls[N-2]), stored to every row of
//              the slot; the lane's share of |sm - ls|^2 per slot, of the CFO phasor sum ls[0][k] conj(ls[1][k]) and of each slot's time-alignment phasor
//              sum ls[k] conj(ls[k-1])
//   reduction  nine sums, in a fixed order: xor butterfly across the wave, the four waves through LDS, lane 0 adds them 0 .. 3 and finishes the noise
//              estimate with the reference's calibration (chest_ul.c:211-219, in double as there).  No atomics: a run gives the same bits every time.
// LDS: 2 x 1296 float2 of estimates (20.25 KB) + 4 x 9 floats.
#include "chest_ul_device.h"

namespace phyhip {
namespace chest_ul {
namespace {

#define CHEST_UL_LANES 256u
#define CHEST_UL_SUMS 9u // noise[2], |rx|^2, cfo re / im, ta[2] re / im
#define CHEST_UL_STRIDES ((2u * CHEST_UL_MAX_REFS + CHEST_UL_LANES - 1u) / CHEST_UL_LANES) // 11: a lane's points at most

__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b) // a conj(b)
{
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

__global__ __launch_bounds__(CHEST_UL_LANES) void chest_ul_kernel(const Params p)
{
  __shared__ float2 ls[2 * CHEST_UL_MAX_REFS];
  __shared__ float  part[CHEST_UL_LANES / 64][CHEST_UL_SUMS];
  if (blockIdx.x >= p.n_jobs) {
    return;
  }
  const Job      j = p.jobs[blockIdx.x];
  const uint32_t n = j.n, tid = threadIdx.x;
  const uint64_t out_rows = (uint64_t)max(j.row0[0] + j.rows[0], j.row0[1] + j.rows[1]);
  if (n < 2 || n > CHEST_UL_MAX_REFS || (uint64_t)j.o_rx + 2 * n > p.in_points || (uint64_t)j.o_r + 2 * n > p.in_points ||
      (uint64_t)j.o_out + out_rows * n > p.out_points) { // (uniform over the workgroup: in front of every barrier)
    if (tid == 0) {
      p.rec[blockIdx.x] = Record{NAN, NAN, {NAN, NAN}, {{NAN, NAN}, {NAN, NAN}}};
      if (p.eq) {
        p.eq[blockIdx.x] = modem::EqJob{j.end_pair, 0.f, 0u};
      }
    }
    return;
  }
  const float2* rx = p.in + j.o_rx;
  const float2* r  = p.in + j.o_r;
  float         s[CHEST_UL_SUMS];
#pragma unroll
  for (uint32_t q = 0; q < CHEST_UL_SUMS; q++) {
    s[q] = 0.f;
  }
  // (the rows are read across the bus: all of a lane's loads are issued before the first is used -- the index is clamped into the job, never branched on)
  float2         y[CHEST_UL_STRIDES], d[CHEST_UL_STRIDES];
  const uint32_t strides = (2 * n + CHEST_UL_LANES - 1) / CHEST_UL_LANES;
#pragma unroll
  for (uint32_t q = 0; q < CHEST_UL_STRIDES; q++) {
    y[q] = d[q] = make_float2(0.f, 0.f);
    if (q < strides) { // (uniform)
      const uint32_t i = min(tid + q * CHEST_UL_LANES, 2 * n - 1);
      y[q]             = rx[i];
      d[q]             = r[i];
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < CHEST_UL_STRIDES; q++) {
    const uint32_t i = tid + q * CHEST_UL_LANES;
    if (i < 2 * n) {
      ls[i] = cmul_conj(y[q], d[q]);
      s[2] += y[q].x * y[q].x + y[q].y * y[q].y;
    }
  }
  __syncthreads();
  const bool smooth = j.filter_len == 3;
  for (uint32_t i = tid; i < 2 * n; i += CHEST_UL_LANES) {
    const uint32_t slot = i >= n ? 1u : 0u, k = i - slot * n;
    const float2*  e = ls + slot * n; // k - 1 and k + 1 are read inside [0, n) only
    const float2   c = e[k];
    float2         sm = c;
    if (smooth) {
      float2 a, b;
      if (k > 0) {
        a = e[k - 1];
      } else {
        a = make_float2(3.f * e[1].x - 2.f * c.x, 3.f * e[1].y - 2.f * c.y);
      }
      if (k + 1 < n) {
        b = e[k + 1];
      } else {
        b = make_float2(3.f * c.x - 2.f * e[n - 2].x, 3.f * c.y - 2.f * e[n - 2].y);
      }
      sm = make_float2(a.x * j.filter[0] + c.x * j.filter[1] + b.x * j.filter[2], a.y * j.filter[0] + c.y * j.filter[1] + b.y * j.filter[2]);
      const float dx = sm.x - c.x, dy = sm.y - c.y;
      s[slot] += dx * dx + dy * dy;
    }
    float2* o = p.out + j.o_out + (size_t)j.row0[slot] * n + k;
    for (uint32_t l = 0; l < j.rows[slot]; l++) {
      o[(size_t)l * n] = sm;
    }
    if (slot == 0) {
      const float2 t = cmul_conj(c, ls[n + k]);
      s[3] += t.x;
      s[4] += t.y;
    }
    if (k > 0) {
      const float2 t = cmul_conj(c, e[k - 1]);
      s[5 + 2 * slot] += t.x;
      s[6 + 2 * slot] += t.y;
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < CHEST_UL_SUMS; q++) {
    float v = s[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v += __shfl_xor(v, off);
    }
    if ((tid & 63u) == 0) {
      part[tid >> 6][q] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float t[CHEST_UL_SUMS];
#pragma unroll
    for (uint32_t q = 0; q < CHEST_UL_SUMS; q++) {
      t[q] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
    }
    float noise = 0.f;
    if (smooth) { // estimate_noise_pilots, chest_ul.c:200-221
      float power = 0.f;
      power += t[0] / (float)n;
      power += t[1] / (float)n;
      power /= 2;
      const float  w = j.filter[0];
      const float  a = (float)(7.419 * w * w + 0.1117 * w - 0.005387);
      noise          = (float)(power / (a * 0.8));
    }
    p.rec[blockIdx.x] = Record{noise, t[2] / (float)(2 * n), {t[3], t[4]}, {{t[5], t[6]}, {t[7], t[8]}}};
    if (p.eq) {
      p.eq[blockIdx.x] = modem::EqJob{j.end_pair, noise, noise > 0.f ? 1u : 0u};
    }
  }
}

} // namespace

hipError_t launch(const Params& p, hipStream_t stream)
{
  if (p.n_jobs == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(chest_ul_kernel, dim3(p.n_jobs), dim3(CHEST_UL_LANES), 0, stream, p);
  return hipGetLastError();
}

} // namespace chest_ul
} // namespace phyhip
