// nr_chest_kernels.hip -- the NR shared channels' DMRS channel estimator and RE extraction on the device (gfx950).
//
// nr_dmrs_est_kernel restates srsran_dmrs_sch_estimate (dmrs_sch.c:798-981) on one port and one layer (delta = 0), one workgroup of four waves per
// codeword of the call.  P = pilots per DMRS symbol (6 or 4 per granted PRB, at most 1650), lanes stride over the pilots; every pass is separated from
// the next by a workgroup barrier and a lane only ever writes the LDS elements it owns (k = tid, tid + 256, ...):
//   chips      wave s makes the Gold chips of DMRS symbol s from its seed (make_chips of modem_arith.h: 12 or 8 bits per carrier PRB, at most 3300)
//   LSE        ls[s][k] = rx conj(pilot): pilot k of the concatenated granted PRBs (:71-133; the chips of carrier PRB p start at bit 2 p pilots_x_prb)
//   sums A     per symbol the lag-1 correlation of srsran_vec_estimate_frequency -> sync_err (:814-820)
//   phasor     ls[s][k] *= exp(j 2 pi sync_err k) where sync_err is normal (:824-831), a closed form per pilot (the product in double)
//   sums B     per symbol the plain sum and the power sum -> RSRP, EPRE, noise, CFO and the per-symbol cfo_correction (:835-879), lane 0
//   average    the per-symbol cfo_correction is removed (:882-888), the symbols are averaged (:899-905) into row 0
//   smoothing  5 taps through srsran_conv_same_cf's end rule (convolution.c:181-218) from row 0 into row 1; called in place, it is a recurrence (below)
//   output     one lane per RE of a table entry (nr_map.h): srsran_interp_linear_offset with M = 2 / 3 (interp.c:258-284; its last-segment rule),
//              the removal of the sync pre-compensation (:939-941), the time hold ce[i] * cfo_correction[l] (:975), stored as extracted estimates
// The output of a large grant is stored by up to 16 workgroups (blockIdx.y), each of which forms the estimates for itself.
// Every sum is reduced in a fixed order (lane partials in stride order, xor butterfly across the wave, the four waves through LDS added 0 .. 3): no
// atomics, and the same call gives the same bits every time.  The noise estimate also goes to device memory for the front end behind.
// LDS: 4 x 1650 float2 of estimates (51.6 KB) + 4 chip strips (2.1 KB) + the partial sums.
//
// nr_demap_kernel: srsran_pdsch_nr_cp's gather (pdsch_nr.c:225-270), the shape of pdsch_demap_kernel: blockIdx.y is the codeword, a workgroup of 192 lanes
// covers 16 table entries, lane t entry t / 12 and RE t % 12.  Every index is checked against the extents in the parameter block.
#include "hip_common.h"
#include "modem_arith.h"
#include "nr_chest_device.h"
#include <algorithm>

namespace phyhip {
namespace nr_chest {
namespace {

#define NR_EST_LANES 256u
#define NR_EST_MAX_SUMS 12u
#define NR_EST_WARM 64u // steps a run of the smoothing recurrence starts in front of its first output

// (complex products with every partial product rounded: a contracted a.y b.x - a.x b.y leaves a residue where the reference's is exactly zero, and a flat
// noiseless channel would no longer skip the isnormal branches)
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
  return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}
__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b) // a conj(b)
{
  return make_float2(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fsub_rn(__fmul_rn(a.y, b.x), __fmul_rn(a.x, b.y)));
}

// exp(j 2 pi f n): the turn count in double, reduced to (-0.5, 0.5] before the single-precision sine and cosine
__device__ __forceinline__ float2 phasor(float f, uint32_t n)
{
  double t = (double)f * (double)n;
  t -= rint(t);
  float s, c;
  sincospif(2.0f * (float)t, &s, &c);
  return make_float2(c, s);
}

// totals of K per-lane sums, the same in every lane.  part: [4][NR_EST_MAX_SUMS]
template <uint32_t K>
__device__ __forceinline__ void reduce(float (&v)[K], float (*part)[NR_EST_MAX_SUMS])
{
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (uint32_t q = 0; q < K; q++) {
    float x = v[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      x += __shfl_xor(x, off);
    }
    if ((tid & 63u) == 0) {
      part[tid >> 6][q] = x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < K; q++) {
    v[q] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
  }
  __syncthreads(); // part may be written again
}

__global__ __launch_bounds__(NR_EST_LANES) void nr_dmrs_est_kernel(const EstParams p)
{
  __shared__ float2 ls[nr_map::MAX_DMRS_SYM][nr_map::MAX_PILOTS];
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][MODEM_TILE_BITS / 128 + 4];
  __shared__ float  part[4][NR_EST_MAX_SUMS];
  __shared__ float2 cfo_corr[nr_map::NSYMB];
  __shared__ EstJob sjob;
  if (blockIdx.x >= p.n_jobs) {
    return;
  }
  const uint32_t tid = threadIdx.x;
  // blockIdx.y is the slice of the codeword's output this workgroup stores.  Every slice forms the same estimates from the same pilots in the same order
  // (1650 pilots are cheap next to tens of thousands of REs); slice 0 files the measurements.
  if (blockIdx.y > 0 && blockIdx.y * NR_EST_LANES >= p.jobs[blockIdx.x].n_seg * 12) { // (uniform: in front of every barrier) nothing to store
    return;
  }
  const bool files = blockIdx.y == 0;
  if (tid < sizeof(EstJob) / 4) {
    ((uint32_t*)&sjob)[tid] = ((const uint32_t*)(p.jobs + blockIdx.x))[tid];
  }
  if ((tid & 63u) == 0) {
    cb[tid >> 6][MODEM_TILE_BITS / 128] = 0; // chips_at reads one word past the last one
  }
  __syncthreads();
  const EstJob&  j    = sjob;
  const uint32_t nppp = j.type == 0 ? 6u : 4u, M = j.type == 0 ? 2u : 3u;
  const uint32_t P    = j.n_prbs * nppp;
  bool           ok   = j.nof_prb >= 1 && j.nof_prb <= nr_map::MAX_PRB && j.n_prbs >= 1 && j.n_prbs <= j.nof_prb && j.n_sym >= 1 && j.n_sym <= nr_map::MAX_DMRS_SYM &&
            j.type <= 1 && (uint64_t)j.o_prb + j.n_prbs <= p.n_prbs_total && (uint64_t)j.o_tab + j.n_seg <= p.n_tab && (uint64_t)j.o_ce + j.nof_re <= p.ce_points &&
            (j.n_seg == 0 || p.ce != nullptr) && (uint64_t)nr_map::NSYMB * 12 * j.nof_prb <= p.grid_points;
  for (uint32_t s = 0; s < nr_map::MAX_DMRS_SYM; s++) {
    ok = ok && (s >= j.n_sym || j.sym[s] < nr_map::NSYMB);
  }
  if (!ok) { // (uniform over the workgroup: in front of every further barrier)
    if (tid == 0 && files) {
      p.rec[blockIdx.x] = Record{NAN, NAN, NAN, NAN, NAN, NAN};
      if (p.noise) {
        p.noise[blockIdx.x] = 0.f;
      }
    }
    return;
  }
  const uint32_t n_sym = j.n_sym;
  // ---- chips: wave s, symbol s
  if ((tid >> 6) < n_sym) {
    modem::make_chips(p.x1_bits, p.x2_cols, j.seed[tid >> 6], 0, j.nof_prb * nppp * 2, cb[tid >> 6]);
  }
  __syncthreads();
  // ---- least-squares estimates
  const uint16_t* prbs = p.prbs + j.o_prb;
  for (uint32_t k = tid; k < P; k += NR_EST_LANES) {
    const uint32_t ord = k / nppp, q = k - ord * nppp;
    const uint32_t rb  = min((uint32_t)prbs[ord], j.nof_prb - 1);
    const uint32_t sc  = j.type == 0 ? 2 * q : 6 * (q >> 1) + (q & 1u);
    const uint32_t bit = 2 * (rb * nppp + q);
    for (uint32_t s = 0; s < n_sym; s++) {
      const float2   rx = p.grid[(j.sym[s] * j.nof_prb + rb) * 12 + sc];
      const uint32_t c  = modem::chips_at(cb[s], bit);
      const float2   d  = make_float2((c & 1u) ? -j.amplitude : j.amplitude, (c & 2u) ? -j.amplitude : j.amplitude);
      ls[s][k]          = cmul_conj(rx, d);
    }
  }
  __syncthreads();
  // ---- sums A: lag-1 correlations (vector_simd.c:1741-1784)
  float a[8];
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    a[q] = 0.f;
  }
  for (uint32_t k = tid; k < P; k += NR_EST_LANES) {
    if (k > 0) {
#pragma unroll
      for (uint32_t s = 0; s < nr_map::MAX_DMRS_SYM; s++) {
        if (s < n_sym) {
          const float2 t = cmul_conj(ls[s][k], ls[s][k - 1]);
          a[2 * s] += t.x;
          a[2 * s + 1] += t.y;
        }
      }
    }
  }
  reduce<8>(a, part);
  float sync_err = 0.0f;
  for (uint32_t s = 0; s < n_sym; s++) {
    sync_err += (float)((double)(-atan2f(a[2 * s + 1], a[2 * s])) * M_1_PI * 0.5f);
  }
  sync_err /= (float)n_sym;
  const bool sync_on = isfinite(sync_err) && fabsf(sync_err) >= 1.17549435e-38f; // isnormal
  // ---- the sync pre-compensation; sums B: plain sums and powers
  float b[NR_EST_MAX_SUMS];
#pragma unroll
  for (uint32_t q = 0; q < NR_EST_MAX_SUMS; q++) {
    b[q] = 0.f;
  }
  for (uint32_t k = tid; k < P; k += NR_EST_LANES) {
    const float2 ph = sync_on ? phasor(sync_err, k) : make_float2(1.f, 0.f);
#pragma unroll
    for (uint32_t s = 0; s < nr_map::MAX_DMRS_SYM; s++) {
      if (s < n_sym) {
        float2 v = ls[s][k];
        if (sync_on) {
          v        = cmul(v, ph);
          ls[s][k] = v;
        }
        b[3 * s] += v.x;
        b[3 * s + 1] += v.y;
        b[3 * s + 2] += v.x * v.x + v.y * v.y;
      }
    }
  }
  reduce<NR_EST_MAX_SUMS>(b, part);
  // ---- measurements (:835-879), every lane the same; lane 0 files them
  float2 corr[nr_map::MAX_DMRS_SYM];
  float  rsrp = 0.0f, epre = 0.0f;
  for (uint32_t s = 0; s < n_sym; s++) {
    corr[s] = make_float2(b[3 * s] / (float)P, b[3 * s + 1] / (float)P);
    rsrp += corr[s].x * corr[s].x + corr[s].y * corr[s].y;
    epre += b[3 * s + 2] / (float)P;
  }
  rsrp /= (float)n_sym;
  epre /= (float)n_sym;
  rsrp = (float)fmin((double)rsrp, (double)epre - (double)epre * 1e-7);
  float cfo_avg = 0.0f;
  for (uint32_t s = 0; s + 1 < n_sym; s++) {
    const float  td = j.dist_next[s];
    const float2 t  = cmul_conj(corr[s + 1], corr[s]);
    const float  ph = atan2f(t.y, t.x);
    if (isfinite(td) && fabsf(td) >= 1.17549435e-38f) {
      cfo_avg = (float)((double)cfo_avg + (double)ph / (2.0 * M_PI * (double)td * (double)(n_sym - 1)));
    }
  }
  const bool cfo_on = isfinite(cfo_avg) && fabsf(cfo_avg) >= 1.17549435e-38f;
  if (tid < nr_map::NSYMB) {
    float2 c = make_float2(1.f, 0.f);
    if (cfo_on) {
      const float arg0 = (float)((double)atan2f(corr[0].y, corr[0].x) - 2.0 * M_PI * (double)j.dist0[j.sym[0]] * (double)cfo_avg);
      const float arg  = (float)((double)arg0 + 2.0 * M_PI * (double)cfo_avg * (double)j.dist0[tid]);
      sincosf(arg, &c.y, &c.x);
    }
    cfo_corr[tid] = c;
  }
  if (tid == 0 && files) {
    const float noise = epre - rsrp;
    p.rec[blockIdx.x] = Record{noise, rsrp, epre, cfo_avg, sync_err / j.subc_hz, sync_err};
    if (p.noise) {
      p.noise[blockIdx.x] = noise;
    }
  }
  if (j.n_seg == 0) { // (uniform) measurements only
    return;
  }
  __syncthreads();
  // ---- the CFO removal and the time average into row 0
  const float inv_n = 1.0f / (float)n_sym;
  for (uint32_t k = tid; k < P; k += NR_EST_LANES) {
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (uint32_t s = 0; s < nr_map::MAX_DMRS_SYM; s++) {
      if (s < n_sym) {
        float2 v = ls[s][k];
        if (cfo_on) {
          v = cmul_conj(v, cfo_corr[j.sym[s]]);
        }
        acc = s == 0 ? v : make_float2(acc.x + v.x, acc.y + v.y);
      }
    }
    ls[0][k] = make_float2(acc.x * inv_n, acc.y * inv_n);
  }
  __syncthreads();
  // ---- smoothing: row 0 -> row 1, srsran_conv_same_cf as the reference calls it: IN PLACE (dmrs_sch.c:909-910).  The two first and the two last outputs
  // come from copies of the input (convolution.c:190-208, :213-216 with M = 5: the virtual neighbours in front of element 0 are 3 x[1] - 2 x[0] and
  // 4 x[1] - 3 x[0], those behind the last one 4 x[N-1] - 3 x[N-2] and 5 x[N-1] - 4 x[N-2]).  The outputs in between (:210-212) read the two elements in
  // front of them after they were overwritten: y[i] = f0 y[i-2] + f1 y[i-1] + f2 x[i] + f3 x[i+1] + f4 x[i+2], a recurrence.  Its homogeneous part decays
  // by 0.52 per step (the larger root of z^2 = f1 z + f0 with the Gauss taps), so a lane that owns a run of consecutive outputs starts NR_EST_WARM = 64
  // steps in front of it from x itself: what the start value leaves of itself after 64 steps, 5e-19, is far below a float's rounding.  The run that
  // starts at element 2 takes y[0] and y[1] as they are.  Every real index read lies in [0, P), P >= 4.
  const float2* x = ls[0];
  auto          end_tap = [&](uint32_t k) { // outputs 0, 1, P - 2, P - 1
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 5; t++) {
      const int i = (int)k - 2 + t;
      float2    v;
      if (i < 0) {
        const float w = (float)(2 - i); // i = -1: 3, -2: 4
        v             = make_float2(w * x[1].x - (w - 1.f) * x[0].x, w * x[1].y - (w - 1.f) * x[0].y);
      } else if (i >= (int)P) {
        const float w = (float)(4 + i - (int)P); // i = P: 4, P + 1: 5
        v             = make_float2(w * x[P - 1].x - (w - 1.f) * x[P - 2].x, w * x[P - 1].y - (w - 1.f) * x[P - 2].y);
      } else {
        v = x[i];
      }
      acc.x += v.x * j.filter[t];
      acc.y += v.y * j.filter[t];
    }
    return acc;
  };
  if (tid < 4) {
    const uint32_t k = tid < 2 ? tid : P - 4 + tid;
    ls[1][k]         = end_tap(k);
  }
  {
    const uint32_t n_mid = P - 4, run = (n_mid + NR_EST_LANES - 1) / NR_EST_LANES; // outputs 2 .. P - 3
    const uint32_t lo = 2 + tid * run, hi = min(lo + run, P - 2);
    if (run > 0 && lo < hi) {
      const uint32_t i0 = lo >= 2 + NR_EST_WARM ? lo - NR_EST_WARM : 2;
      float2         y2 = i0 == 2 ? end_tap(0) : x[i0 - 2], y1 = i0 == 2 ? end_tap(1) : x[i0 - 1];
      for (uint32_t i = i0; i < hi; i++) {
        float2 acc = make_float2(y2.x * j.filter[0], y2.y * j.filter[0]);
        acc.x += y1.x * j.filter[1], acc.y += y1.y * j.filter[1];
#pragma unroll
        for (int t = 2; t < 5; t++) {
          acc.x += x[i - 2 + t].x * j.filter[t];
          acc.y += x[i - 2 + t].y * j.filter[t];
        }
        y2 = y1, y1 = acc;
        if (i >= lo) {
          ls[1][i] = acc;
        }
      }
    }
  }
  __syncthreads();
  // ---- interpolation, removal of the sync pre-compensation, time hold, extraction
  const float        inv_M   = 1.0f / (float)M;
  const float        back_f  = -sync_err / (float)M;
  const nr_map::Seg* tab     = p.tab + j.o_tab;
  float2*            out     = p.ce + j.o_ce;
  const float2*      sm      = ls[1];
  for (uint32_t idx = blockIdx.y * NR_EST_LANES + tid; idx < j.n_seg * 12; idx += NR_EST_LANES * gridDim.y) {
    const uint32_t    e = idx / 12, sc = idx - e * 12;
    const nr_map::Seg g = tab[e];
    if (!((g.mask >> sc) & 1u)) {
      continue;
    }
    const uint32_t l = g.ce_sym >> 16, m = (g.ce_sym & 0xffffu) + sc;
    const uint32_t dst = g.out_off + (uint32_t)__popc(g.mask & ((1u << sc) - 1u));
    if (l >= nr_map::NSYMB || m >= P * M || dst >= j.nof_re) {
      continue;
    }
    uint32_t i = m / M;
    const uint32_t r = m - i * M;
    float2         v;
    if (i + 1 < P) { // interp.c:267-276
      const float2 d = make_float2((sm[i + 1].x - sm[i].x) * inv_M, (sm[i + 1].y - sm[i].y) * inv_M);
      v              = make_float2(sm[i].x + d.x * (float)r, sm[i].y + d.y * (float)r);
    } else { // :278-283
      i              = P - 1;
      const float2 d = make_float2(sm[i].x - sm[i - 1].x, sm[i].y - sm[i - 1].y);
      v              = make_float2(sm[i].x + ((float)r * d.x) / (float)M, sm[i].y + ((float)r * d.y) / (float)M);
    }
    if (sync_on) {
      v = cmul(v, phasor(back_f, m));
    }
    out[dst] = cmul(v, cfo_corr[l]);
  }
}

__global__ __launch_bounds__(12 * NR_DEMAP_SEGS) void nr_demap_kernel(const DemapParams p)
{
  if (blockIdx.y >= p.n_jobs) {
    return;
  }
  const DemapJob j = p.jobs[blockIdx.y];
  const uint32_t e = blockIdx.x * NR_DEMAP_SEGS + threadIdx.x / 12u;
  const uint32_t k = threadIdx.x % 12u;
  if (e >= j.n_seg || (uint64_t)j.o_tab + e >= p.n_tab || (uint64_t)j.o_out + j.nof_re > p.out_points) {
    return;
  }
  const nr_map::Seg s   = p.tab[j.o_tab + e];
  const uint32_t    src = s.grid_off + k;
  const uint32_t    dst = s.out_off + (uint32_t)__popc(s.mask & ((1u << k) - 1u));
  if (((s.mask >> k) & 1u) && src < p.grid_points && dst < j.nof_re) {
    p.out[j.o_out + dst] = p.grid[src];
  }
}

} // namespace

hipError_t launch_est(const EstParams& p, hipStream_t stream)
{
  if (p.n_jobs == 0) {
    return hipSuccess;
  }
  if (!p.grid || !p.jobs || !p.prbs || !p.rec || !p.x1_bits || !p.x2_cols || (p.n_tab && !p.tab)) {
    return hipErrorInvalidValue;
  }
  // slices: at most 8 table entries' REs per lane, at most 16 workgroups per codeword
  const uint32_t slices = std::min(16u, std::max(1u, ceil_div(p.max_seg * 12u, NR_EST_LANES * 8u)));
  hipLaunchKernelGGL(nr_dmrs_est_kernel, dim3(p.n_jobs, slices), dim3(NR_EST_LANES), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_demap(const DemapParams& p, hipStream_t stream)
{
  if (p.n_jobs == 0 || p.max_seg == 0) {
    return hipSuccess;
  }
  if (!p.grid || !p.jobs || !p.tab || !p.out || p.n_jobs > 65535u || p.max_seg > nr_map::MAX_SEG) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(nr_demap_kernel, dim3(ceil_div(p.max_seg, NR_DEMAP_SEGS), p.n_jobs), dim3(12 * NR_DEMAP_SEGS), 0, stream, p);
  return hipGetLastError();
}

} // namespace nr_chest
} // namespace phyhip
