// prach_kernels.hip -- PRACH detection (srsran_prach_detect_offset / srsran_prach_process, prach.c:772-914) for gfx950 in two launches.
//
//   1. prach_stream_fft_kernel: the forward transform of N = 1536 * D points pruned to the 839 bins the detector reads.  With n = D m + d,
//        X[k] = sum_d w_N^(d k) F_d[k mod 1536],   F_d = the 1536-point DFT of the decimated stream x[D m + d],
//      one workgroup per (occasion, stream d) runs a 1536-point LDS transform on its strided input, in double, and stores the 839 values of F_d the
//      wanted bins need.  The D-point second step over all N outputs and the mirror re-ordering pass of the four-step transform do not exist.
//   2. prach_corr_kernel: one workgroup per (occasion, searched root).  It combines the D streams into the 839 bins (w_N from a table in double, 1 / sqrt(N)),
//      multiplies by the conjugate root spectrum (corr_spec, :790), sums corr_spec[k] conj(corr_spec[k + 1]) over k < 838 (cross, :792), evaluates the
//      unnormalised backward 839-point DFT from LDS, takes |.|^2 and its mean (corr_ave, :800) and, per window, the maximum and its first position
//      (:811-829).  839 is prime: the transform is evaluated directly, blocked so that a lane carries its outputs n = lane + 256 q through one pass over
//      k.  With w^(n k) = w^(256 q k) w^(lane k) the pass reads ONE gathered twiddle per k (the only access with bank conflicts) and four lane-uniform
//      operands y_q[k] = corr_spec[k] w^(256 q k), which are prepared once in LDS.
// Every sum runs in an order fixed by the block shape alone: the same bits on every run and for every number of occasions in the launch.
#include "fft_device.h"
#include "hip_common.h"
#include "prach_device.h"

namespace phyhip {
namespace prach {

using namespace fft;

constexpr int kStreamLanes = 256;
constexpr int kCorrLanes   = 256;
constexpr int kQ           = (kNzc + kCorrLanes - 1) / kCorrLanes; // outputs a lane carries
constexpr int kChunk       = 32; // terms of the backward DFT summed before they join the total

__device__ __forceinline__ double2 dadd(double2 a, double2 b)
{
  return make_double2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ double2 dmul(double2 a, double2 b)
{
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One Stockham pass of radix R over the 1536 points of image a into image b (the index scheme of lds_pass, dft_kernels.hip); NS = product of the earlier
// radices; tw = e^{-j 2 pi i / 1536} in double.  The radix-R butterfly is evaluated directly against the same table.
template <int R>
__device__ __forceinline__ void first_pass(const double2* a, double2* b, int NS, const double2* __restrict__ tw)
{
  constexpr int NB = kFirst / R;
  for (int q = threadIdx.x; q < NB; q += kStreamLanes) {
    const int k = q % NS, step = kFirst / (NS * R);
    double2   v[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      v[r] = a[q + r * NB];
      if (r > 0 && NS > 1) {
        v[r] = dmul(v[r], tw[k * r * step]); // k < NS, r < R: the index stays below 1536
      }
    }
    const int j0 = (q / NS) * NS * R + k;
#pragma unroll
    for (int s = 0; s < R; s++) {
      double2 acc = v[0];
#pragma unroll
      for (int r = 1; r < R; r++) {
        acc = dadd(acc, dmul(v[r], tw[((r * s) % R) * NB]));
      }
      b[j0 + s * NS] = acc;
    }
  }
  __syncthreads();
}

// The first stage runs in double: the record's tolerance on prach_bins is the float rounding of the reference's OUTPUT (its transform is held in double by
// the oracle), which a float transform of 1536 D points is not expected to meet.  What double costs here against the float 1536-point plan of
// fft_device.h has not been measured; the stage is 6 passes over 1536 points per workgroup.
__global__ __launch_bounds__(kStreamLanes) void prach_stream_fft_kernel(const Params p)
{
  __shared__ double2 img[2][kFirst];
  const int          d = blockIdx.x, occ = blockIdx.y, D = p.D;
  const float2*      src = p.sig + (size_t)occ * p.N + d;
  double2*           dst = p.streams + ((size_t)occ * D + d) * kNzc;
  const int          first = p.k0[occ] % kFirst; // F_d is periodic in 1536: the wanted bins are 839 consecutive ones from here, cyclically
  for (int n = threadIdx.x; n < kFirst; n += kStreamLanes) {
    const float2 x = src[(size_t)n * D];
    img[0][n]      = make_double2((double)x.x, (double)x.y);
  }
  __syncthreads();
  first_pass<4>(img[0], img[1], 1, p.tw_first);
  first_pass<4>(img[1], img[0], 4, p.tw_first);
  first_pass<4>(img[0], img[1], 16, p.tw_first);
  first_pass<4>(img[1], img[0], 64, p.tw_first);
  first_pass<2>(img[0], img[1], 256, p.tw_first);
  first_pass<3>(img[1], img[0], 512, p.tw_first);
  for (int k = threadIdx.x; k < kFirst; k += kStreamLanes) {
    int i = k - first;
    i += i < 0 ? kFirst : 0;
    if (i < kNzc) {
      dst[i] = img[0][k];
    }
  }
}

// The spectrum of a root (get_precoded_dft, prach.c:346-357): the forward 839-point DFT of its sequence with norm -- object creation, once per root.
// Evaluated directly in double, twiddles from sincospi: the record's tolerance on the spectra is 1.2e-6 of a bin, and the float direct evaluation of
// dft_kernel (839 unit terms into one float sum: about 6e-7 rms by the rounding model, a few times that at worst over 64 x 839 bins) was not expected to
// stay inside it.  That estimate was not put to a run; this path is cold.
__global__ __launch_bounds__(kCorrLanes) void prach_root_spec_kernel(const float2* __restrict__ seq, float2* __restrict__ spec)
{
  __shared__ double2 x[kNzc];
  __shared__ double2 tw[kNzc];
  const float2*      in = seq + (size_t)blockIdx.x * kNzc;
  for (int n = threadIdx.x; n < kNzc; n += kCorrLanes) {
    x[n] = make_double2((double)in[n].x, (double)in[n].y);
    double sn, cs;
    sincospi(-2.0 * (double)n / (double)kNzc, &sn, &cs);
    tw[n] = make_double2(cs, sn);
  }
  __syncthreads();
  const double norm = 1.0 / sqrt((double)kNzc);
  for (int k = threadIdx.x; k < kNzc; k += kCorrLanes) {
    double2 acc = make_double2(0.0, 0.0);
    int     idx = 0;
    for (int n = 0; n < kNzc; n++) {
      acc = dadd(acc, dmul(x[n], tw[idx]));
      idx += k;
      idx -= idx >= kNzc ? kNzc : 0;
    }
    spec[(size_t)blockIdx.x * kNzc + k] = make_float2((float)(acc.x * norm), (float)(acc.y * norm));
  }
}

// sum over the block in a fixed order: lane sums first (the caller's), then a halving tree
template <class T, class Add>
__device__ __forceinline__ T block_sum(T v, T* red, Add add)
{
  const int tid = threadIdx.x;
  red[tid]      = v;
  __syncthreads();
  for (int s = kCorrLanes / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] = add(red[tid], red[tid + s]);
    }
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kCorrLanes) void prach_corr_kernel(const Params p)
{
  __shared__ float2 y[kQ][kNzc]; // y[0] = corr_spec
  __shared__ float2 tw[kNzc];
  __shared__ float  corr[kNzc];
  __shared__ float2 red[kCorrLanes];
  const int         r = blockIdx.x, occ = blockIdx.y, tid = threadIdx.x;
  const int         N = p.N, D = p.D, k0 = p.k0[occ];
  const double2*    F  = p.streams + (size_t)occ * D * kNzc;
  const float2*     rs = p.root_spec + (size_t)r * kNzc;
  uint32_t*         rec = p.rec + ((size_t)occ * p.n_search + r) * p.rec_words;

  for (int i = tid; i < kNzc; i += kCorrLanes) {
    tw[i] = p.tw_zc[i];
  }
  // the bins: X[k0 + i] = sum_d w_N^(d k) F_d[i], d ascending, in double as the first stage
  for (int i = tid; i < kNzc; i += kCorrLanes) {
    int k = k0 + i;
    k -= k >= N ? N : 0;
    double2 sum = F[i];
    int     idx = 0;
    for (int d = 1; d < D; d++) {
      idx += k;
      idx -= idx >= N ? N : 0;
      sum = dadd(sum, dmul(F[d * kNzc + i], p.tw_n[idx]));
    }
    const float2 acc = make_float2((float)(sum.x * p.norm), (float)(sum.y * p.norm));
    if (r == 0 && p.bins_out) {
      p.bins_out[(size_t)occ * kNzc + i] = acc;
    }
    const float2 s = rs[i];
    y[0][i]        = make_float2(acc.x * s.x + acc.y * s.y, acc.y * s.x - acc.x * s.y); // bins * conj(root spectrum)
  }
  __syncthreads();
  // cross: N_zc - 1 products
  float2 cr = make_float2(0.f, 0.f);
  for (int k = tid; k < kNzc - 1; k += kCorrLanes) {
    const float2 a = y[0][k], b = y[0][k + 1];
    cr.x += a.x * b.x + a.y * b.y;
    cr.y += a.y * b.x - a.x * b.y;
  }
  cr = block_sum(cr, red, [](float2 a, float2 b) { return cadd(a, b); });
  // y_q[k] = corr_spec[k] e^{+j 2 pi 256 q k / 839}
  for (int k = tid; k < kNzc; k += kCorrLanes) {
    const float2 x = y[0][k];
#pragma unroll
    for (int q = 1; q < kQ; q++) {
      float2 w = tw[(((kCorrLanes * q) % kNzc) * k) % kNzc];
      w.y      = -w.y;
      y[q][k]  = cmul(x, w);
    }
  }
  __syncthreads();
  // corr_spec <- unnormalised backward DFT: out[n] = sum_k y_q[k] e^{+j 2 pi lane k / 839}, n = lane + 256 q
  float2 acc[kQ];
#pragma unroll
  for (int q = 0; q < kQ; q++) {
    acc[q] = make_float2(0.f, 0.f);
  }
  // summed in chunks of kChunk terms: at a peak the terms add coherently, and a running float sum over all 839 would round at the size of the peak 839 times
  int idx = 0; // (lane k) mod 839
  for (int k1 = 0; k1 < kNzc; k1 += kChunk) {
    float2 part[kQ];
#pragma unroll
    for (int q = 0; q < kQ; q++) {
      part[q] = make_float2(0.f, 0.f);
    }
    const int ke = k1 + kChunk < kNzc ? k1 + kChunk : kNzc;
    for (int k = k1; k < ke; k++) {
      const float2 w  = tw[idx];
      const float  wc = w.x, ws = -w.y;
#pragma unroll
      for (int q = 0; q < kQ; q++) {
        const float2 x = y[q][k];
        part[q].x += x.x * wc - x.y * ws;
        part[q].y += x.x * ws + x.y * wc;
      }
      idx += tid;
      idx -= idx >= kNzc ? kNzc : 0;
    }
#pragma unroll
    for (int q = 0; q < kQ; q++) {
      acc[q] = cadd(acc[q], part[q]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < kQ; q++) {
    const int n = tid + kCorrLanes * q;
    if (n < kNzc) {
      const float v = acc[q].x * acc[q].x + acc[q].y * acc[q].y;
      corr[n]       = v;
      sum += v;
      if (p.corr_out) {
        p.corr_out[((size_t)occ * p.n_search + r) * kNzc + n] = v;
      }
    }
  }
  sum = block_sum(sum, reinterpret_cast<float*>(red), [](float a, float b) { return a + b; }); // its first barrier publishes corr[]
  if (tid == 0) {
    rec[0] = __float_as_uint(sum / (float)kNzc);
    rec[1] = __float_as_uint(cr.x);
    rec[2] = __float_as_uint(cr.y);
    rec[3] = 0;
  }
  // the windows: one wave each, maximum and its first position, strict > from a peak of 0
  const int lane = tid & 63, wsz = p.N_cs ? p.N_cs : kNzc;
  for (int j = tid >> 6; j < p.n_wins; j += kCorrLanes / 64) {
    const int start = (kNzc - j * p.N_cs) % kNzc;
    float     best  = 0.f;
    int       at    = 0;
    for (int t = lane; t < wsz; t += 64) {
      const float v = corr[start + t];
      if (v > best) {
        best = v;
        at   = t;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int   oa = __shfl_xor(at, o);
      if (ob > best || (ob == best && oa < at)) {
        best = ob;
        at   = oa;
      }
    }
    if (lane == 0) {
      rec[kRecHead + j]            = __float_as_uint(best);
      rec[kRecHead + p.n_wins + j] = (uint32_t)at;
    }
  }
}

hipError_t launch(const Params& p, hipStream_t stream)
{
  hipLaunchKernelGGL(prach_stream_fft_kernel, dim3(p.D, p.n_occ), dim3(kStreamLanes), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    return e;
  }
  hipLaunchKernelGGL(prach_corr_kernel, dim3(p.n_search, p.n_occ), dim3(kCorrLanes), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_root_spectra(const float2* seq, float2* spec, int n_roots, hipStream_t stream)
{
  hipLaunchKernelGGL(prach_root_spec_kernel, dim3(n_roots), dim3(kCorrLanes), 0, stream, seq, spec);
  return hipGetLastError();
}

} // namespace prach
} // namespace phyhip
