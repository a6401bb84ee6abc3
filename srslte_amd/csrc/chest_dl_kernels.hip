// chest_dl_kernels.hip -- the downlink channel estimator, srsran_chest_dl_estimate_cfg (chest_dl.c:1004) for SRSRAN_SF_NORM subframes, AS WRITTEN, for the
// (rx antenna, port) pairs of a call in ONE launch: one workgroup of four waves per pair.  In order (a barrier between each):
//   1  gather the port's CRS REs (srsran_refsignal_cs_get_sf) and multiply by the conjugate of the caller's pilot row -> pe in LDS; the lane's share of
//      sum |rx|^2 (RSRP), sum pe (rsrp_corr) and of |x|^2 over the whole rows of the CRS symbols (chest_dl_rssi)
//   2  the lane's share of the CFO phasor sum (chest_estimate_cfo: rows 0, 1 against rows 2, 3) and of estimate_noise_pilots -- the LAST symbol only: the
//      reference assigns sum_power per symbol and returns the last.  Reduction of the seven sums in a fixed order: xor butterfly across the wave, the four
//      waves through LDS, lane 0 adds them 0 .. 3, finishes the REFS estimate and, with automatic Gauss taps, makes the taps from it (or from the state's)
//   3  smoothing (average_pilots): AVERAGE first adds and interleaves the rows into one row of 4 nof_prb (by cs_fidx(port, 0) < 3) and scales by 2 / nsymbols;
//      srsran_conv_same_cf with its uneven end rule, any length 0 .. 9 (0 taps: zeros, as the reference's loops give)
//   4  srsran_interp_linear_offset: AVERAGE one row with M = 3 and offset id % 3 (for every port; with no filter the source is the first 4 nof_prb RAW
//      estimates, rows 0 and 1 end to end); INTERPOLATE each CRS symbol's row with M = 6 and the symbol's cs_fidx
//   5  a lane per column: AVERAGE stores the row to every symbol; INTERPOLATE runs the reference's per-port, per-CP schedule of srsran_interp_linear_vector{,2}
//      as chains of additions (all indices compile-time: the column stays in registers) and stores the column.  The value at the PSS symbol goes to LDS
//   6  wave 0: estimate_noise_pss (62 points, from the finished ce row and the grid) or estimate_noise_empty_sc (4 x 5 points); lane 0 stores the record
// No atomics: a run gives the same bits every time.  LDS: pe and the smoothed rows (2 x 880 points), four frequency-interpolated rows (4 x 1320), 62 points
// of ce at the PSS: 57 KB static.
#include "chest_dl_device.h"

namespace phyhip {
namespace chest_dl {
namespace {

#define CHEST_DL_LANES 256u
#define CHEST_DL_SUMS 7u // |rx|^2, rssi, acc re / im, cfo re / im, REFS noise
#define CHEST_DL_MAX_REF (8u * CHEST_DL_MAX_PRB)
#define CHEST_DL_MAX_NRE (12u * CHEST_DL_MAX_PRB)

__device__ __forceinline__ float2 cmul_conj(float2 a, float2 b) // a conj(b)
{
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b)
{
  return make_float2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ float2 csub(float2 a, float2 b)
{
  return make_float2(a.x - b.x, a.y - b.y);
}
__device__ __forceinline__ float2 cscale(float2 a, float f)
{
  return make_float2(a.x * f, a.y * f);
}
__device__ __forceinline__ float norm2(float2 a)
{
  return a.x * a.x + a.y * a.y;
}

// output i of srsran_conv_same_cf (convolution.c:181-218) over x[0 .. N), N >= 12 > M: every index read lies in [0, N)
__device__ float2 conv_at(const float2* x, uint32_t N, const float* f, uint32_t M, uint32_t i)
{
  const uint32_t h = M / 2;
  float2         acc = make_float2(0.f, 0.f);
  for (uint32_t t = 0; t < M; t++) {
    float2 v;
    if (i < h) { // first[i + t]
      const uint32_t q = i + t;
      v = q < h ? csub(cscale(x[1], (float)(2 + h - q)), cscale(x[0], (float)(1 + h - q))) : x[q - h];
    } else if (i < N - h) {
      v = x[i - h + t];
    } else { // last[(i - (N - h)) + t]
      const uint32_t q = i - (N - h) + t;
      v = q >= M - 1 ? csub(cscale(x[N - 1], (float)(2 + q - h)), cscale(x[N - 2], (float)(1 + q - h))) : x[N - M + q + 1];
    }
    acc.x += v.x * f[t];
    acc.y += v.y * f[t];
  }
  return acc;
}

// output o of srsran_interp_linear_offset (interp.c:258-284) over x[0 .. L) with ratio M, off_st < M points in front and M - off_st behind: o < L M
__device__ float2 interp_at(const float2* x, uint32_t L, uint32_t M, uint32_t off_st, uint32_t o)
{
  const float fm = (float)M;
  if (o < off_st) {
    const float  w = (float)(off_st - o); // j + 1 with o = off_st - j - 1
    const float2 d = csub(x[1], x[0]);
    return make_float2(x[0].x - (w * d.x) / fm, x[0].y - (w * d.y) / fm);
  }
  o -= off_st;
  const uint32_t i = min(o / M, L - 1), jj = o - i * M;
  if (i < L - 1) {
    const float2 d = cscale(csub(x[i + 1], x[i]), 1.0f / fm);
    return make_float2(x[i].x + d.x * (float)jj, x[i].y + d.y * (float)jj);
  }
  const float2 d = csub(x[L - 1], x[L - 2]);
  return make_float2(x[L - 1].x + ((float)jj * d.x) / fm, x[L - 1].y + ((float)jj * d.y) / fm);
}

// srsran_interp_linear_vector3 to the right (interp.c:158-188): `between` and the M - 1 rows behind it <- start + k (in1 - in0) (1 / d), one addition per row
#define CHEST_DL_CHAIN(in0, in1, start, between, d, M)                      \
  {                                                                         \
    const float2 step = cscale(csub(c[in1], c[in0]), (float)1 / (float)(d)); \
    float2       prev = c[start];                                           \
    _Pragma("unroll") for (int q = 0; q < (M); q++)                         \
    {                                                                       \
      prev             = cadd(prev, step);                                  \
      c[(between) + q] = prev;                                              \
    }                                                                       \
  }

// one column of interpolate_pilots' time interpolation (chest_dl.c:524-553): the CRS symbols' values from the frequency-interpolated rows, the schedule,
// the stores; returns the value at symbol NSYMB - 1 (the PSS)
template <int NSYMB, bool LOW>
__device__ __forceinline__ float2 time_column(const float2* fr, uint32_t nre, uint32_t k, float2* ce)
{
  float2 c[2 * NSYMB];
  if constexpr (LOW) { // ports 0, 1
    c[0]             = fr[k];
    c[NSYMB - 3]     = fr[nre + k];
    c[NSYMB]         = fr[2 * nre + k];
    c[2 * NSYMB - 3] = fr[3 * nre + k];
    if constexpr (NSYMB == 7) {
      CHEST_DL_CHAIN(0, 4, 0, 1, 4, 3)
      CHEST_DL_CHAIN(4, 7, 4, 5, 3, 2)
      CHEST_DL_CHAIN(7, 11, 7, 8, 4, 3)
      CHEST_DL_CHAIN(7, 11, 11, 12, 4, 2)
    } else {
      CHEST_DL_CHAIN(0, 3, 0, 1, 3, 2)
      CHEST_DL_CHAIN(3, 6, 3, 4, 3, 2)
      CHEST_DL_CHAIN(6, 9, 6, 7, 3, 2)
      CHEST_DL_CHAIN(6, 9, 9, 10, 3, 2)
    }
  } else { // ports 2, 3: the rows behind the second CRS symbol start at the FIRST one, as the reference writes them
    c[1]         = fr[k];
    c[1 + NSYMB] = fr[nre + k];
    CHEST_DL_CHAIN(1 + NSYMB, 1, 1, 0, NSYMB, 1)
    CHEST_DL_CHAIN(1, 1 + NSYMB, 1, 2, NSYMB, NSYMB - 1)
    CHEST_DL_CHAIN(1, 1 + NSYMB, 1, 2 + NSYMB, NSYMB, NSYMB - 2)
  }
  if (ce) {
#pragma unroll
    for (int l = 0; l < 2 * NSYMB; l++) {
      ce[(size_t)l * nre + k] = c[l];
    }
  }
  return c[NSYMB - 1];
}

__global__ __launch_bounds__(CHEST_DL_LANES) void chest_dl_kernel(const Params p)
{
  __shared__ float2   pe[CHEST_DL_MAX_REF], av[CHEST_DL_MAX_REF], fr[4 * CHEST_DL_MAX_NRE], pss_ce[CHEST_DL_PSS_LEN];
  __shared__ float    part[CHEST_DL_LANES / 64][CHEST_DL_SUMS];
  __shared__ float    fil[CHEST_DL_MAX_TAPS];
  __shared__ uint32_t fil_len;
  if (blockIdx.x >= p.n_jobs) {
    return;
  }
  const Job      j = p.jobs[blockIdx.x];
  const uint32_t tid = threadIdx.x, prb = j.nof_prb, nsymb = j.cp_nsymb, port = j.port;
  bool           ok = prb >= 6 && prb <= CHEST_DL_MAX_PRB && (nsymb == 6 || nsymb == 7) && (j.nof_ports == 1 || j.nof_ports == 2 || j.nof_ports == 4) &&
            port < j.nof_ports && j.cell_id <= 503 && j.filter <= FILTER_AUTO && j.n_taps <= CHEST_DL_MAX_TAPS && j.late <= LATE_EMPTY;
  const uint32_t nre = 12 * prb, nref = 2 * prb, nsym = nof_symbols(port);
  const uint64_t grid_points = (uint64_t)2 * nsymb * nre;
  ok = ok && (uint64_t)j.o_grid + grid_points <= p.in_points && (uint64_t)j.o_pilots + nsym * nref <= p.in_points &&
       (j.late != LATE_PSS || (uint64_t)j.o_pss + CHEST_DL_PSS_LEN <= p.in_points) && (j.o_ce == CHEST_DL_NONE || (uint64_t)j.o_ce + grid_points <= p.out_points);
  if (!ok) { // (uniform over the workgroup: in front of every barrier)
    if (tid == 0) {
      p.rec[blockIdx.x] = Record{NAN, NAN, {NAN, NAN}, {NAN, NAN}, NAN, NAN, NAN};
      if (p.noise_dev) {
        p.noise_dev[blockIdx.x] = NAN;
      }
    }
    return;
  }
  const float2* grid   = p.in + j.o_grid;
  const float2* pilots = p.in + j.o_pilots;
  float2*       ce     = j.o_ce == CHEST_DL_NONE ? nullptr : p.out + j.o_ce;
  float         s[CHEST_DL_SUMS];
#pragma unroll
  for (uint32_t q = 0; q < CHEST_DL_SUMS; q++) {
    s[q] = 0.f;
  }
  // 1: least-squares estimates; 6 k + fidx <= 12 nof_prb - 1 and the symbol < 2 cp_nsymb: inside the grid
  for (uint32_t i = tid; i < nsym * nref; i += CHEST_DL_LANES) {
    const uint32_t l = i / nref, k = i - l * nref;
    const float2   x = grid[(size_t)cs_nsymbol(l, nsymb, port) * nre + cs_fidx(j.cell_id, l, port) + 6 * k];
    const float2   e = cmul_conj(x, pilots[i]);
    pe[i]            = e;
    s[0] += norm2(x);
    s[2] += e.x;
    s[3] += e.y;
  }
  for (uint32_t i = tid; i < nsym * nre; i += CHEST_DL_LANES) {
    const uint32_t l = i / nre, k = i - l * nre;
    s[1] += norm2(grid[(size_t)cs_nsymbol(l, nsymb, port) * nre + k]);
  }
  __syncthreads();
  // 2: the CFO phasor (ports 0 and 1 have the four rows) and estimate_noise_pilots' last symbol (chest_dl.c:353-400 with i = nsymbols): X the last row, A the
  // one before, B the virtual row behind (2 row[2] - row[0] with four symbols, row[0] with two)
  if (nsym == 4) {
    for (uint32_t i = tid; i < 2 * nref; i += CHEST_DL_LANES) {
      const float2 t = cmul_conj(pe[i], pe[i + 2 * nref]);
      s[4] += t.x;
      s[5] += t.y;
    }
  }
  {
    const bool    shifted = cs_fidx(j.cell_id, 0, port) >= 3; // offset 1
    const float2* X = pe + (nsym - 1) * nref;
    const float2* A = pe + (nsym - 2) * nref;
    for (uint32_t k = tid; k < nref; k += CHEST_DL_LANES) {
      float2 t = X[k];
#pragma unroll
      for (int side = 0; side < 2; side++) {
        auto nb = [&](uint32_t q) { // q < nref
          if (side == 0) {
            return A[q];
          }
          return nsym == 4 ? csub(cscale(pe[2 * nref + q], 2.0f), pe[q]) : pe[q];
        };
        t = cadd(t, nb(k));
        if (shifted) {
          t = cadd(t, k >= 1 ? nb(k - 1) : csub(cscale(nb(0), 2.0f), nb(1)));
        } else {
          t = cadd(t, k + 1 < nref ? nb(k + 1) : csub(cscale(nb(nref - 2), 2.0f), nb(nref - 1)));
        }
      }
      s[6] += norm2(csub(X[k], cscale(t, 1.0f / 5.0f)));
    }
  }
#pragma unroll
  for (uint32_t q = 0; q < CHEST_DL_SUMS; q++) {
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
  float t[CHEST_DL_SUMS] = {}; // (lane 0's)
  float noise_refs = 0.f;
  if (tid == 0) {
#pragma unroll
    for (uint32_t q = 0; q < CHEST_DL_SUMS; q++) {
      t[q] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
    }
    noise_refs = t[6] / (float)nref / (float)nsym * sqrtf(5.0f);
    uint32_t len = 0;
    if (j.filter == FILTER_TAPS) {
      len = j.n_taps;
      for (uint32_t q = 0; q < len; q++) {
        fil[q] = p.jobs[blockIdx.x].taps[q]; // (not from the copy: a dynamic index would take it out of registers)
      }
    } else if (j.filter == FILTER_AUTO) { // chest_dl.c:707-708
      len = gauss_taps(fil, 4, (j.auto_refs ? noise_refs : j.state_noise) * 200.0f);
    }
    fil_len = len;
  }
  __syncthreads();
  // 3: average_pilots (chest_dl.c:558-601)
  const uint32_t flen = fil_len;
  if (j.filter != FILTER_OFF) { // (uniform)
    if (j.average) {
      const bool low = cs_fidx(j.cell_id, 0, port) < 3;
      float2*    tmp = fr; // (the frequency rows are not there yet)
      for (uint32_t i = tid; i < 2 * nref; i += CHEST_DL_LANES) {
        const uint32_t k = i >> 1, first = ((i & 1u) != 0) == low ? 1u : 0u;
        float2         v = pe[first * nref + k];
        if (nsym == 4) {
          v = cadd(v, pe[(first + 2) * nref + k]);
        }
        tmp[i] = cscale(v, 2.0f / (float)nsym);
      }
      __syncthreads();
      for (uint32_t i = tid; i < 2 * nref; i += CHEST_DL_LANES) {
        av[i] = conv_at(tmp, 2 * nref, fil, flen, i);
      }
    } else {
      for (uint32_t i = tid; i < nsym * nref; i += CHEST_DL_LANES) {
        const uint32_t l = i / nref;
        av[i]            = conv_at(pe + l * nref, nref, fil, flen, i - l * nref);
      }
    }
  }
  __syncthreads();
  // 4: frequency interpolation (chest_dl.c:458-509)
  const float2* src = j.filter == FILTER_OFF ? pe : av;
  if (j.average) {
    for (uint32_t o = tid; o < nre; o += CHEST_DL_LANES) {
      fr[o] = interp_at(src, 2 * nref, 3, j.cell_id % 3, o);
    }
  } else {
    for (uint32_t i = tid; i < nsym * nre; i += CHEST_DL_LANES) {
      const uint32_t l = i / nre;
      fr[i]            = interp_at(src + l * nref, nref, 6, cs_fidx(j.cell_id, l, port), i - l * nre);
    }
  }
  __syncthreads();
  // 5: time (chest_dl.c:512-555)
  const uint32_t k_pss = nre / 2 - 31;
  for (uint32_t k = tid; k < nre; k += CHEST_DL_LANES) {
    float2 at_pss;
    if (j.average) {
      at_pss = fr[k];
      for (uint32_t l = 0; ce && l < 2 * nsymb; l++) {
        ce[(size_t)l * nre + k] = at_pss;
      }
    } else if (nsymb == 7) {
      at_pss = port < 2 ? time_column<7, true>(fr, nre, k, ce) : time_column<7, false>(fr, nre, k, ce);
    } else {
      at_pss = port < 2 ? time_column<6, true>(fr, nre, k, ce) : time_column<6, false>(fr, nre, k, ce);
    }
    if (k >= k_pss && k < k_pss + CHEST_DL_PSS_LEN) {
      pss_ce[k - k_pss] = at_pss;
    }
  }
  __syncthreads();
  // 6: wave 0: the PSS / EMPTY noise estimate (chest_dl.c:403-434); the 5 sub-carriers on either side of the 62 lie inside the symbol's row (nre >= 72)
  if (tid < 64) {
    float v = 0.f;
    if (j.late == LATE_PSS && tid < CHEST_DL_PSS_LEN) {
      const float2 x = grid[(size_t)(nsymb - 1) * nre + k_pss + tid];
      v              = norm2(csub(cmul(pss_ce[tid], p.in[j.o_pss + tid]), x));
    } else if (j.late == LATE_EMPTY && tid < 20) {
      const uint32_t g = tid / 5, q = tid - 5 * g;
      const uint32_t at = (nsymb - 2 + g / 2) * nre + k_pss + ((g & 1u) ? CHEST_DL_PSS_LEN + q : q - 5u);
      v                 = norm2(grid[at]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v += __shfl_xor(v, off);
    }
    if (tid == 0) {
      float late = 0.f;
      if (j.late == LATE_PSS) {
        late = (float)((double)((float)j.nof_ports * (v / (float)CHEST_DL_PSS_LEN)) * M_SQRT1_2);
      } else if (j.late == LATE_EMPTY) {
        late = v / 5.0f;
      }
      const float out   = j.auto_refs ? noise_refs : j.late != LATE_NONE ? late : j.state_noise;
      p.rec[blockIdx.x] = Record{t[0], t[1], {t[2], t[3]}, {t[4], t[5]}, noise_refs, late, out};
      if (p.noise_dev) {
        p.noise_dev[blockIdx.x] = out;
      }
    }
  }
}

} // namespace

hipError_t launch(const Params& p, hipStream_t stream)
{
  if (p.n_jobs == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(chest_dl_kernel, dim3(p.n_jobs), dim3(CHEST_DL_LANES), 0, stream, p);
  return hipGetLastError();
}

} // namespace chest_dl
} // namespace phyhip
