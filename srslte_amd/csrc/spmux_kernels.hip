// spmux_kernels.hip -- PDSCH spatial multiplexing and large-delay CDD on 2 ports with 2 receive antennas (TM3 / TM4; TS 36.211 6.3.4.2) (gfx950).
//
// Reference behaviour, receive: srsran_predecoding_type with SRSRAN_TXSCHEME_CDD / _SPATIALMUX (lib/src/phy/mimo/precoding.c:841-1858: the precoder applied to
// the channel estimates, then a 2x2 zero-forcing or MMSE solve, or maximum-ratio combining for one layer) -> per codeword srsran_demod_soft_demodulate_{s,b}
// -> srsran_sequence_pdsch_apply_{s,c}, as srsran_pdsch_decode chains them (pdsch.c:880-899, 693-744): one pass over six planes, then two passes per
// codeword.  spmux_front_kernel is ONE pass for both codewords: it reads the six planes once and writes Qm soft bits per RE and codeword; the equalised
// symbols live in registers only.  Transmit: per codeword srsran_mod_modulate_bytes behind the packed scrambler -> srsran_precoding_type (:2044-2203):
// spmux_mod_kernel is the modulator of both codewords whose store is the precoder, writing both port planes and no intermediate d.
// The per-stage kernels behind srsran_hip_predecoding_mimo / srsran_hip_precoding_mimo come first; all four kernels call mimo_equalise / mimo_precode of
// modem_arith.h, so the fused kernels and the per-stage ones agree bit for bit (their operations carry
// `#pragma clang fp contract(off)`: nothing contracts, whatever the file's flags).
//
// Launch shape of the two fused kernels: that of txdiv_front_kernel / txdiv_mod_kernel on 2 ports.  One workgroup of 256 lanes = one tile of 2048 REs, 512
// consecutive ones per wave; a lane owns RE pairs (pair l, l + 64, l + 128, l + 192 of the wave's 256): one float4 per plane and pair, so every load
// instruction of a wave covers one contiguous 1 KB, and all of a lane's loads (6 planes x 4 pairs = 24 float4) are issued before the first is used.  A pair
// starts at an even RE: the parity CDD alternates its precoder with is the position inside the pair.  Each wave makes the chips of both codewords (its own
// <= 4096 of each, one LDS strip per codeword) while its loads are in flight.  A lane's two symbols of a codeword are adjacent in it: their soft bits leave
// as one vector store into that codeword's e-bit image.  An odd grant (spatial multiplexing only) ends in half a pair: its lane loads the whole pair (the
// planes of the staging image are padded) and stores one symbol's bits.
#include "hip_common.h"
#include "modem_arith.h"
#include "spmux_device.h"

namespace phyhip {
namespace spmux {

using namespace modem;

namespace {

constexpr int PAIRS = MODEM_TILE_SYMS / 4 / 2 / 64; // RE pairs a lane owns: 4

__device__ __forceinline__ float2 point_at(const float* plane, size_t i)
{
  return make_float2(plane[2 * i], plane[2 * i + 1]);
}
__device__ __forceinline__ void point_to(float* plane, size_t i, float2 v)
{
  plane[2 * i]     = v.x;
  plane[2 * i + 1] = v.y;
}

// ---- srsran_hip_predecoding_mimo on device planes: one lane per RE
__global__ __launch_bounds__(256) void spmux_eq_kernel(const EqParams p)
{
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) {
    return;
  }
  float2 x0, x1 = make_float2(0.f, 0.f);
  float  c0, c1 = 0.f;
  const float noise = p.s.dev_noise.v ? modem::noise_avg(p.s.dev_noise) : p.s.noise; // (uniform)
  mimo_equalise(p.s.layers, p.s.pre[i & 1u], p.s.mmse != 0, point_at(p.y[0], i), point_at(p.y[1], i), point_at(p.h[0][0], i), point_at(p.h[1][0], i),
                point_at(p.h[0][1], i), point_at(p.h[1][1], i), p.s.norm, noise, x0, x1, c0, c1);
  point_to(p.x[0], i, x0);
  if (p.csi[0]) {
    p.csi[0][i] = c0;
  }
  if (p.s.layers == 2) {
    point_to(p.x[1], i, x1);
    if (p.csi[1]) {
      p.csi[1][i] = c1;
    }
  }
}

// ---- srsran_hip_precoding_mimo on device planes: one lane per RE
__global__ __launch_bounds__(256) void spmux_precode_kernel(const PrecodeParams p)
{
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) {
    return;
  }
  const uint32_t kind = p.kind[i & 1u];
  const float2   x0   = point_at(p.x[0], i);
  const float2   x1   = kind < TXPRE_MUX1 ? point_at(p.x[1], i) : x0;
  float2         y0, y1;
  mimo_precode(kind, x0, x1, p.scale, y0, y1);
  point_to(p.y[0], i, y0);
  point_to(p.y[1], i, y1);
}

// ---- receive front end.  One codeword's symbols of the lane's pairs (x[r][0 / 1]: the pair's even / odd RE) -> soft bits, descrambled; one store per pair
template <typename T, int MOD>
__device__ __forceinline__ void codeword_bits(const FrontParams& p, const float2 (&x)[PAIRS][2], T* out, uint32_t w0, const uint32_t* cbw)
{
  constexpr int  QM   = MOD == 0 ? 1 : 2 * MOD;
  const bool     al   = (((uintptr_t)out) & 15u) == 0;
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int r = 0; r < PAIRS; r++) {
    const uint32_t ls = 2 * (r * 64u + lane), s = w0 + ls; // first of the pair's two symbols: in the wave, in the codeword
    if (s >= p.n) {
      continue;
    }
    int iv[2 * QM];
    demod_int<T, MOD>(x[r][0].x, x[r][0].y, s, p.n, p.k, iv);
    demod_int<T, MOD>(x[r][1].x, x[r][1].y, s + 1, p.n, p.k, iv + QM); // (of an odd grant's last pair: computed from the padding, not stored)
    const uint32_t c = chips_at(cbw, ls * QM);
    T              v[2 * QM];
#pragma unroll
    for (int i = 0; i < 2 * QM; i++) {
      v[i] = flip<T>((T)iv[i], (c >> i) & 1u);
    }
    if (s + 1 < p.n) {
      store_bits<T, 2 * QM>(out + (size_t)s * QM, v, al);
    } else {
      store_bits<T, QM>(out + (size_t)s * QM, v, al);
    }
  }
}

// the wave's chips of one codeword: REs w0 .. w0 + 511 of n, Qm chips each
__device__ __forceinline__ void codeword_chips(const uint32_t* x1_bits, const uint32_t* x2_cols, uint32_t seed, uint32_t mod, uint32_t w0, uint32_t n, uint32_t* cbw)
{
  const uint32_t qm = mod == 0 ? 1u : 2u * mod;
  make_chips(x1_bits, x2_cols, seed, w0 * qm, min((MODEM_TILE_SYMS / 4) * qm, (n - w0) * qm), cbw);
}

template <typename T>
__device__ __forceinline__ void codeword_bits_of(const FrontParams& p, uint32_t cw, const float2 (&x)[PAIRS][2], uint32_t w0, const uint32_t* cbw)
{
  T* out = (T*)p.out[cw];
  switch (p.mod[cw]) {
    case 0:
      codeword_bits<T, 0>(p, x, out, w0, cbw);
      break;
    case 1:
      codeword_bits<T, 1>(p, x, out, w0, cbw);
      break;
    case 2:
      codeword_bits<T, 2>(p, x, out, w0, cbw);
      break;
    case 3:
      codeword_bits<T, 3>(p, x, out, w0, cbw);
      break;
    default:
      codeword_bits<T, 4>(p, x, out, w0, cbw);
      break;
  }
}

// CSI: the equaliser's channel-state values (what spmux_eq_kernel files; a two-layer zero-forcing solve: 1.0 in both rows) go to p.csi[layer], one float
// per RE, for the weighting behind (csi_kernels.hip); the plain calls run the instantiations without
template <typename T, bool CSI>
__global__ __launch_bounds__(256) void spmux_front_kernel(const FrontParams p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][2][MODEM_TILE_BITS / 128 + 4]; // [wave][codeword]
  if ((threadIdx.x & 63u) < 2) {
    cb[threadIdx.x >> 6][threadIdx.x & 1u][MODEM_TILE_BITS / 128] = 0; // chips_at reads one word past the last one
  }
  __syncthreads();
  uint32_t(*cbw)[MODEM_TILE_BITS / 128 + 4] = cb[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = blockIdx.x * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4); // first RE of this wave
  if (w0 >= p.n) {
    return;
  }
  // a lane past the end of the grant loads the grant's last pair (in bounds) and stores nothing
  const uint32_t last = (p.n + 1) / 2 - 1;
  float4         y0[PAIRS], y1[PAIRS], a0[PAIRS], b0[PAIRS], a1[PAIRS], b1[PAIRS];
#pragma unroll
  for (int r = 0; r < PAIRS; r++) {
    const uint32_t i = min(w0 / 2 + r * 64u + lane, last);
    y0[r]            = p.y[0][i];
    y1[r]            = p.y[1][i];
    a0[r]            = p.h[0][0][i];
    b0[r]            = p.h[1][0][i];
    a1[r]            = p.h[0][1][i];
    b1[r]            = p.h[1][1][i];
  }
  // (the loads are in flight while the first lanes run the shift registers; the conditions are wave-uniform)
  const bool want0 = p.out[0] != nullptr, want1 = p.s.layers == 2 && p.out[1] != nullptr;
  if (want0) {
    codeword_chips(p.x1_bits, p.x2_cols, p.seed[0], p.mod[0], w0, p.n, cbw[0]);
  }
  if (want1) {
    codeword_chips(p.x1_bits, p.x2_cols, p.seed[1], p.mod[1], w0, p.n, cbw[1]);
  }
  float2 x0[PAIRS][2], x1[PAIRS][2];
  const float noise = p.s.dev_noise.v ? modem::noise_avg(p.s.dev_noise) : p.s.noise; // (uniform)
#pragma unroll
  for (int r = 0; r < PAIRS; r++) {
    float c0[2], c1[2] = {0.f, 0.f};
    x1[r][0] = x1[r][1] = make_float2(0.f, 0.f);
    mimo_equalise(p.s.layers, p.s.pre[0], p.s.mmse != 0, lo(y0[r]), lo(y1[r]), lo(a0[r]), lo(b0[r]), lo(a1[r]), lo(b1[r]), p.s.norm, noise, x0[r][0], x1[r][0], c0[0], c1[0]);
    mimo_equalise(p.s.layers, p.s.pre[1], p.s.mmse != 0, hi(y0[r]), hi(y1[r]), hi(a0[r]), hi(b0[r]), hi(a1[r]), hi(b1[r]), p.s.norm, noise, x0[r][1], x1[r][1], c0[1], c1[1]);
    if (CSI) {
      const uint32_t s = w0 + 2 * (r * 64u + lane); // the pair's even RE
      if (s + 1 < p.n) {
        *(float2*)(p.csi[0] + s) = make_float2(c0[0], c0[1]);
        if (p.s.layers == 2) {
          *(float2*)(p.csi[1] + s) = make_float2(c1[0], c1[1]);
        }
      } else if (s < p.n) {
        p.csi[0][s] = c0[0];
        if (p.s.layers == 2) {
          p.csi[1][s] = c1[0];
        }
      }
    }
  }
  // the codewords one after the other: their modulations may differ
  if (want0) {
    codeword_bits_of<T>(p, 0, x0, w0, cbw[0]);
  }
  if (want1) {
    codeword_bits_of<T>(p, 1, x1, w0, cbw[1]);
  }
}

// ---- transmit: one codeword's constellation points of the lane's pairs, scrambled
template <int MOD>
__device__ __forceinline__ void codeword_points(const ModParams& p, const ModJob& job, uint32_t cw, uint32_t w0, const uint32_t* cbw, float2 (&d)[PAIRS][2])
{
  constexpr int  QM     = MOD == 0 ? 1 : 2 * MOD;
  const uint32_t lane   = threadIdx.x & 63u;
  const uint8_t* bits   = p.bits + job.bits_off[cw];
  const float2*  tab    = p.table + mod_table_offset(MOD);
  const uint32_t nbytes = (job.n * QM + 7) / 8;
#pragma unroll
  for (int r = 0; r < PAIRS; r++) {
    const uint32_t ls = 2 * (r * 64u + lane), s = w0 + ls;
    d[r][0] = d[r][1] = make_float2(0.f, 0.f);
    if (s < job.n) {
      d[r][0] = mod_point<MOD>(bits, nbytes, tab, s, ls, cbw);
    }
    if (s + 1 < job.n) {
      d[r][1] = mod_point<MOD>(bits, nbytes, tab, s + 1, ls + 1, cbw);
    }
  }
}

__device__ __forceinline__ void codeword_points_of(const ModParams& p, const ModJob& job, uint32_t cw, uint32_t w0, uint32_t* cbw, float2 (&d)[PAIRS][2])
{
  codeword_chips(p.x1_bits, p.x2_cols, job.seed[cw], job.mod[cw], w0, job.n, cbw);
  switch (job.mod[cw]) {
    case 0:
      codeword_points<0>(p, job, cw, w0, cbw, d);
      break;
    case 1:
      codeword_points<1>(p, job, cw, w0, cbw, d);
      break;
    case 2:
      codeword_points<2>(p, job, cw, w0, cbw, d);
      break;
    case 3:
      codeword_points<3>(p, job, cw, w0, cbw, d);
      break;
    default:
      codeword_points<4>(p, job, cw, w0, cbw, d);
      break;
  }
}

__global__ __launch_bounds__(256) void spmux_mod_kernel(const ModParams p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][2][MODEM_TILE_BITS / 128 + 4]; // [wave][codeword]
  __shared__ ModJob sjob;
  if (threadIdx.x < sizeof(ModJob) / 4) {
    ((uint32_t*)&sjob)[threadIdx.x] = ((const uint32_t*)(p.jobs + p.tile_job[blockIdx.x]))[threadIdx.x];
  }
  if ((threadIdx.x & 63u) < 2) {
    cb[threadIdx.x >> 6][threadIdx.x & 1u][MODEM_TILE_BITS / 128] = 0;
  }
  __syncthreads();
  const ModJob job = sjob;
  uint32_t(*cbw)[MODEM_TILE_BITS / 128 + 4] = cb[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = (blockIdx.x - job.tile0) * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4);
  if (w0 >= job.n) {
    return;
  }
  float2 d0[PAIRS][2], d1[PAIRS][2];
  codeword_points_of(p, job, 0, w0, cbw[0], d0);
  if (job.layers == 2) {
    codeword_points_of(p, job, 1, w0, cbw[1], d1);
  }
  float2* y0 = p.out + job.out_off[0];
  float2* y1 = p.out + job.out_off[1];
#pragma unroll
  for (int r = 0; r < PAIRS; r++) {
    const uint32_t s = w0 + 2 * (r * 64u + lane);
    if (s >= job.n) {
      continue;
    }
    const float2 e0 = job.layers == 2 ? d1[r][0] : d0[r][0], e1 = job.layers == 2 ? d1[r][1] : d0[r][1];
    float2       p0a, p1a, p0b, p1b; // port 0 / 1 on the pair's even (a) and odd (b) RE
    mimo_precode(job.kind[0], d0[r][0], e0, job.scale, p0a, p1a);
    mimo_precode(job.kind[1], d0[r][1], e1, job.scale, p0b, p1b);
    if (s + 1 < job.n) {
      *(float4*)(y0 + s) = make_float4(p0a.x, p0a.y, p0b.x, p0b.y);
      *(float4*)(y1 + s) = make_float4(p1a.x, p1a.y, p1b.x, p1b.y);
    } else {
      y0[s] = p0a;
      y1[s] = p1a;
    }
  }
}

bool scheme_ok(const Scheme& s)
{
  return (s.layers == 2 && s.pre[0] <= HEFF_MP && s.pre[1] <= HEFF_MP) || (s.layers == 1 && s.pre[0] <= PRE_MINUS_J && s.pre[1] == s.pre[0]);
}

bool kind_ok(uint32_t layers, const uint32_t kind[2])
{
  return layers == 2 ? kind[0] < TXPRE_MUX1 && kind[1] < TXPRE_MUX1 : kind[0] >= TXPRE_MUX1 && kind[0] <= TXPRE_MUX1 + 3 && kind[1] == kind[0];
}

} // namespace

hipError_t launch_eq(const EqParams& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if (!scheme_ok(p.s) || !p.y[0] || !p.y[1] || !p.h[0][0] || !p.h[0][1] || !p.h[1][0] || !p.h[1][1] || !p.x[0] || (p.s.layers == 2 && !p.x[1])) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(spmux_eq_kernel, dim3(ceil_div(p.n, 256u)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_precode(const PrecodeParams& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  const bool two = p.kind[0] < TXPRE_MUX1;
  if (!kind_ok(two ? 2 : 1, p.kind) || !p.x[0] || (two && !p.x[1]) || !p.y[0] || !p.y[1]) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(spmux_precode_kernel, dim3(ceil_div(p.n, 256u)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_front(const FrontParams& p, bool llr8, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if (!scheme_ok(p.s) || !p.y[0] || !p.y[1] || !p.h[0][0] || !p.h[0][1] || !p.h[1][0] || !p.h[1][1] || p.mod[0] > 4 || p.mod[1] > 4 || !p.x1_bits || !p.x2_cols) {
    return hipErrorInvalidValue;
  }
  const dim3 grid(ceil_div(p.n, MODEM_TILE_SYMS));
  const bool csi = p.csi[0] != nullptr;
  if (csi && ((((uintptr_t)p.csi[0]) & 7u) || (p.s.layers == 2 && (!p.csi[1] || (((uintptr_t)p.csi[1]) & 7u))))) {
    return hipErrorInvalidValue;
  }
  if (llr8) {
    if (csi) {
      hipLaunchKernelGGL((spmux_front_kernel<int8_t, true>), grid, dim3(256), 0, stream, p);
    } else {
      hipLaunchKernelGGL((spmux_front_kernel<int8_t, false>), grid, dim3(256), 0, stream, p);
    }
  } else if (csi) {
    hipLaunchKernelGGL((spmux_front_kernel<int16_t, true>), grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL((spmux_front_kernel<int16_t, false>), grid, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

hipError_t launch_mod(const ModParams& p, hipStream_t stream)
{
  if (p.n_tiles == 0 || !p.bits || !p.out || !p.table || !p.jobs || !p.tile_job) {
    return p.n_tiles ? hipErrorInvalidValue : hipSuccess;
  }
  hipLaunchKernelGGL(spmux_mod_kernel, dim3(p.n_tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

} // namespace spmux
} // namespace phyhip
