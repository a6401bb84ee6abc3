// txdiv_kernels.hip -- PDSCH transmit diversity (SFBC, TS 36.211 6.3.3.3 / 6.3.4.3) on 2 and 4 ports (gfx950).
//
// Reference behaviour, receive: srsran_predecoding_diversity_csi (lib/src/phy/mimo/precoding.c:673-778) -> srsran_layerdemap_diversity
// (layermap.c:138-147) -> srsran_demod_soft_demodulate_{s,b} -> srsran_sequence_pdsch_apply_{s,c}, as srsran_pdsch_decode chains them (pdsch.c:880-899,
// 693-744): four passes over the grant, the first reading (1 + nof_ports) nof_rx planes.  txdiv_front_kernel is ONE pass: it reads the planes once and
// writes Qm soft bits per RE; the combined symbols live in registers only.  Transmit: srsran_mod_modulate_bytes behind the packed scrambler ->
// srsran_layermap_diversity (layermap.c:38-47) -> srsran_precoding_diversity (precoding.c:1943-1992): txdiv_mod_kernel is the modulator whose store is
// the layer map and the precoder, writing every port's plane (zeros on the idle ports of a 4-port pair included) and no intermediate d.
// The per-stage kernels behind the reference-named entry points (txdiv_eq_kernel, txdiv_precode_kernel, txdiv_layer_kernel) come first; the
// combining arithmetic of both receive kernels is sfbc_add / sfbc_finish of modem_arith.h, so their symbols agree bit for bit.
//
// Launch shape of the two fused kernels: that of modem_kernel (modem_kernels.hip).  One workgroup of 256 lanes = one tile of 2048 REs, 512 consecutive
// ones per wave, each wave making its own <= 4096 chips.  2 ports: a lane owns RE pairs (pair l, l + 64, ... of the wave's 256): one float4 per plane
// and pair, so every load instruction of a wave covers one contiguous 1 KB, and all of a lane's loads (3 planes x 4 pairs per receive antenna, 24 float4
// with two) are issued before the first is used.  4 ports: a lane owns RE quads (quad l, l + 64 of the wave's 128) and loads only the halves of the
// channel planes the formulas read: ports 0 / 2 at 4i, 4i + 1 and ports 1 / 3 at 4i + 2, 4i + 3 (2 + 4 float4 per quad and antenna, again 24).
// A lane's two (four) output symbols are adjacent in the codeword: their soft bits leave as one (two) vector stores.
#include "hip_common.h"
#include "modem_arith.h"
#include "txdiv_device.h"

namespace phyhip {
namespace txdiv {

using namespace modem;

namespace {

// ---- srsran_predecoding_diversity_multi on device planes: one lane per RE pair (2 ports) or quad (4 ports)
template <int PORTS>
__global__ __launch_bounds__(256) void txdiv_eq_kernel(const EqParams p)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (PORTS * i >= p.n) {
    return;
  }
  const float nrx = (float)p.nof_rx;
  if (PORTS == 2) {
    Sfbc a;
#pragma unroll
    for (int rx = 0; rx < 2; rx++) {
      if (rx == 0 || p.nof_rx == 2) {
        const float4 y = p.y[rx][i], h0 = p.h[0][rx][i], h1 = p.h[1][rx][i];
        sfbc_add<2>(a, lo(h0), hi(h1), lo(h1), hi(h0), lo(y), hi(y));
      }
    }
    float2 x0, x1, c;
    sfbc_finish<2>(a, p.scaling, nrx, x0, x1, c);
    p.x[0][(size_t)i * p.x_stride] = x0;
    p.x[1][(size_t)i * p.x_stride] = x1;
    if (p.csi) {
      ((float2*)p.csi)[i] = c;
    }
  } else {
    Sfbc a, b;
#pragma unroll
    for (int rx = 0; rx < 2; rx++) {
      if (rx == 0 || p.nof_rx == 2) {
        const float4 y0 = p.y[rx][2 * i], y1 = p.y[rx][2 * i + 1];
        const float4 h0 = p.h[0][rx][2 * i], h2 = p.h[2][rx][2 * i], h1 = p.h[1][rx][2 * i + 1], h3 = p.h[3][rx][2 * i + 1];
        sfbc_add<4>(a, lo(h0), hi(h2), lo(h2), hi(h0), lo(y0), hi(y0));
        sfbc_add<4>(b, lo(h1), hi(h3), lo(h3), hi(h1), lo(y1), hi(y1));
      }
    }
    float2 x0, x1, x2, x3, c0, c1;
    sfbc_finish<4>(a, p.scaling, nrx, x0, x1, c0);
    sfbc_finish<4>(b, p.scaling, nrx, x2, x3, c1);
    p.x[0][(size_t)i * p.x_stride] = x0;
    p.x[1][(size_t)i * p.x_stride] = x1;
    p.x[2][(size_t)i * p.x_stride] = x2;
    p.x[3][(size_t)i * p.x_stride] = x3;
    if (p.csi) {
      ((float4*)p.csi)[i] = make_float4(c0.x, c0.y, c1.x, c1.y);
    }
  }
}

// ---- srsran_precoding_diversity: one lane per layer symbol index i; every written component is ONE float product by p.scale (or a zero)
__device__ __forceinline__ float4 sfbc_tx_a(float2 d0, float2 d1, float s) // the pair on the first port of the pair: d0, d1
{
  return make_float4(__fmul_rn(d0.x, s), __fmul_rn(d0.y, s), __fmul_rn(d1.x, s), __fmul_rn(d1.y, s));
}
__device__ __forceinline__ float4 sfbc_tx_b(float2 d0, float2 d1, float s) // on the second: -conj(d1), conj(d0)
{
  return make_float4(__fmul_rn(-d1.x, s), __fmul_rn(d1.y, s), __fmul_rn(d0.x, s), __fmul_rn(-d0.y, s));
}

__global__ __launch_bounds__(256) void txdiv_precode_kernel(const PrecodeParams p)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) {
    return;
  }
  const float2 d0 = p.x[0][i], d1 = p.x[1][i];
  if (p.ports == 2) {
    ((float4*)p.y[0])[i] = sfbc_tx_a(d0, d1, p.scale);
    ((float4*)p.y[1])[i] = sfbc_tx_b(d0, d1, p.scale);
  } else {
    const float2 d2 = p.x[2][i], d3 = p.x[3][i];
    const float4 z  = make_float4(0.f, 0.f, 0.f, 0.f);
    ((float4*)p.y[0])[2 * i]     = sfbc_tx_a(d0, d1, p.scale);
    ((float4*)p.y[2])[2 * i]     = sfbc_tx_b(d0, d1, p.scale);
    ((float4*)p.y[1])[2 * i]     = z;
    ((float4*)p.y[3])[2 * i]     = z;
    ((float4*)p.y[0])[2 * i + 1] = z;
    ((float4*)p.y[2])[2 * i + 1] = z;
    ((float4*)p.y[1])[2 * i + 1] = sfbc_tx_a(d2, d3, p.scale);
    ((float4*)p.y[3])[2 * i + 1] = sfbc_tx_b(d2, d3, p.scale);
  }
}

// ---- srsran_layermap_diversity / srsran_layerdemap_diversity: one lane per codeword symbol
__global__ __launch_bounds__(256) void txdiv_layer_kernel(const LayerParams p)
{
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= p.n * p.layers) {
    return;
  }
  const uint32_t i = s / p.layers, j = s - i * p.layers;
  if (p.to_layers) {
    p.x[j][i] = p.d[s];
  } else {
    p.d[s] = p.x[j][i];
  }
}

// ---- receive front end.  The two symbols of one pair (s, s + 1 of the codeword; ls: s counted from the wave's first) -> soft bits, descrambled, one store
template <typename T, int MOD>
__device__ __forceinline__ void pair_bits(const FrontParams& p, float2 x0, float2 x1, uint32_t s, uint32_t ls, const uint32_t* cbw, T* out, bool al)
{
  constexpr int QM = MOD == 0 ? 1 : 2 * MOD;
  int           iv[2 * QM];
  demod_int<T, MOD>(x0.x, x0.y, s, p.n, p.k, iv);
  demod_int<T, MOD>(x1.x, x1.y, s + 1, p.n, p.k, iv + QM);
  const uint32_t c = chips_at(cbw, ls * QM);
  T              v[2 * QM];
#pragma unroll
  for (int i = 0; i < 2 * QM; i++) {
    v[i] = flip<T>((T)iv[i], (c >> i) & 1u);
  }
  store_bits<T, 2 * QM>(out + (size_t)s * QM, v, al);
}

template <typename T, int MOD, int PORTS, bool CSI>
__device__ __forceinline__ void front_tile(const FrontParams& p, uint32_t tile, uint32_t* cbw)
{
  constexpr int  QM   = MOD == 0 ? 1 : 2 * MOD;
  T*             out  = (T*)p.out;
  const bool     al   = (((uintptr_t)out) & 15u) == 0;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = tile * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4); // first RE of this wave
  if (w0 >= p.n) {
    return;
  }
  const bool  rx2 = p.nof_rx == 2; // wave-uniform
  const float nrx = (float)p.nof_rx;
  // a lane past the end of the grant loads the grant's last pair / quad (in bounds) and stores nothing
  if constexpr (PORTS == 2) {
    constexpr int  R     = MODEM_TILE_SYMS / 4 / 2 / 64;
    const uint32_t last  = p.n / 2 - 1;
    float4         y[2][R], h0[2][R], h1[2][R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t i = min(w0 / 2 + r * 64u + lane, last);
      y[0][r]          = p.y[0][i];
      h0[0][r]         = p.h[0][0][i];
      h1[0][r]         = p.h[1][0][i];
    }
    if (rx2) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t i = min(w0 / 2 + r * 64u + lane, last);
        y[1][r]          = p.y[1][i];
        h0[1][r]         = p.h[0][1][i];
        h1[1][r]         = p.h[1][1][i];
      }
    }
    // (the loads are in flight while the first lanes run the shift registers)
    make_chips(p.x1_bits, p.x2_cols, p.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (p.n - w0) * QM), cbw);
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t ls = 2 * (r * 64u + lane), s = w0 + ls; // first of the pair's two symbols: in the wave, in the codeword
      if (s >= p.n) {
        continue;
      }
      Sfbc a;
      sfbc_add<2>(a, lo(h0[0][r]), hi(h1[0][r]), lo(h1[0][r]), hi(h0[0][r]), lo(y[0][r]), hi(y[0][r]));
      if (rx2) {
        sfbc_add<2>(a, lo(h0[1][r]), hi(h1[1][r]), lo(h1[1][r]), hi(h0[1][r]), lo(y[1][r]), hi(y[1][r]));
      }
      float2 x0, x1, c;
      sfbc_finish<2>(a, p.scaling, nrx, x0, x1, c);
      if (CSI) {
        *(float2*)(p.csi + s) = c;
      }
      pair_bits<T, MOD>(p, x0, x1, s, ls, cbw, out, al);
    }
  } else {
    constexpr int  R    = MODEM_TILE_SYMS / 4 / 4 / 64;
    const uint32_t last = p.n / 4 - 1;
    float4         y0[2][R], y1[2][R], h0[2][R], h1[2][R], h2[2][R], h3[2][R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t i = min(w0 / 4 + r * 64u + lane, last);
      y0[0][r]         = p.y[0][2 * i];
      y1[0][r]         = p.y[0][2 * i + 1];
      h0[0][r]         = p.h[0][0][2 * i];
      h2[0][r]         = p.h[2][0][2 * i];
      h1[0][r]         = p.h[1][0][2 * i + 1];
      h3[0][r]         = p.h[3][0][2 * i + 1];
    }
    if (rx2) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t i = min(w0 / 4 + r * 64u + lane, last);
        y0[1][r]         = p.y[1][2 * i];
        y1[1][r]         = p.y[1][2 * i + 1];
        h0[1][r]         = p.h[0][1][2 * i];
        h2[1][r]         = p.h[2][1][2 * i];
        h1[1][r]         = p.h[1][1][2 * i + 1];
        h3[1][r]         = p.h[3][1][2 * i + 1];
      }
    }
    make_chips(p.x1_bits, p.x2_cols, p.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (p.n - w0) * QM), cbw);
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t ls = 4 * (r * 64u + lane), s = w0 + ls;
      if (s >= p.n) {
        continue;
      }
      Sfbc a, b;
      sfbc_add<4>(a, lo(h0[0][r]), hi(h2[0][r]), lo(h2[0][r]), hi(h0[0][r]), lo(y0[0][r]), hi(y0[0][r]));
      sfbc_add<4>(b, lo(h1[0][r]), hi(h3[0][r]), lo(h3[0][r]), hi(h1[0][r]), lo(y1[0][r]), hi(y1[0][r]));
      if (rx2) {
        sfbc_add<4>(a, lo(h0[1][r]), hi(h2[1][r]), lo(h2[1][r]), hi(h0[1][r]), lo(y0[1][r]), hi(y0[1][r]));
        sfbc_add<4>(b, lo(h1[1][r]), hi(h3[1][r]), lo(h3[1][r]), hi(h1[1][r]), lo(y1[1][r]), hi(y1[1][r]));
      }
      float2 x0, x1, x2, x3, c0, c1;
      sfbc_finish<4>(a, p.scaling, nrx, x0, x1, c0);
      sfbc_finish<4>(b, p.scaling, nrx, x2, x3, c1);
      if (CSI) {
        *(float4*)(p.csi + s) = make_float4(c0.x, c0.y, c1.x, c1.y);
      }
      pair_bits<T, MOD>(p, x0, x1, s, ls, cbw, out, al);
      pair_bits<T, MOD>(p, x2, x3, s + 2, ls + 2, cbw, out, al);
    }
  }
}

// CSI: the combiner's channel-state values (what txdiv_eq_kernel files) go to p.csi, one float per RE, for the weighting behind (csi_kernels.hip); the
// plain calls run the instantiations without
template <typename T, bool CSI>
__global__ __launch_bounds__(256) void txdiv_front_kernel(const FrontParams p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][MODEM_TILE_BITS / 128 + 4];
  if ((threadIdx.x & 63u) == 0) {
    cb[threadIdx.x >> 6][MODEM_TILE_BITS / 128] = 0; // chips_at reads one word past the last one
  }
  __syncthreads();
  uint32_t* cbw = cb[threadIdx.x >> 6];
  if (p.ports == 2) {
    switch (p.mod) {
      case 0:
        front_tile<T, 0, 2, CSI>(p, blockIdx.x, cbw);
        break;
      case 1:
        front_tile<T, 1, 2, CSI>(p, blockIdx.x, cbw);
        break;
      case 2:
        front_tile<T, 2, 2, CSI>(p, blockIdx.x, cbw);
        break;
      case 3:
        front_tile<T, 3, 2, CSI>(p, blockIdx.x, cbw);
        break;
      default:
        front_tile<T, 4, 2, CSI>(p, blockIdx.x, cbw);
        break;
    }
  } else {
    switch (p.mod) {
      case 0:
        front_tile<T, 0, 4, CSI>(p, blockIdx.x, cbw);
        break;
      case 1:
        front_tile<T, 1, 4, CSI>(p, blockIdx.x, cbw);
        break;
      case 2:
        front_tile<T, 2, 4, CSI>(p, blockIdx.x, cbw);
        break;
      case 3:
        front_tile<T, 3, 4, CSI>(p, blockIdx.x, cbw);
        break;
      default:
        front_tile<T, 4, 4, CSI>(p, blockIdx.x, cbw);
        break;
    }
  }
}

// ---- transmit: one tile (a symbol of the codeword as a constellation point: mod_point of modem_arith.h)
template <int MOD>
__device__ __forceinline__ void mod_tile(const ModParams& p, const ModJob& job, uint32_t tile, uint32_t* cbw)
{
  constexpr int  QM   = MOD == 0 ? 1 : 2 * MOD;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = tile * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4);
  if (w0 >= job.n) {
    return;
  }
  make_chips(p.x1_bits, p.x2_cols, job.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (job.n - w0) * QM), cbw);
  const uint8_t* bits   = p.bits + job.bits_off;
  const float2*  tab    = p.table + mod_table_offset(MOD);
  const uint32_t nbytes = (job.n * QM + 7) / 8;
  const float    sc     = job.scale;
  if (job.ports == 2) {
    float4* y0 = (float4*)(p.out + job.out_off[0]);
    float4* y1 = (float4*)(p.out + job.out_off[1]);
#pragma unroll
    for (int r = 0; r < (int)(MODEM_TILE_SYMS / 4 / 2 / 64); r++) {
      const uint32_t ls = 2 * (r * 64u + lane), s = w0 + ls;
      if (s >= job.n) {
        continue;
      }
      const float2 d0 = mod_point<MOD>(bits, nbytes, tab, s, ls, cbw), d1 = mod_point<MOD>(bits, nbytes, tab, s + 1, ls + 1, cbw);
      y0[s / 2] = sfbc_tx_a(d0, d1, sc);
      y1[s / 2] = sfbc_tx_b(d0, d1, sc);
    }
  } else {
    float4*      y0 = (float4*)(p.out + job.out_off[0]);
    float4*      y1 = (float4*)(p.out + job.out_off[1]);
    float4*      y2 = (float4*)(p.out + job.out_off[2]);
    float4*      y3 = (float4*)(p.out + job.out_off[3]);
    const float4 z  = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < (int)(MODEM_TILE_SYMS / 4 / 4 / 64); r++) {
      const uint32_t ls = 4 * (r * 64u + lane), s = w0 + ls;
      if (s >= job.n) {
        continue;
      }
      const float2 d0 = mod_point<MOD>(bits, nbytes, tab, s, ls, cbw), d1 = mod_point<MOD>(bits, nbytes, tab, s + 1, ls + 1, cbw);
      const float2 d2 = mod_point<MOD>(bits, nbytes, tab, s + 2, ls + 2, cbw), d3 = mod_point<MOD>(bits, nbytes, tab, s + 3, ls + 3, cbw);
      y0[s / 2]     = sfbc_tx_a(d0, d1, sc);
      y2[s / 2]     = sfbc_tx_b(d0, d1, sc);
      y1[s / 2]     = z;
      y3[s / 2]     = z;
      y0[s / 2 + 1] = z;
      y2[s / 2 + 1] = z;
      y1[s / 2 + 1] = sfbc_tx_a(d2, d3, sc);
      y3[s / 2 + 1] = sfbc_tx_b(d2, d3, sc);
    }
  }
}

__global__ __launch_bounds__(256) void txdiv_mod_kernel(const ModParams p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][MODEM_TILE_BITS / 128 + 4];
  __shared__ ModJob sjob;
  if (threadIdx.x < sizeof(ModJob) / 4) {
    ((uint32_t*)&sjob)[threadIdx.x] = ((const uint32_t*)(p.jobs + p.tile_job[blockIdx.x]))[threadIdx.x];
  }
  if ((threadIdx.x & 63u) == 0) {
    cb[threadIdx.x >> 6][MODEM_TILE_BITS / 128] = 0;
  }
  __syncthreads();
  const ModJob   job  = sjob;
  const uint32_t tile = blockIdx.x - job.tile0;
  uint32_t*      cbw  = cb[threadIdx.x >> 6];
  switch (job.mod) {
    case 0:
      mod_tile<0>(p, job, tile, cbw);
      break;
    case 1:
      mod_tile<1>(p, job, tile, cbw);
      break;
    case 2:
      mod_tile<2>(p, job, tile, cbw);
      break;
    case 3:
      mod_tile<3>(p, job, tile, cbw);
      break;
    default:
      mod_tile<4>(p, job, tile, cbw);
      break;
  }
}

} // namespace

hipError_t launch_eq(const EqParams& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if ((p.ports != 2 && p.ports != 4) || (p.nof_rx != 1 && p.nof_rx != 2) || p.n % p.ports || p.x_stride == 0) {
    return hipErrorInvalidValue;
  }
  const dim3 grid(ceil_div(p.n / p.ports, 256u));
  if (p.ports == 2) {
    hipLaunchKernelGGL(txdiv_eq_kernel<2>, grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL(txdiv_eq_kernel<4>, grid, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

hipError_t launch_precode(const PrecodeParams& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if (p.ports != 2 && p.ports != 4) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(txdiv_precode_kernel, dim3(ceil_div(p.n, 256u)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_layers(const LayerParams& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if (p.layers == 0 || p.layers > 4 || (uint64_t)p.n * p.layers > 0xffffffffull) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(txdiv_layer_kernel, dim3(ceil_div(p.n * p.layers, 256u)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_front(const FrontParams& p, bool llr8, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  if ((p.ports != 2 && p.ports != 4) || (p.nof_rx != 1 && p.nof_rx != 2) || p.n % p.ports || p.mod > 4 || !p.out || !p.x1_bits || !p.x2_cols) {
    return hipErrorInvalidValue;
  }
  const dim3 grid(ceil_div(p.n, MODEM_TILE_SYMS));
  if (p.csi && (((uintptr_t)p.csi) & 15u)) {
    return hipErrorInvalidValue;
  }
  if (llr8) {
    if (p.csi) {
      hipLaunchKernelGGL((txdiv_front_kernel<int8_t, true>), grid, dim3(256), 0, stream, p);
    } else {
      hipLaunchKernelGGL((txdiv_front_kernel<int8_t, false>), grid, dim3(256), 0, stream, p);
    }
  } else if (p.csi) {
    hipLaunchKernelGGL((txdiv_front_kernel<int16_t, true>), grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL((txdiv_front_kernel<int16_t, false>), grid, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

hipError_t launch_mod(const ModParams& p, hipStream_t stream)
{
  if (p.n_tiles == 0 || !p.bits || !p.out || !p.table || !p.jobs || !p.tile_job) {
    return p.n_tiles ? hipErrorInvalidValue : hipSuccess;
  }
  hipLaunchKernelGGL(txdiv_mod_kernel, dim3(p.n_tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

} // namespace txdiv
} // namespace phyhip
