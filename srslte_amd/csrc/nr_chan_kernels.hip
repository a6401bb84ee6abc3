// nr_chan_kernels.hip -- the NR codeword front end and its transmit counterpart (gfx950).
//
// Reference behaviour, receive: pdsch_nr_decode_codeword (lib/src/phy/phch/pdsch_nr.c:426-483) behind srsran_predecoding_type(... PORT0 ...) (:540),
// pusch_nr_decode_codeword without control information (pusch_nr.c:830-911): srsran_predecoding_single -> srsran_demod_soft_demodulate_b ->
// srsran_vec_neg_bb -> srsran_sequence_apply_c.  Four passes over nof_re points in the reference and in the per-stage calls of this library; here ONE
// pass reads 8 (16 with channel estimates) bytes per symbol and writes Qm soft bits.  The equalised symbol lives in registers only.
// Transmit: pdsch_nr_encode_codeword (pdsch_nr.c:304-351): srsran_sequence_apply_bit -> srsran_mod_modulate on the rate matcher's output, one bit
// per byte: Qm bytes read and 8 bytes written per symbol, no packing pass.
//
// Launch shape (both kernels): that of modem_kernel (modem_kernels.hip).  One workgroup of 256 lanes = one tile of 2048 symbols of one job (the host
// lists the job of every workgroup), 512 consecutive symbols per wave, lane l takes l, l + 64, ...: every load instruction of a wave is one contiguous
// 512 B, and all of a wave's loads (8, or 16 with channel estimates) are issued before the first is used.  Each wave makes its own <= 4096 chips.
#include "hip_common.h"
#include "modem_arith.h"
#include "nr_chan_device.h"

namespace phyhip {
namespace nrchan {

using namespace modem;

namespace {

// ---- receive: one tile
template <int MOD>
__device__ __forceinline__ void front_tile(const FrontParams& p, const FrontJob& job, uint32_t tile, uint32_t* cbw, uint32_t* strip)
{
  using T              = int8_t;
  constexpr int  QM    = 2 * MOD;
  constexpr bool STAGE = QM == 6;
  const float2*  sym   = p.in + job.sym_off;
  const bool     eq    = job.ce_off != NR_CHAN_NO_CE;
  const float2*  ce    = p.in + (eq ? job.ce_off : job.sym_off);
  T*             out   = p.out + job.out_off;
  const bool     al    = (((uintptr_t)out) & 15u) == 0;
  const uint32_t lane  = threadIdx.x & 63u;
  const uint32_t w0    = tile * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4); // first symbol of this wave
  if (w0 >= job.n) {
    return;
  }
  constexpr int R = MODEM_TILE_SYMS / 256;
  float2        x[R], h[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t s = w0 + r * 64u + lane;
    x[r]             = s < job.n ? sym[s] : make_float2(0.f, 0.f);
  }
  if (eq) { // wave-uniform; both sets of loads are in flight before either is used
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint32_t s = w0 + r * 64u + lane;
      h[r]             = s < job.n ? ce[s] : make_float2(1.f, 0.f);
    }
  }
  // (the loads are in flight while the first lanes run the shift registers)
  make_chips(p.x1_bits, p.x2_cols, job.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (job.n - w0) * QM), cbw);
  if (eq) {
    // srsran_predecoding_single: the operation sequence of eq_kernel (modem_kernels.hip) with inv_scaling = 1, symbol by symbol
#pragma unroll
    for (int r = 0; r < R; r++) {
      float c0 = __fadd_rn(__fmul_rn(h[r].x, h[r].x), __fmul_rn(h[r].y, h[r].y));
      if (job.add_noise) {
        c0 = __fadd_rn(c0, job.noise);
      }
      const float re = __fmul_rn(__fdiv_rn(__fadd_rn(__fmul_rn(x[r].x, h[r].x), __fmul_rn(x[r].y, h[r].y)), c0), 1.0f);
      const float im = __fmul_rn(__fdiv_rn(__fsub_rn(__fmul_rn(x[r].y, h[r].x), __fmul_rn(x[r].x, h[r].y)), c0), 1.0f);
      x[r]           = make_float2(re, im);
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t sw   = w0 + r * 64u;     // first symbol of this pass
    const uint32_t s    = sw + lane;
    const bool     full = sw + 64 <= job.n; // wave-uniform
    if (s >= job.n) {
      continue;
    }
    int iv[QM];
    demod_int<T, MOD>(x[r].x, x[r].y, s, job.n, p.k, iv);
    // srsran_vec_neg_bb, then srsran_sequence_apply_c (pdsch_nr.c:467-470; pusch_nr.c has the two in the other order): one flip where the chip is 0
    const uint32_t c = ~chips_at(cbw, (r * 64u + lane) * QM);
    T              v[QM];
#pragma unroll
    for (int i = 0; i < QM; i++) {
      v[i] = flip<T>((T)iv[i], (c >> i) & 1u);
    }
    if (STAGE && al && full) {
      store_bits_staged<T, QM>(out + (size_t)sw * QM, v, strip);
    } else {
      store_bits<T, QM>(out + (size_t)s * QM, v, al);
    }
  }
}

__global__ __launch_bounds__(256) void nr_front_kernel(const FrontParams p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[4][MODEM_TILE_BITS / 128 + 4];
  __shared__ __attribute__((aligned(16))) uint32_t strips[4][96]; // 64 symbols x 6 bytes
  __shared__ FrontJob sjob;
  if (threadIdx.x < sizeof(FrontJob) / 4) {
    ((uint32_t*)&sjob)[threadIdx.x] = ((const uint32_t*)(p.jobs + p.tile_job[blockIdx.x]))[threadIdx.x];
  }
  if ((threadIdx.x & 63u) == 0) {
    cb[threadIdx.x >> 6][MODEM_TILE_BITS / 128] = 0; // chips_at reads one word past the last one
  }
  __syncthreads();
  FrontJob job = sjob;
  if (p.noise_dev) { // the estimator in front of this launch left the codeword's noise estimate on the device
    job.noise     = p.noise_dev[p.tile_job[blockIdx.x]];
    job.add_noise = job.noise > 0.f ? 1u : 0u;
  }
  const uint32_t tile = blockIdx.x - job.tile0;
  if (tile >= job.ntiles) {
    return;
  }
  uint32_t* cbw   = cb[threadIdx.x >> 6];
  uint32_t* strip = strips[threadIdx.x >> 6];
  switch (job.mod) {
    case 1:
      front_tile<1>(p, job, tile, cbw, strip);
      break;
    case 2:
      front_tile<2>(p, job, tile, cbw, strip);
      break;
    case 3:
      front_tile<3>(p, job, tile, cbw, strip);
      break;
    case 4:
      front_tile<4>(p, job, tile, cbw, strip);
      break;
    default:
      break;
  }
}

// ---- transmit: the QM bits of one symbol (one per byte, 0 / 1; the codeword starts 16-byte aligned), first bit most significant
template <int QM>
__device__ __forceinline__ uint32_t load_bits(const uint8_t* b)
{
  uint32_t w[2] = {0, 0};
  if (QM == 2) {
    w[0] = *(const uint16_t*)b;
  } else if (QM == 4) {
    w[0] = *(const uint32_t*)b;
  } else if (QM == 6) {
    const uint16_t* q = (const uint16_t*)b;
    w[0]              = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
    w[1]              = q[2];
  } else {
    const uint2 q = *(const uint2*)b;
    w[0] = q.x, w[1] = q.y;
  }
  return (w[0] & 0x01010101u) | (QM > 4 ? (w[1] & 0x01010101u) << 4 : 0u); // bit i of the symbol: bit 8 i (i < 4), bit 8 (i - 4) + 4
}
template <int QM>
__device__ __forceinline__ uint32_t symbol_index(uint32_t w, uint32_t chips)
{
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < QM; i++) {
    const uint32_t bit = (w >> (i < 4 ? 8 * i : 8 * (i - 4) + 4)) & 1u;
    v |= (bit ^ ((chips >> i) & 1u)) << (QM - 1 - i);
  }
  return v;
}

template <int MOD>
__device__ __forceinline__ void mod_tile(const ModParams& p, const ModJob& job, uint32_t tile, uint32_t* cbw)
{
  constexpr int  QM   = 2 * MOD;
  const uint8_t* bits = p.bits + job.bits_off;
  float2*        out  = p.out + job.out_off;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w0   = tile * MODEM_TILE_SYMS + (threadIdx.x >> 6) * (MODEM_TILE_SYMS / 4);
  if (w0 >= job.n) {
    return;
  }
  constexpr int R = MODEM_TILE_SYMS / 256;
  uint32_t      w[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t s = w0 + r * 64u + lane;
    w[r]             = s < job.n ? load_bits<QM>(bits + (size_t)s * QM) : 0u;
  }
  make_chips(p.x1_bits, p.x2_cols, job.seed, w0 * QM, min((MODEM_TILE_SYMS / 4) * QM, (job.n - w0) * QM), cbw);
  const float2* tab = p.table + mod_table_offset(MOD);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t s = w0 + r * 64u + lane;
    if (s >= job.n) {
      continue;
    }
    float2 o = tab[symbol_index<QM>(w[r], chips_at(cbw, (r * 64u + lane) * QM))];
    if (job.scale != 1.0f) {
      o.x = __fmul_rn(o.x, job.scale);
      o.y = __fmul_rn(o.y, job.scale);
    }
    out[s] = o;
  }
}

__global__ __launch_bounds__(256) void nr_mod_kernel(const ModParams p)
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
  if (tile >= job.ntiles) {
    return;
  }
  uint32_t* cbw = cb[threadIdx.x >> 6];
  switch (job.mod) {
    case 1:
      mod_tile<1>(p, job, tile, cbw);
      break;
    case 2:
      mod_tile<2>(p, job, tile, cbw);
      break;
    case 3:
      mod_tile<3>(p, job, tile, cbw);
      break;
    case 4:
      mod_tile<4>(p, job, tile, cbw);
      break;
    default:
      break;
  }
}

} // namespace

hipError_t launch_front(const FrontParams& p, hipStream_t stream)
{
  if (p.n_tiles == 0 || !p.in || !p.out || !p.jobs || !p.tile_job) {
    return p.n_tiles ? hipErrorInvalidValue : hipSuccess;
  }
  hipLaunchKernelGGL(nr_front_kernel, dim3(p.n_tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_mod(const ModParams& p, hipStream_t stream)
{
  if (p.n_tiles == 0 || !p.bits || !p.out || !p.table || !p.jobs || !p.tile_job) {
    return p.n_tiles ? hipErrorInvalidValue : hipSuccess;
  }
  hipLaunchKernelGGL(nr_mod_kernel, dim3(p.n_tiles), dim3(256), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrchan
} // namespace phyhip
