// pdcch_kernels.hip -- srsran_pdcch_extract_llr (phch/pdcch.c:424-487) as ONE kernel on the staged control rows of the subframe grids: REG de-mapping,
// equaliser, layer de-mapping, QPSK demodulator and descrambler.  gfx950, wave64.
//
// One lane per group of `ports` neighbouring REs of a REG (a REG has four, so a group never leaves it): one symbol on one port, an SFBC pair on two, a quad
// on four.  The lane reads its REs of every plane straight from the staged grids through the REG table (pdcch_map.h) -- there is no extracted plane in
// memory -- equalises them (pdcch_arith.h: eq_group), and stores its 2 * ports soft bits where the layer de-mapping puts them: symbol j of group g is
// symbol g * ports + j of d;
// then soft bit = component * (float)-M_SQRT2 (srsran_demod_soft_demodulate, QPSK to float), its sign flipped where the chip of the sequence with
// c_init = sf_idx * 512 + cell_id is 1 (srsran_scrambling_f_offset).  A wave covers 128 * ports consecutive soft bits, so its chips start at a multiple of
// 128: make_chips (modem_arith.h) from the tables srsran_sequence_apply_f uses.  Every operation of the one-port and four-port arithmetic is rounded once in a
// fixed order (rn_*); no atomics: the same input gives the same bits.  Indices are 32-bit; the table's entries were bounds-checked when it was built.
// In the search from the received grids alone the CFI, and so the table and the region's size, and the noise estimate are read from device memory, where the
// kernels ahead on the stream left them (pdcch_device.h: FrontParams::cfi_dev, noise_dev).
#include "pdcch_arith.h"
#include "pdcch_device.h"

namespace phyhip {
namespace pdcch {
namespace {

using namespace modem;

template <int PORTS>
__global__ __launch_bounds__(64) void pdcch_front_kernel(const FrontParams p)
{
  constexpr uint32_t                               BITS = 2 * PORTS; // soft bits of a lane
  __shared__ __attribute__((aligned(16))) uint32_t cb[4 * PORTS + 4];
  const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane, bit0 = blockIdx.x * 64u * BITS;
  const uint32_t* tab  = p.tab;
  uint32_t        nsym = p.nsym;
  if (p.cfi_dev) { // the region of the CFI the PCFICH kernel left (wave-uniform)
    const uint32_t c = min(*p.cfi_dev - 1u, 2u);
    tab  = p.tab3[c];
    nsym = p.nsym3[c];
    if (bit0 >= 2u * nsym) {
      return;
    }
  }
  if (lane < 4 * PORTS + 4) {
    cb[lane] = 0; // chips_at reads one word past the last one
  }
  make_chips(p.x1_bits, p.x2_cols, p.seed, bit0, min(64u * BITS, 2u * nsym - bit0), cb);
  if (g * PORTS >= nsym) {
    return;
  }
  uint32_t idx[PORTS];
  if constexpr (PORTS == 4) {
    const uint4 t = *reinterpret_cast<const uint4*>(tab + g * 4u);
    idx[0] = t.x, idx[1] = t.y, idx[2] = t.z, idx[3] = t.w;
  } else if constexpr (PORTS == 2) {
    const uint2 t = *reinterpret_cast<const uint2*>(tab + g * 2u);
    idx[0] = t.x, idx[1] = t.y;
  } else {
    idx[0] = tab[g];
  }
  const uint32_t stride = p.plane_stride, nof_rx = p.nof_rx;
  float2         x[PORTS];
  const float noise = (PORTS == 1 && p.noise_dev.v) ? rn_mul(noise_avg(p.noise_dev), 0.5f) : p.noise; // pdcch.c:471
  eq_group<PORTS>(p.planes, p.ce ? p.ce : p.planes + nof_rx * stride, stride, nof_rx, idx, noise, x);
  const uint32_t c = chips_at(cb, lane * BITS);
  float          v[BITS];
#pragma unroll
  for (int j = 0; j < PORTS; j++) {
    v[2 * j]     = flip<float>(rn_mul(x[j].x, p.qpsk_f), (c >> (2 * j)) & 1u);
    v[2 * j + 1] = flip<float>(rn_mul(x[j].y, p.qpsk_f), (c >> (2 * j + 1)) & 1u);
  }
  store_bits<float, BITS>(p.llr + g * BITS, v, true);
  if (p.dbg_d) {
#pragma unroll
    for (int j = 0; j < PORTS; j++) {
      p.dbg_d[g * PORTS + j] = x[j];
    }
  }
  if (p.dbg_planes) {
    const uint32_t n_planes = nof_rx * (1u + p.ports);
    for (uint32_t pl = 0; pl < n_planes; pl++) {
#pragma unroll
      for (int j = 0; j < PORTS; j++) {
        p.dbg_planes[pl * p.dbg_stride + g * PORTS + j] = p.planes[pl * stride + idx[j]];
      }
    }
  }
}

__global__ __launch_bounds__(256) void pdcch_gather_kernel(const float2* __restrict__ planes, uint32_t plane_stride, const uint32_t* __restrict__ tab, uint32_t nsym,
                                                           uint32_t n_planes, float2* __restrict__ out, uint32_t out_stride)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nsym) {
    return;
  }
  const uint32_t k = tab[i];
  for (uint32_t pl = 0; pl < n_planes; pl++) {
    out[pl * out_stride + i] = planes[pl * plane_stride + k];
  }
}

} // namespace

hipError_t launch_front(const FrontParams& p, hipStream_t st)
{
  if ((p.ports != 1 && p.ports != 2 && p.ports != 4) || (p.nof_rx != 1 && p.nof_rx != 2) || p.nsym == 0 || p.nsym % 36 || !p.planes || !p.tab || !p.llr ||
      !p.x1_bits || !p.x2_cols || 2ull * p.nsym > (uint64_t)MODEM_SEQ_NCHUNKS * MODEM_SEQ_CHUNK) {
    return hipErrorInvalidValue;
  }
  const dim3 grid(ceil_div(p.nsym / p.ports, 64u)), block(64);
  if (p.ports == 1) {
    hipLaunchKernelGGL(pdcch_front_kernel<1>, grid, block, 0, st, p);
  } else if (p.ports == 2) {
    hipLaunchKernelGGL(pdcch_front_kernel<2>, grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL(pdcch_front_kernel<4>, grid, block, 0, st, p);
  }
  return hipGetLastError();
}

hipError_t launch_gather(const float2* planes, uint32_t plane_stride, const uint32_t* tab, uint32_t nsym, uint32_t n_planes, float2* out, uint32_t out_stride,
                         hipStream_t st)
{
  if (!planes || !tab || !out || nsym == 0 || n_planes == 0 || n_planes > kMaxPlanes) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(pdcch_gather_kernel, dim3(ceil_div(nsym, 256u)), dim3(256), 0, st, planes, plane_stride, tab, nsym, n_planes, out, out_stride);
  return hipGetLastError();
}

} // namespace pdcch
} // namespace phyhip
