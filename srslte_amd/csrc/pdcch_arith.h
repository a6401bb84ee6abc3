// pdcch_arith.h -- the equaliser of the downlink control channels on one group of `PORTS` neighbouring REs of a REG, as pdcch.c:466-475, pcfich.c:197-205 and
// phich.c:248-256 run it: one symbol on one port, an SFBC pair on two, a quad on four.  Shared by pdcch_kernels.hip, ctrl_kernels.hip and pbch_kernels.hip (pbch.c:506-512: the same calls).  Device code only.
//   one port    x = sum_rx y conj(h) / (sum_rx |h|^2 [+ noise when noise > 0])      srsran_predecoding_single_multi, precoding.c:182-305
//   two ports   modem_arith.h sfbc_add<2> / sfbc_finish<2>                           srsran_predecoding_diversity_gen_, :438-463 (hh == 0 -> 1e-4)
//   four ports  modem_arith.h sfbc4_add / sfbc4_finish                               the body WITHOUT CSI, :465-498
// Every operation of the one-port and four-port arithmetic is rounded once in a fixed order (rn_*).
#pragma once
#include "modem_arith.h"

namespace phyhip {
namespace pdcch {
namespace {

// rx: the received grids, antenna a at rx + a * stride; ce: the estimate grids, [port][rx] at ce + (port * nof_rx + a) * stride; idx: the group's grid
// indices; x: its symbols in the order of d (the layer de-mapping is where the caller stores them)
template <int PORTS>
__device__ __forceinline__ void eq_group(const float2* rx, const float2* ce, uint32_t stride, uint32_t nof_rx, const uint32_t* idx, float noise, float2* x)
{
  using namespace modem;
  if constexpr (PORTS == 1) {
    float xr = 0.f, xi = 0.f, gain = 0.f;
    for (uint32_t a = 0; a < nof_rx; a++) {
      const float2 y = rx[a * stride + idx[0]], h = ce[a * stride + idx[0]];
      const float  pr = rn_add(rn_mul(h.x, y.x), rn_mul(h.y, y.y)); // conj(h) y
      const float  pi = rn_sub(rn_mul(h.x, y.y), rn_mul(h.y, y.x));
      const float  sq = rn_add(rn_mul(h.x, h.x), rn_mul(h.y, h.y));
      xr              = a == 0 ? pr : rn_add(xr, pr);
      xi              = a == 0 ? pi : rn_add(xi, pi);
      gain            = a == 0 ? sq : rn_add(gain, sq);
    }
    if (noise > 0.f) {
      gain = rn_add(gain, noise);
    }
    x[0] = make_float2(rn_div(xr, gain), rn_div(xi, gain));
  } else if constexpr (PORTS == 2) {
    Sfbc acc;
    for (uint32_t a = 0; a < nof_rx; a++) {
      const float2*  y  = rx + a * stride;
      const float2*  h0 = ce + a * stride;
      const float2*  h1 = ce + (nof_rx + a) * stride;
      const uint32_t k0 = idx[0], k1 = idx[1];
      sfbc_add<2>(acc, h0[k0], h1[k1], h1[k0], h0[k1], y[k0], y[k1]);
    }
    float2 csi;
    sfbc_finish<2>(acc, 1.0f, (float)nof_rx, x[0], x[1], csi);
  } else {
    Sfbc4 acc;
    for (uint32_t a = 0; a < nof_rx; a++) {
      const float2*  y  = rx + a * stride;
      const uint32_t k0 = idx[0], k1 = idx[1], k2 = idx[2], k3 = idx[3];
      const float2   h0 = ce[a * stride + k0], h1 = ce[(nof_rx + a) * stride + k2];
      const float2   h2 = ce[(2 * nof_rx + a) * stride + k0], h3 = ce[(3 * nof_rx + a) * stride + k2];
      sfbc4_add(acc, h0, h1, h2, h3, y[k0], y[k1], y[k2], y[k3]);
    }
    sfbc4_finish(acc, 1.0f, x);
  }
}

} // namespace
} // namespace pdcch
} // namespace phyhip
