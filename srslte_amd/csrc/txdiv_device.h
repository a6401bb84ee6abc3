// txdiv_device.h -- parameter blocks and launchers of txdiv_kernels.hip: transmit diversity (SFBC, TS 36.211 6.3.3.3 / 6.3.4.3) on 2 and 4 ports
#pragma once
#include "modem_device.h"

namespace phyhip {
namespace txdiv {

// ---- per-stage kernels (srsran_predecoding_diversity_multi, srsran_precoding_diversity, srsran_layer{,de}map_diversity on device buffers)

// y[rx], h[port][rx]: n REs each; x[layer]: n / ports symbols each, element i of layer j at x[j][i * x_stride] (1: layer planes; ports with x[j] = d + j:
// the layer-demapped codeword); csi: n floats or nullptr.  n a multiple of `ports`, every plane 16-byte aligned (x[j]: 8 when x_stride > 1)
struct EqParams {
  const float4* y[2];
  const float4* h[4][2];
  float2*       x[4];
  float*        csi;
  uint32_t      x_stride;
  uint32_t      ports, nof_rx, n;
  float         scaling;
};
hipError_t launch_eq(const EqParams& p, hipStream_t stream);

// x[layer]: n symbols each -> y[port]: ports * n points each; scale: the reference's float factor (host evaluated)
struct PrecodeParams {
  const float2* x[4];
  float2*       y[4];
  uint32_t      ports, n;
  float         scale;
};
hipError_t launch_precode(const PrecodeParams& p, hipStream_t stream);

// to_layers: x[j][i] = d[layers i + j], else d[layers i + j] = x[j][i]; i < n
struct LayerParams {
  float2*  d;
  float2*  x[4];
  uint32_t layers, n, to_layers;
};
hipError_t launch_layers(const LayerParams& p, hipStream_t stream);

// ---- receive front end of one codeword: SFBC combining + layer de-mapping + soft demodulation + descrambling in one pass (txdiv_front_kernel)
struct FrontParams {
  const float4*   y[2];    // [rx]: n REs
  const float4*   h[4][2]; // [port][rx]
  void*           out;     // n * Qm soft bits (int16 / int8), 16-byte aligned
  float*          csi;     // n floats, 16-byte aligned: the channel-state values of srsran_predecoding_diversity_multi; nullptr: not wanted
  uint32_t        mod, n, seed;
  uint32_t        ports, nof_rx;
  float           scaling;
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
  modem::Consts   k;
};
hipError_t launch_front(const FrontParams& p, bool llr8, hipStream_t stream);

// ---- transmit: scrambling + modulation + layer map + SFBC precoder (txdiv_mod_kernel); the job of every workgroup is listed by the host.
// A workgroup covers MODEM_TILE_SYMS symbols of the codeword; a lane modulates one RE pair (2 ports) or quad (4 ports) and writes it on every port.
struct ModJob {
  uint32_t mod, n, seed, ports;
  float    scale;      // the precoder's factor: every written component is one product table value * scale
  uint32_t bits_off;   // first byte of the job's packed bits
  uint32_t out_off[4]; // first point of each port's plane (float2 units from ModParams::out)
  uint32_t tile0;      // first workgroup of the job
};
struct ModParams {
  const uint8_t*  bits;
  float2*         out;
  const float2*   table; // modem::mod_tables()
  const ModJob*   jobs;  // device-readable
  const uint32_t* tile_job;
  uint32_t        n_tiles;
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
};
hipError_t launch_mod(const ModParams& p, hipStream_t stream);

} // namespace txdiv
} // namespace phyhip
