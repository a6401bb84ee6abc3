// spmux_device.h -- parameter blocks and launchers of spmux_kernels.hip: spatial multiplexing and large-delay CDD on 2 ports, 2 receive antennas
// (TS 36.211 6.3.4.2; the arithmetic is mimo_equalise / mimo_precode of modem_arith.h)
#pragma once
#include "modem_device.h"

namespace phyhip {
namespace spmux {

// what the receive kernels need to know of the transmission.  layers 2: pre[parity of the RE] is a HEFF_* value (modem_arith.h), mmse selects the
// equaliser; layers 1: pre[] is the codebook index (a PRE_* value).  norm: the reference's float 2 / scaling or (float)M_SQRT2 / scaling
struct Scheme {
  uint32_t layers;
  uint32_t pre[2];
  uint32_t mmse;
  float    norm, noise;
  modem::NoiseAvg dev_noise; // v != nullptr: the noise estimate is made on the device ahead on the stream (`noise` is then not looked at)
};

// ---- per-stage kernels (srsran_hip_predecoding_mimo / srsran_hip_precoding_mimo on device planes): one lane per RE, planes of any 4-byte alignment

// y[rx], h[port][rx], x[layer]: n complex points each as float pairs; csi[layer]: n floats or nullptr
struct EqParams {
  const float* y[2];
  const float* h[2][2];
  float*       x[2];
  float*       csi[2];
  uint32_t     n;
  Scheme       s;
};
hipError_t launch_eq(const EqParams& p, hipStream_t stream);

// x[layer] -> y[port], n points each; kind[parity of the RE]: a TXPRE_* value; scale: the reference's float factor (host evaluated)
struct PrecodeParams {
  const float* x[2];
  float*       y[2];
  uint32_t     n;
  uint32_t     kind[2];
  float        scale;
};
hipError_t launch_precode(const PrecodeParams& p, hipStream_t stream);

// ---- receive front end of the grant's codewords: effective channel + equaliser + soft demodulation + descrambling in one pass (spmux_front_kernel).
// Codeword k is layer k.  out[k] == nullptr: the codeword is not wanted (it is equalised, as its layer is part of the solve, and nothing else).
struct FrontParams {
  const float4*   y[2];    // [rx]: n REs, 16-byte aligned, readable up to the next multiple of 2 REs
  const float4*   h[2][2]; // [port][rx]
  void*           out[2];  // [codeword]: n * Qm soft bits (int16 / int8), 16-byte aligned
  float*          csi[2];  // [layer]: n floats, 8-byte aligned: the channel-state values of srsran_hip_predecoding_mimo; csi[0] == nullptr: not wanted
  uint32_t        mod[2], seed[2];
  uint32_t        n;
  Scheme          s;
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
  modem::Consts   k;
};
hipError_t launch_front(const FrontParams& p, bool llr8, hipStream_t stream);

// ---- transmit: scrambling + modulation of each codeword + precoder (spmux_mod_kernel); the job of every workgroup is listed by the host.
// A workgroup covers MODEM_TILE_SYMS REs; a lane modulates one RE pair of each codeword and writes the pair on both ports.
struct ModJob {
  uint32_t mod[2], seed[2];
  uint32_t bits_off[2]; // first byte of each codeword's packed bits
  uint32_t n;           // REs
  uint32_t layers;      // 1: codeword 0 only
  uint32_t kind[2];     // TXPRE_* of an even / odd RE
  float    scale;
  uint32_t out_off[2];  // first point of each port's plane (float2 units from ModParams::out), an even number
  uint32_t tile0;       // first workgroup of the job
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

} // namespace spmux
} // namespace phyhip
