// nr_chan_device.h -- job lists and launchers of nr_chan_kernels.hip: the NR codeword front end (equaliser + int8 demodulator + sign change +
// descrambler in one pass) and its transmit counterpart (scrambler + modulator on the rate matcher's bit-per-byte output).
#pragma once
#include "modem_device.h"

namespace phyhip {
namespace nrchan {

#define NR_CHAN_NO_CE 0xffffffffu

// one received codeword.  Offsets count from FrontParams::in (cf_t units) and FrontParams::out (soft bits = bytes).
struct FrontJob {
  uint32_t mod;       // srsran_mod_t, QPSK .. 256-QAM
  uint32_t n;         // symbols (nof_re)
  uint32_t sym_off;   // first symbol
  uint32_t ce_off;    // first channel estimate, NR_CHAN_NO_CE: the symbols are already equalised
  uint32_t out_off;   // first soft bit
  uint32_t seed;      // c_init
  uint32_t tile0;     // first workgroup of this job
  uint32_t ntiles;
  float    noise;     // noise_estimate of srsran_predecoding_single
  uint32_t add_noise; // noise > 0 (MMSE), as launch_eq derives it
};

struct FrontParams {
  const float2*   in;       // symbols and channel estimates of all jobs (a pinned host image or device memory)
  int8_t*         out;      // soft bits of all jobs
  const FrontJob* jobs;     // device-readable
  const uint32_t* tile_job; // job index of every workgroup
  uint32_t        n_tiles;
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
  modem::Consts   k;
  const float*    noise_dev = nullptr; // nullptr, or DEVICE memory, one float per job: replaces FrontJob::noise / add_noise (nr_dmrs_est_kernel writes it)
};
hipError_t launch_front(const FrontParams& p, hipStream_t stream);

// one codeword to transmit: n Qm bits, one per byte, from ModParams::bits + bits_off -> n constellation points at ModParams::out + out_off
struct ModJob {
  uint32_t mod, n, seed;
  float    scale;    // 1.0f: none
  uint32_t bits_off; // first bit (byte) of the codeword
  uint32_t out_off;  // first constellation point
  uint32_t tile0;
  uint32_t ntiles;
};
struct ModParams {
  const uint8_t*  bits;  // the rate matcher's output (srsran_hip_sch_nr_encode: d_e_bits)
  float2*         out;
  const float2*   table; // modem::mod_tables()
  const ModJob*   jobs;  // device-readable
  const uint32_t* tile_job;
  uint32_t        n_tiles;
  const uint32_t* x1_bits;
  const uint32_t* x2_cols;
};
hipError_t launch_mod(const ModParams& p, hipStream_t stream);

} // namespace nrchan
} // namespace phyhip
