// csi_device.h -- parameter block and launcher of csi_kernels.hip: CSI weighting of a PDSCH codeword's soft bits (csi_correction, pdsch.c:523-618)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace phyhip {
namespace csi {

// one codeword: n * Qm soft bits at `e` (int16 / int8, weighted in place), one CSI value per modulation symbol at `csi` (device-readable, >= 0)
struct WeightJob {
  void*        e;
  const float* csi;
  uint32_t     mod; // srsran_mod_t
  uint32_t     n;   // modulation symbols
};
// the codewords of a call in ONE launch: a workgroup covers CSI_TILE_SYMS symbols of one of them; job 1's first workgroup is tile1.  (A quarter of the
// demodulator's tile: the largest grant is 8 of those, too few workgroups to hide the latency of a kernel that starts with a reduction.)
#define CSI_TILE_SYMS 512u
struct WeightParams {
  WeightJob job[2];
  uint32_t  n_jobs;
  uint32_t  tile1;
};
hipError_t launch_weight(const WeightParams& p, bool llr8, hipStream_t stream);

} // namespace csi
} // namespace phyhip
