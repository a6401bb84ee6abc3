// chest_dl_device.h -- parameter block and launcher of chest_dl_kernels.hip: srsran_chest_dl_estimate_cfg (chest_dl.c:1004) for the pairs of a call
#pragma once
#include "chest_dl.h"

#include <hip/hip_runtime.h>

namespace phyhip {
namespace chest_dl {

// ONE launch, one workgroup of 256 lanes per job.  A job whose fields are out of range or whose offsets do not fit in_points / out_points writes nothing but
// a record of NANs.
struct Params {
  const float2* in;   // device-readable (the pinned image): the grids, the pilot rows, the PSS
  float2*       out;  // the ce grids (the pinned image, or device scratch in a grant call)
  const Job*    jobs; // device-readable, n_jobs entries
  Record*       rec;  // n_jobs entries
  float*        noise_dev; // nullptr, or n_jobs floats of DEVICE memory: Record::noise_out for the front-end kernels behind on the stream
  uint32_t      n_jobs;
  uint32_t      in_points, out_points;
};
hipError_t launch(const Params& p, hipStream_t stream);

} // namespace chest_dl
} // namespace phyhip
