// chest_ul_device.h -- parameter block and launcher of chest_ul_kernels.hip: srsran_chest_ul_estimate_pusch (chest_ul.c:370-404) for the grants of a call
#pragma once
#include "chest_ul.h"
#include "modem_device.h"

#include <hip/hip_runtime.h>

namespace phyhip {
namespace chest_ul {

// ONE launch, one workgroup of 256 lanes per job.  A job whose offsets do not fit in_points / out_points, or whose n is outside 2 .. CHEST_UL_MAX_REFS,
// writes nothing but a record of NANs.
struct Params {
  const float2* in;   // device-readable (the pinned image): the received reference rows and the DMRS rows
  float2*       out;  // the estimates' rows
  const Job*    jobs; // device-readable, n_jobs entries
  Record*       rec;  // n_jobs entries
  modem::EqJob* eq;   // nullptr, or n_jobs entries of DEVICE memory: {end_pair, noise_estimate, noise_estimate > 0} for the equaliser launch behind
  uint32_t      n_jobs;
  uint32_t      in_points, out_points;
};
hipError_t launch(const Params& p, hipStream_t stream);

} // namespace chest_ul
} // namespace phyhip
