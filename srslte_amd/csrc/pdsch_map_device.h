// pdsch_map_device.h -- parameter block and launcher of pdsch_map_kernels.hip: RE de-mapping of a PDSCH grant (srsran_pdsch_get, pdsch.c:246)
#pragma once
#include "pdsch_map.h"

#include <hip/hip_runtime.h>

namespace phyhip {
namespace pdsch_map {

// n_planes planes in ONE launch: plane p reads the staged image at in + p * in_stride (in_points points of it are there) and writes nof_re points at
// out + p * out_stride (with in_b: see below), plus a zero behind them when nof_re is odd (out_stride > nof_re then).  Strides in points.
struct DemapParams {
  const float2* in;
  float2*       out;
  const Seg*    tab; // device-readable, n_seg entries
  uint32_t      n_seg, n_planes;
  uint32_t      in_stride, in_points;
  uint32_t      out_stride, nof_re;
  const float2* in_b;     // nullptr, or where the planes from planes_a on lie (same stride, same extent): plane p reads in_b + (p - planes_a) * in_stride --
  uint32_t      planes_a; // the _est grant calls: the received grids in the pinned image, the estimator's ce grids in device scratch
};
#define PDSCH_DEMAP_SEGS 16u // table entries of a workgroup: 12 lanes each, 192 lanes = three whole waves
hipError_t launch_demap(const DemapParams& p, hipStream_t stream);

} // namespace pdsch_map
} // namespace phyhip
