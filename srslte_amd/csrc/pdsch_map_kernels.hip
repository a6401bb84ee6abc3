// pdsch_map_kernels.hip -- RE de-mapping of a PDSCH grant on the device (gfx950): the gather srsran_pdsch_get (pdsch.c:246; srsran_pdsch_cp :136-220) does
// once per receive antenna and once per (port, antenna) estimate grid, for all those planes in one launch.
//
// The host states the mapping as a table (pdsch_map.h): one entry per allocated PRB of a grid row -- where its 12 REs start in the staged grid, where its
// taken REs go in the plane, a 12-bit mask of the REs taken.  A lane owns one RE of one entry: RE k of a mask m goes to out[off + popcount(m & ((1 << k) - 1))].
// No lane depends on another: no atomics, no LDS, no barrier.
//
// Launch shape: blockIdx.y is the plane, a workgroup of 192 lanes (three whole waves) covers PDSCH_DEMAP_SEGS = 16 consecutive entries, lane t entry t / 12
// and RE t % 12.  Consecutive entries of a row are consecutive PRBs of an allocation, so a wave's 8-byte loads run along the sub-carriers (512 contiguous
// bytes per wave-instruction where the allocation is contiguous) and its stores are contiguous up to the reference-signal holes.  8 bytes per lane is one
// point: wider loads would put two REs with different destinations into a lane and buy nothing -- the kernel moves at most 1540 x 12 points x 10 planes
// (1.5 MB each way), so it is bound by the launch, not by bandwidth.  The largest grant is 97 workgroups per plane.
// Every index is bounded by the extents in the parameter block: entry < n_seg, grid index < in_points, plane index < nof_re.
#include "hip_common.h"
#include "pdsch_map_device.h"

namespace phyhip {
namespace pdsch_map {

namespace {

__global__ __launch_bounds__(12 * PDSCH_DEMAP_SEGS) void pdsch_demap_kernel(const DemapParams p)
{
  const uint32_t plane = blockIdx.y;
  const float2*  in    = (p.in_b && plane >= p.planes_a) ? p.in_b + (size_t)(plane - p.planes_a) * p.in_stride : p.in + (size_t)plane * p.in_stride;
  float2*        out   = p.out + (size_t)plane * p.out_stride;
  const uint32_t e     = blockIdx.x * PDSCH_DEMAP_SEGS + threadIdx.x / 12u;
  const uint32_t k     = threadIdx.x % 12u;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (p.nof_re & 1u) && p.nof_re < p.out_stride) {
    out[p.nof_re] = make_float2(0.f, 0.f); // the padding point behind an odd plane: the MIMO front ends read the last pair whole
  }
  if (e >= p.n_seg) {
    return;
  }
  const Seg      s   = p.tab[e];
  const uint32_t src = s.grid_off + k;
  const uint32_t dst = s.out_off + (uint32_t)__popc(s.mask & ((1u << k) - 1u));
  if (((s.mask >> k) & 1u) && src < p.in_points && dst < p.nof_re) {
    out[dst] = in[src];
  }
}

} // namespace

hipError_t launch_demap(const DemapParams& p, hipStream_t stream)
{
  if (p.n_seg == 0 || p.n_planes == 0) {
    return hipSuccess;
  }
  if (!p.in || !p.out || !p.tab || p.n_seg > MAX_SEG || p.n_planes > 65535u || p.in_points > p.in_stride || p.nof_re > p.out_stride) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(pdsch_demap_kernel, dim3(ceil_div(p.n_seg, PDSCH_DEMAP_SEGS), p.n_planes), dim3(12 * PDSCH_DEMAP_SEGS), 0, stream, p);
  return hipGetLastError();
}

} // namespace pdsch_map
} // namespace phyhip
