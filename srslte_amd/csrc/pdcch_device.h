// pdcch_device.h -- what pdcch_host.cpp and pdcch_kernels.hip share: the parameter block of the PDCCH front end and the launches.
#pragma once
#include "hip_common.h"
#include "modem_device.h"

namespace phyhip {
namespace pdcch {

constexpr uint32_t kMaxPlanes = 10; // nof_rx * (1 + nof_ports) of the largest region taken: 2 * (1 + 4)

// The staged image holds the region's rows of every plane, plane p at planes + p * plane_stride: the received grids [rx], then the estimate grids
// [port][rx] at nof_rx + port * nof_rx + rx.  tab: the region's 4 nregs grid indices (pdcch_map.h), every one below plane_stride (checked when it is built).
struct FrontParams {
  const float2*   planes;
  uint32_t        plane_stride; // points
  const uint32_t* tab;
  uint32_t        nsym; // 4 nregs: a multiple of 36
  uint32_t        ports, nof_rx;
  float           noise; // one port: added to the gain when above 0
  uint32_t        seed;  // c_init of the scrambling sequence
  float           qpsk_f; // (float)-M_SQRT2, as modem::Consts has it
  const uint32_t* x1_bits; // modem::Params: the sequence tables
  const uint32_t* x2_cols;
  float*          llr;        // 2 nsym soft bits, 16-byte aligned
  float2*         dbg_d;      // nullptr, or nsym equalised symbols
  float2*         dbg_planes; // nullptr, or the extracted planes: plane p at dbg_planes + p * dbg_stride, nsym points each
  uint32_t        dbg_stride;
  // what the search from the received grids alone sets (srsran_hip_pdcch_search_est); all null / zero: the behaviour above
  const float2*   ce;        // nullptr: the estimate grids lie behind the received ones in `planes`; else [port][rx] at ce + (port * nof_rx + rx) * plane_stride
  modem::NoiseAvg noise_dev; // v != nullptr: one port takes half the estimate a kernel ahead on the stream left, instead of `noise`
  const uint32_t* cfi_dev;   // nullptr, or the CFI (1 .. 3) in device memory: the launch covers nsym (the largest region), the kernel takes
  const uint32_t* tab3[3];   //   the table and the size of that CFI's region, and the lanes past it leave
  uint32_t        nsym3[3];
};
hipError_t launch_front(const FrontParams& p, hipStream_t st);
// srsran_regs_pdcch_get on n_planes staged planes: out[p * out_stride + i] = planes[p * plane_stride + tab[i]], i < nsym
hipError_t launch_gather(const float2* planes, uint32_t plane_stride, const uint32_t* tab, uint32_t nsym, uint32_t n_planes, float2* out, uint32_t out_stride,
                         hipStream_t st);

} // namespace pdcch
} // namespace phyhip
