// ctrl_kernels.hip -- srsran_pcfich_decode (phch/pcfich.c:118-137, 156-222) and srsran_phich_decode (phch/phich.c:147-171, 181-312) as ONE small kernel on
// the staged rows of the subframe grids.  gfx950, wave64.
//
// One launch; every workgroup is one wave.  With Params::pcfich workgroup 0 is the PCFICH and workgroups 1 .. n_phich are one PHICH resource each; without it
// workgroups 0 .. n_phich - 1 are the resources.  A lane takes one group of `ports` neighbouring REs of a REG (pdcch_arith.h: eq_group, the PDCCH's equaliser --
// but the noise estimate is NOT halved here) and stores its symbols where the layer de-mapping puts them, in LDS; the few sums behind that run on lanes 0 .. 2 in
// the reference's order, every operation rounded once (rn_*):
//   PCFICH  32 soft bits = component * (float)-M_SQRT2, sign flipped where the chip is 1; corr[c] = sum over i from 0 of (2 b[c][i] - 1) data_f[i]
//           (srsran_vec_dot_prod_fff is a plain loop); max_corr starts at 0 and the comparison is strict: no positive correlation gives cfi 1, corr 0
//   PHICH   d = d0, or d0[4 i + 2 (ngroup % 2) + {0, 1}] with the extended prefix; chips; z[i] = sum over j from 0 of conj(w[nseq][j]) d[NSF i + j] / NSF (the
//           products by 0 and +-1 and the division by 2 or 4 are exact); bit = (float)((double)-(re + im) * M_SQRT1_2); corr of the NACK row, then of the ACK
//           row: the sum from 0 in index order, / 3; max_corr starts at -9999, strict
// The kernel is latency-sized: a few dozen REs.  Indices are 32-bit and were bounds-checked when the table was built; no atomics; plain vector stores.
#include "ctrl_device.h"
#include "pdcch_arith.h"

namespace phyhip {
namespace ctrl {
namespace {

using namespace modem;

static_assert(kPhichRe <= kPcfichRe, "the PHICH reuses the LDS arrays sized for the PCFICH's 16 REs; its extended-prefix index 4 (k >> 1) + 2 + 1 stays below 12");

// the group `lane` of a channel of n_re REs -> its symbols in d (LDS)
template <int PORTS>
__device__ __forceinline__ void eq_lane(const Params& p, const uint32_t* re_idx, uint32_t n_re, float noise, uint32_t lane, float2* d)
{
  if (lane * PORTS < n_re) {
    uint32_t idx[PORTS];
    float2   x[PORTS];
#pragma unroll
    for (int j = 0; j < PORTS; j++) {
      idx[j] = re_idx[lane * PORTS + j];
    }
    pdcch::eq_group<PORTS>(p.rx, p.ce, p.stride, p.nof_rx, idx, noise, x);
#pragma unroll
    for (int j = 0; j < PORTS; j++) {
      d[lane * PORTS + j] = x[j];
    }
  }
}

__global__ __launch_bounds__(64) void ctrl_kernel(const Params p)
{
  __shared__ __attribute__((aligned(16))) uint32_t cb[8];
  __shared__ uint32_t                              re_idx[kPcfichRe];
  __shared__ float2                                d[kPcfichRe];
  __shared__ float                                 data_f[32];
  __shared__ float                                 corr[3];
  const uint32_t lane = threadIdx.x;
  const bool     pcfich = p.pcfich && blockIdx.x == 0;
  const uint32_t r = blockIdx.x - (p.pcfich ? 1u : 0u), n_re = pcfich ? kPcfichRe : kPhichRe;
  if (lane < 8) {
    cb[lane] = 0; // chips_at reads one word past the last one
  }
  if (lane < n_re) {
    re_idx[lane] = pcfich ? p.pcfich_idx[lane] : p.jobs[r].idx[lane];
  }
  make_chips(p.x1_bits, p.x2_cols, p.seed, 0, 32, cb); // ends with the wave's LDS fence
  const float noise = p.noise_dev.v ? noise_avg(p.noise_dev) : p.noise;
  if (p.ports == 1) {
    eq_lane<1>(p, re_idx, n_re, noise, lane, d);
  } else if (p.ports == 2) {
    eq_lane<2>(p, re_idx, n_re, noise, lane, d);
  } else {
    eq_lane<4>(p, re_idx, n_re, noise, lane, d);
  }
  wave_sync_lds();
  const uint32_t chips = chips_at(cb, 0);
  if (pcfich) {
    if (lane < 32) {
      const float2 s = d[lane >> 1];
      data_f[lane]   = flip<float>(rn_mul((lane & 1u) ? s.y : s.x, p.qpsk_f), (chips >> lane) & 1u);
    }
    wave_sync_lds();
    if (lane < 3) {
      float acc = 0.f;
      for (uint32_t i = 0; i < 32; i++) {
        acc = kCfiTable[lane][i] ? rn_add(acc, data_f[i]) : rn_sub(acc, data_f[i]);
      }
      corr[lane] = acc;
    }
    wave_sync_lds();
    PcfichRow& o = *p.pcfich_out;
    if (lane == 0) {
      uint32_t index    = 0;
      float    max_corr = 0.f;
      for (uint32_t c = 0; c < 3; c++) {
        if (corr[c] > max_corr) {
          max_corr = corr[c];
          index    = c;
        }
      }
      o.cfi  = index + 1;
      o.corr = max_corr;
      if (p.cfi_word) {
        *p.cfi_word = (index == 2 && p.cfi3_to_2) ? 2u : index + 1;
      }
    }
    if (lane < 3) {
      o.corr3[lane] = corr[lane];
    }
    if (lane < 32) {
      o.data_f[lane] = data_f[lane];
    }
    if (lane < kPcfichRe) {
      o.d[lane][0] = d[lane].x;
      o.d[lane][1] = d[lane].y;
    }
    return;
  }
  // PHICH: lane i < 3 de-spreads z[i], lane 0 decides
  const PhichJob& job = p.jobs[r];
  const uint32_t  nsf = p.ext ? 2u : 4u;
  float*          bits = data_f;
  float2          z    = make_float2(0.f, 0.f);
  if (lane < 3) {
    for (uint32_t j = 0; j < nsf; j++) {
      const uint32_t k  = nsf * lane + j; // index into d
      const float2   s0 = p.ext ? d[4u * (k >> 1) + 2u * (job.ngroup & 1u) + (k & 1u)] : d[k];
      const uint32_t c  = (chips >> k) & 1u;
      const float2   s  = make_float2(flip<float>(s0.x, c), flip<float>(s0.y, c));
      const float    wr = p.ext ? (float)kPhichWExt[job.nseq][j][0] : (float)kPhichWNormal[job.nseq][j][0];
      const float    wi = p.ext ? (float)kPhichWExt[job.nseq][j][1] : (float)kPhichWNormal[job.nseq][j][1];
      const float    tr = rn_add(rn_mul(wr, s.x), rn_mul(wi, s.y)); // conj(w) d
      const float    ti = rn_sub(rn_mul(wr, s.y), rn_mul(wi, s.x));
      z                 = make_float2(rn_add(z.x, rn_div(tr, (float)nsf)), rn_add(z.y, rn_div(ti, (float)nsf)));
    }
    bits[lane] = __double2float_rn(__dmul_rn((double)(-rn_add(z.x, z.y)), 0.70710678118654752440));
  }
  wave_sync_lds();
  PhichRow& o = p.phich_out[r];
  if (lane < 3) {
    o.bits[lane] = bits[lane];
    o.z[lane][0] = z.x;
    o.z[lane][1] = z.y;
  }
  if (lane == 0) {
    float    max_corr = -9999.f, distance = 0.f;
    uint32_t index = 0;
    for (uint32_t i = 0; i < 2; i++) {
      float acc = 0.f;
      for (uint32_t k = 0; k < 3; k++) {
        acc = i ? rn_add(acc, bits[k]) : rn_sub(acc, bits[k]);
      }
      const float c = rn_div(acc, 3.f);
      if (c > max_corr) {
        max_corr = c;
        distance = c;
        index    = i;
      }
    }
    o.ack_value = index;
    o.distance  = distance;
  }
}

} // namespace

hipError_t launch(const Params& p, hipStream_t st)
{
  if ((p.ports != 1 && p.ports != 2 && p.ports != 4) || (p.nof_rx != 1 && p.nof_rx != 2) || !p.rx || !p.ce || !p.x1_bits || !p.x2_cols || p.n_phich > kMaxPhich ||
      (p.pcfich && !p.pcfich_out) || (p.n_phich && (!p.jobs || !p.phich_out)) || (!p.pcfich && !p.n_phich)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(ctrl_kernel, dim3((p.pcfich ? 1u : 0u) + p.n_phich), dim3(64), 0, st, p);
  return hipGetLastError();
}

} // namespace ctrl
} // namespace phyhip
