// pbch_kernels.hip -- srsran_pbch_decode (phch/pbch.c:444-557) with EVERY hypothesis of a call at once: one wave per (cell, antenna hypothesis, nb, dst, src),
// one launch per call.  gfx950, wave64.
//
// (a) The newest frame.  A wave whose combination reads the newest row (src + nb + 1 == frame_idx), and the wave of combination 0, compute the newest
// frame's soft bits for their own antenna hypothesis from the call's planes: the REs in closed form (pbch_map.h: re_pos), the control-channel equaliser on
// groups of `nant` neighbouring REs (pdcch_arith.h: eq_group -- one port with the caller's whole noise estimate, added only when > 0; an SFBC pair; a quad),
// the layer de-mapping by where the group's symbols are stored, soft bit = component * (float)-M_SQRT2.  The row stays in LDS: recomputing 240 symbols per
// wave is cheaper than a second launch or a dependency across the grid.
// (b) decode_frame (pbch.c:399-434).  temp[k], k < 4 nof_bits, is SRSRAN_RX_NULL outside rows [dst, dst + n) and row src + (k / nof_bits - dst) of the soft
// bits inside, its sign flipped where chip k of the cell's sequence is 1; rows below frame_idx - 1 come from the caller's history, row frame_idx - 1 is the
// wave's own.  temp is never stored: it is the soft-bit source of the shared rate de-matcher (conv_wave.h: rm_conv_wave), whose == 10000.f comparisons treat
// a soft bit that happens to equal 10000.f as NULL, as the reference does.  Then the product with (float)(1.0 / (2 n)), the quantiser of
// srsran_viterbi_decode_f with gain 1000, the tail-biting decoder over 40 bits, and on lane 0 the CRC remainder and the count of payload ones.  The mask of
// the antenna hypothesis and the verdict are the host's (pbch_map.h: verdict).
// (c) The history row.  Combination 0 of the cell's LAST antenna hypothesis stores its newest row to the output image: q->llr is one buffer in the
// reference, so the rows a later call combines hold the last hypothesis's soft bits, even where one port is tried.
// LDS per wave: 80 decision words, 120 de-matched floats, 120 symbols, 40 bits, the 480 soft bits of the newest row, the 60 sequence words: 3.6 KB.
// Every index is below 2^16; the host checked the cells' offsets against the image.
#include "conv_wave.h"
#include "pbch_device.h"
#include "pdcch_arith.h"

namespace phyhip {
namespace pbch {
namespace {

using namespace modem;

struct Lds {
  uint64_t words[80]; // conv::nof_words(40, true) == 74
  float    rm[pbch_map::kCoded];
  uint16_t sym[pbch_map::kCoded];
  uint8_t  bits[kBits];
  float    row[pbch_map::kMaxBits];
  uint32_t seq[pbch_map::kSeqWords];
};

template <int N>
__device__ __forceinline__ void newest_row(const Params& p, const Cell& c, float noise, float* row, float2* dbg_d)
{
  const uint32_t nre = pbch_map::nof_re(c.cp_nsymb);
  for (uint32_t g = threadIdx.x; g * N < nre; g += 64) {
    uint32_t idx[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
      uint32_t r, col;
      pbch_map::re_pos(g * N + j, c.id, c.cp_nsymb, &r, &col);
      idx[j] = r * c.row_stride + col;
    }
    float2 x[N];
    pdcch::eq_group<N>(p.planes + c.o_rx, p.planes + c.o_ce, c.ce_stride, 1, idx, noise, x);
#pragma unroll
    for (int j = 0; j < N; j++) {
      row[2 * (g * N + j)]     = rn_mul(x[j].x, p.qpsk_f);
      row[2 * (g * N + j) + 1] = rn_mul(x[j].y, p.qpsk_f);
      if (dbg_d) {
        dbg_d[g * N + j] = x[j];
      }
    }
  }
}

__global__ __launch_bounds__(64) void pbch_kernel(const Params p)
{
  __shared__ Lds s;
  const Job      job  = p.jobs[blockIdx.x];
  const uint32_t lane = threadIdx.x, ci = conv::uniform(job.cell), nant = conv::uniform(job.nant), cmb = conv::uniform(job.combo);
  const Cell     c    = p.cells[ci];
  const uint32_t f = conv::uniform(c.f), nof_bits = 2 * pbch_map::nof_re(conv::uniform(c.cp_nsymb));
  uint32_t       nb, dst, src;
  pbch_map::combo(f, cmb, &nb, &dst, &src);
  const uint32_t n = nb + 1;
  if (lane < pbch_map::kSeqWords) {
    s.seq[lane] = p.seq[c.o_seq + lane];
  }
  // (a)
  if (nant != 0 && (src + n == f || cmb == 0)) { // (wave-uniform)
    const uint32_t slot  = c.first_slot + job.slot;
    float2*        dbg_d = (p.dbg_d && cmb == 0) ? p.dbg_d + (size_t)slot * pbch_map::kMaxRe : nullptr;
    if (nant == 1) {
      newest_row<1>(p, c, p.noise_dev.v ? noise_avg(p.noise_dev) : c.noise, s.row, dbg_d);
    } else if (nant == 2) {
      newest_row<2>(p, c, 0.f, s.row, dbg_d);
    } else {
      newest_row<4>(p, c, 0.f, s.row, dbg_d);
    }
    __syncthreads();
    if (cmb == 0) {
      float* keep = nant == c.last_nant ? p.newest + c.o_new : nullptr; // (c)
      float* dbg  = p.dbg_llr ? p.dbg_llr + (size_t)slot * pbch_map::kMaxBits : nullptr;
      for (uint32_t i = lane; i < nof_bits; i += 64) {
        if (keep) {
          keep[i] = s.row[i];
        }
        if (dbg) {
          dbg[i] = s.row[i];
        }
      }
    }
  } else {
    __syncthreads();
  }
  // (b)
  const float*   hist = p.hist + c.o_hist;
  const uint32_t own  = nant != 0 ? f - 1 : 4; // the row that is the wave's own
  const auto     temp = [&](uint32_t k) {
    const uint32_t r = k / nof_bits, w = k - r * nof_bits;
    if (r < dst || r >= dst + n) {
      return 10000.f;
    }
    const uint32_t from = src + r - dst;
    const float    v    = from == own ? s.row[w] : hist[from * nof_bits + w];
    return ((s.seq[k >> 5] >> (k & 31u)) & 1u) ? -v : v;
  };
  conv::rm_conv_wave(temp, 4 * nof_bits, kBits, s.rm);
  const float scale = (float)(1.0 / (double)(float)(2 * n));
  float       mx    = 1e-9f;
  for (uint32_t o = lane; o < pbch_map::kCoded; o += 64) { // the lane's own positions
    const float t = rn_mul(s.rm[o], scale);
    s.rm[o]       = t;
    mx            = fmaxf(mx, fabsf(t));
  }
  const float gain = 1000.f / conv::wave_max(mx);
  for (uint32_t o = lane; o < pbch_map::kCoded; o += 64) {
    const uint16_t q = conv::quant_fus(gain, s.rm[o]);
    s.sym[o]         = q;
    if (p.dbg_rm) {
      p.dbg_rm[(size_t)blockIdx.x * pbch_map::kCoded + o] = s.rm[o];
    }
    if (p.dbg_sym) {
      p.dbg_sym[(size_t)blockIdx.x * pbch_map::kCoded + o] = q;
    }
  }
  __syncthreads();
  uint8_t* out = p.rows + (size_t)blockIdx.x * kOutRow;
  conv::viterbi_wave(s.sym, kBits, true, s.words, out, s.bits);
  __syncthreads();
  if (lane == 0) {
    const uint32_t rem  = conv::crc_rem(s.bits, pbch_map::kPayload);
    uint32_t       ones = 0;
    for (uint32_t i = 0; i < pbch_map::kPayload; i++) {
      ones += s.bits[i];
    }
    out[kBits]     = (uint8_t)(rem & 0xFFu);
    out[kBits + 1] = (uint8_t)(rem >> 8);
    out[kBits + 2] = (uint8_t)ones;
    out[kBits + 3] = 0;
    out[kBits + 4] = out[kBits + 5] = out[kBits + 6] = out[kBits + 7] = 0;
  }
}

} // namespace

hipError_t launch(const Params& p, hipStream_t st)
{
  if (p.n_jobs == 0 || p.n_jobs > kMaxJobs || !p.cells || !p.jobs || !p.hist || !p.seq || !p.rows || !p.newest) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(pbch_kernel, dim3(p.n_jobs), dim3(64), 0, st, p);
  return hipGetLastError();
}

} // namespace pbch
} // namespace phyhip
