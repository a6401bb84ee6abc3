// pss_wave_kernels.hip -- PSS correlation (pss.c:446-534, convolution.c:113-120), one WAVE per overlap-save block.
//
// The arithmetic plan (sync_kernels.hip): 4096-point overlap-save blocks, the block is transformed once, multiplied by the
// cached spectrum of each N_id_2 replica, transformed back, |.|^2 (+ the moving average of pss.c:496-503), block arg-max.
// Where the transform lives:
//   * 4096 = 64 x 64.  Lane l of ONE wave holds the 64 points n = l + 64 r in registers and runs a complete 64-point
//     FFT on them without talking to anybody (8 x 8, all indices and inner twiddles compile-time constants); one
//     multiplication by W_4096^(l k), ONE 64 x 64 transposition through LDS (wave-private: no barrier, 65-element rows:
//     no bank conflict), and a second register FFT gives X[l + 64 k] -- the layout the block was loaded in.  A 4096-point
//     transform therefore costs one LDS round trip instead of the two workgroup-wide exchanges + barriers of the
//     three-pass radix-16 engine, and nothing waits for another wave.
//   * complex numbers are two plain f32 registers; +-i is a renaming of registers, a complex multiplication two v_mul + two v_fma.
//     (The first version ran on the packed f32 pipe, one instruction per complex addition: slower, see `cx` in fft_reg.h; the file is
//     compiled without the SLP vectoriser so that it stays unpacked, srslte_amd/build.py.)
//   * TWO waves per SIMD (235 registers): a wave issues at most one vector instruction per four cycles, the SIMD takes one per
//     two, and a lone wave stands still through every memory wait.  The spectrum of the block serves three hypotheses but does not
//     fit next to the transform's working set at that occupancy: it is parked in global memory in between (pss_wave_kernel).
//   * every global access is 512 contiguous bytes per wave instruction (capture, filter spectra, parked spectrum, correlation row);
//     block borders, the zero padding of the convolution and the ragged last block are the bounds checks of buffer instructions.
#include "fft_reg.h"
#include "hip_common.h"
#include "sync_device.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace phyhip {
namespace sync {

using namespace regfft;

// 4096-point transform of one wave: v[r] of lane l = element l + 64 r, in and out.  T1[b] = W^(l b), T2[a] = W^(8 l a),
// W = e^{-2 pi i / 4096}; `img` = the wave's 64 x 65 LDS image of floats: real and imaginary parts cross it one after the other
// (16.6 KB per wave, so that eight waves fit a CU; LDS operations of one wave execute in order, no barrier is involved).
template <bool INV>
static __device__ __forceinline__ void fft4096_first(cx (&v)[64], const cx (&T1)[8], const cx (&T2)[8], float* img, int lane) // ... up to the transposition
{
  fft64<INV>(v);
#pragma unroll
  for (int k = 0; k < 64; k++) {
    if (k != 0) {
      const cx w = (k & 7) == 0 ? T2[k >> 3] : ((k >> 3) == 0 ? T1[k & 7] : cmul2<false>(T2[k >> 3], T1[k & 7]));
      v[k]       = cmul2<INV>(v[k], w);
    }
    img[k * 65 + lane] = v[k].x;
    if ((k & 7) == 7) {
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int n = 0; n < 64; n++) {
    v[n].x = img[lane * 65 + n];
  }
  __builtin_amdgcn_sched_barrier(0); // (the LDS operations of a wave execute in issue order: every read above precedes every write below)
#pragma unroll
  for (int k = 0; k < 64; k++) {
    img[k * 65 + lane] = v[k].y;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int n = 0; n < 64; n++) {
    v[n].y = img[lane * 65 + n];
  }
  __builtin_amdgcn_sched_barrier(0);
}
template <bool INV>
static __device__ __forceinline__ void fft4096(cx (&v)[64], const cx (&T1)[8], const cx (&T2)[8], float* img, int lane)
{
  fft4096_first<INV>(v, T1, T2, img, lane);
  fft64<INV>(v);
}

// One wave per overlap-save block and TWO waves per SIMD: a lone wave issues one vector instruction every four cycles, half of what
// the SIMD takes, and stands still through every memory wait.  Two need <= 256 registers each, which leaves no room for the
// block's spectrum next to the transform's working set -- it waits in global memory (see below).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void pss_wave_kernel(const PssParams p)
{
  __shared__ float img[64 * 65];
  const int        cap = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x;
  const cx*        x   = reinterpret_cast<const cx*>(p.in) + (size_t)cap * p.in_stride;
  const cx*        tw  = reinterpret_cast<const cx*>(p.twiddle);

  cx T1[8], T2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { // (the host stores these behind the 4096 twiddles in [entry][lane] order)
    T1[j] = tw[4096 + 64 * j + lane];
    T2[j] = tw[4096 + 64 * (8 + j) + lane];
  }

  const int i0  = blk * p.hop;           // first convolution output of this block
  const int off = i0 - (p.fft_size - 1); // capture index of segment element 0
  // the capture as a raw buffer: elements before its start (negative offsets wrap to huge ones) and behind its end read as zero,
  // which is the zero padding of the convolution -- no compare, no branch
  const __amdgpu_buffer_rsrc_t xb = __builtin_amdgcn_make_buffer_rsrc(const_cast<cx*>(x), 0, p.frame_size * 8, 0x00020000);

  const int m_lo = p.fft_size - 1, m_hi = p.fft_size - 1 + p.hop;
  bool      have_spec = false;
  for (int h = 0; h < 3; h++) {
    if (!(p.n_id_2_mask & (1 << h))) {
      continue;
    }
    // Nothing below may look loop-invariant: hoisted out of the hypothesis loop, the 64 twiddle products, the 64 output offsets and
    // the 64 row predicates are several hundred registers that stay live across the whole loop.  Passing the lane index, the twiddle
    // tables and the bounds through an empty asm makes them values of this iteration.
    int lane_h = lane, m_lo_h = m_lo;
    asm volatile("" : "+v"(lane_h), "+s"(m_lo_h));
#pragma unroll
    for (int j = 0; j < 8; j++) {
      asm volatile("" : "+v"(T1[j].x), "+v"(T1[j].y), "+v"(T2[j].x), "+v"(T2[j].y)); // (in place: no second copy of the tables)
    }
    cx        v[64];
    const cx* filt = reinterpret_cast<const cx*>(p.filt) + (size_t)h * 4096 + lane_h;
    cx        f[16];
    // The filter spectrum of a hypothesis comes in batches of 16 values.  (Fenced: short of registers, the compiler otherwise issues one
    // load, waits for it, uses it -- 64 L2 round trips in a row per hypothesis: 1.3 of 2.8 ms per 256 captures.)
    cx* spec = reinterpret_cast<cx*>(p.spec) + ((size_t)cap * p.n_blocks + blk) * 4096 + lane_h;
    if (!have_spec) {
#pragma unroll
      for (int r = 0; r < 64; r++) {
        v[r] = __builtin_bit_cast(cx, __builtin_amdgcn_raw_buffer_load_b64(xb, (off + lane_h + 64 * r) * 8, 0, 0));
      }
      fft4096_first<false>(v, T1, T2, img, lane_h);
      // the first batch is requested before the second half of the forward transform and arrives under it
#pragma unroll
      for (int j = 0; j < 16; j++) {
        f[j] = filt[64 * j];
      }
      __builtin_amdgcn_sched_barrier(0);
      fft64<false>(v);
      __builtin_amdgcn_sched_barrier(0);
      // The spectrum of the block serves every hypothesis, but two waves per SIMD have no registers to keep it (and one wave per SIMD
      // issues at half rate): it is parked in the block's 32 KB of the spectrum area and comes back from L2 / the Infinity Cache in
      // place of the block itself -- the same 64 loads the forward transform would start with, and no second and third transform.
      // (Requesting it row by row while the previous hypothesis is post-processed, into the registers that become free, was built too:
      // the values carried around the loop cost 100 spilled registers and the kernel took 2.3 instead of 1.4 ms.)
      if ((p.n_id_2_mask >> (h + 1)) != 0) {
#pragma unroll
        for (int r = 0; r < 64; r++) {
          spec[64 * r] = v[r];
        }
      }
      have_spec = true;
    } else {
#pragma unroll
      for (int r = 0; r < 64; r++) {
        v[r] = spec[64 * r];
      }
#pragma unroll
      for (int j = 0; j < 16; j++) {
        f[j] = filt[64 * j];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int g = 0; g < 4; g++) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        v[16 * g + j] = cmul2<false>(v[16 * g + j], f[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (g < 3) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
          f[j] = filt[64 * (16 * (g + 1) + j)];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // (the inverse transform wants the same 64 twiddle products as the forward one: common-subexpression elimination would keep all
    // of them alive in between -- 128 registers; the tables go through the empty asm again instead)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      asm volatile("" : "+v"(T1[j].x), "+v"(T1[j].y), "+v"(T2[j].x), "+v"(T2[j].y));
    }
    fft4096<true>(v, T1, T2, img, lane_h);

    // the correlation row as a raw buffer of n_out floats: lanes outside the block's share get an offset beyond it, and the
    // hardware drops their stores (and returns zero for their loads)
    const __amdgpu_buffer_rsrc_t cb =
        __builtin_amdgcn_make_buffer_rsrc(p.corr + ((size_t)cap * 3 + h) * p.corr_stride, 0, p.n_out * 4, 0x00020000);
    float best  = -1.0f;
    int   besti = 0x7fffffff;
    auto  post  = [&](auto ema_tag) {
      constexpr bool EMA = decltype(ema_tag)::value;
#pragma unroll
      for (int r = 0; r < 64; r++) {
        if (64 * r + 63 < m_lo_h) { // wave-uniform: the whole register row lies in the discarded head of the block
          continue;
        }
        const int  m = lane_h + 64 * r, i = off + m;
        const bool ok = m >= m_lo_h && m < m_hi && i < p.n_out;
        const int  bo = ok ? i * 4 : -1;
        float      pw = v[r].x * v[r].x + v[r].y * v[r].y; // srsran_vec_abs_square_cf
        if (EMA) {
          const float old = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(cb, bo, 0, 0));
          pw              = pw * p.ema_alpha + old * (1.0f - p.ema_alpha); // pss.c:497-500
        }
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pw), cb, bo, 0, 0);
        const bool gt = ok && pw > best; // i grows with r: the first maximum of the lane stays
        best          = gt ? pw : best;
        besti         = gt ? i : besti;
      }
    };
    if (p.ema_alpha > 0.0f && p.ema_alpha < 1.0f) {
      post(std::true_type{});
    } else {
      post(std::false_type{});
    }
    // block arg-max (first maximum wins on ties, as srsran_vec_max_fi)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob  = __shfl_down(best, o);
      const int   obi = __shfl_down(besti, o);
      if (ob > best || (ob == best && obi < besti)) {
        best  = ob;
        besti = obi;
      }
    }
    if (lane == 0) {
      const size_t o = ((size_t)cap * 3 + h) * p.n_blocks + blk;
      p.part_val[o]  = best;
      p.part_idx[o]  = besti;
    }
  }
}

hipError_t launch_pss_wave_blocks(const PssParams& p, hipStream_t stream)
{
  hipLaunchKernelGGL(pss_wave_kernel, dim3(p.n_blocks, p.n_cap), dim3(64), 0, stream, p);
  return hipGetLastError();
}

} // namespace sync
} // namespace phyhip
