// turbo_extract.h -- phase 0 of the throughput window decoder (turbo_kernels.hip): the input LLRs of a wave's code blocks, from any of the
// layouts the callers hand over, into the blocked systematic / parity arrays and the tail LLRs of the workspace.  Device code only.
#pragma once
#include "turbo_arith.h"
#include "turbo_layout.h"

namespace phyhip {
namespace turbo {

// the twelve tail LLRs of a code block, by stream; they start at in[tb], behind the block's 3 K (sub-block layout: 3 (K + 32)) values.  One lane per code block
template <class AR, typename T>
__device__ __forceinline__ void extract_tails(const T* in, uint32_t tb, short* TL)
{
#pragma unroll
  for (int i = 0; i < 3; i++) {
    TL[i]     = AR::conv_in(in[tb + 2 * i]);         // syst tail
    TL[3 + i] = AR::conv_in(in[tb + 2 * i + 1]);     // parity0 tail
    TL[6 + i] = AR::conv_in(in[tb + 6 + 2 * i]);     // app2 tail
    TL[9 + i] = AR::conv_in(in[tb + 6 + 2 * i + 1]); // parity1 tail
  }
}

// phase 0: input extraction (turbodecoder_win.h:888-930 / turbodecoder_iter.h:58-70,88-102) from int16 or int8
// LLRs.  All 48 element loads of an 8-step block are issued before the first use (addresses clamped instead
// of branching on the ragged last block), so the block costs one memory round trip, not eight.
template <int LPC, class AR, typename T>
__device__ __forceinline__ void extract_input(const T* in, int sb_layout, uint32_t K, uint32_t long_sb, uint32_t nblk,
                                              int lane, int pl, uint32_t* S, uint32_t* P0, uint32_t* P1, short* TL,
                                              uint32_t b_first = 0, bool tails = true)
{
  constexpr int NB = 2 * LPC;
  for (uint32_t b = b_first; b < nblk; b++) {
    const int nv = (int)(long_sb - b * 8) < 8 ? (int)(long_sb - b * 8) : 8; // valid steps in this block
    short     r[2][24];
    if (sb_layout) {
      // rm_turbo layout: element (step k, sub-block d) of array a at in[a*(K+32) + k*NB + d]
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint32_t k = b * 8 + (j < nv ? j : nv - 1);
#pragma unroll
        for (int a3 = 0; a3 < 3; a3++) {
          r[0][3 * j + a3] = AR::conv_in(in[a3 * (K + 32) + k * NB + 2 * pl]);
          r[1][3 * j + a3] = AR::conv_in(in[a3 * (K + 32) + k * NB + 2 * pl + 1]);
        }
      }
    } else {
      // natural order: the 8 steps of one sub-block are 24 consecutive LLRs [s p0 p1]...
      const T*  c0  = in + 3 * ((size_t)(2 * pl) * long_sb + b * 8);
      const T*  c1  = in + 3 * ((size_t)(2 * pl + 1) * long_sb + b * 8);
      const int lim = 3 * nv - 1;
#pragma unroll
      for (int t = 0; t < 24; t++) {
        const int tt = t < lim ? t : lim;
        r[0][t]      = AR::conv_in(c0[tt]);
        r[1][t]      = AR::conv_in(c1[tt]);
      }
    }
    uint32_t s[8], y0[8], y1[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      s[j]  = (uint32_t)(uint16_t)r[0][3 * j] | ((uint32_t)(uint16_t)r[1][3 * j] << 16);
      y0[j] = (uint32_t)(uint16_t)r[0][3 * j + 1] | ((uint32_t)(uint16_t)r[1][3 * j + 1] << 16);
      y1[j] = (uint32_t)(uint16_t)r[0][3 * j + 2] | ((uint32_t)(uint16_t)r[1][3 * j + 2] << 16);
    }
    store_block_v<AR::kIs8>(S, b * 64 + lane, s);
    store_block_v<AR::kIs8>(P0, b * 64 + lane, y0);
    store_block_v<AR::kIs8>(P1, b * 64 + lane, y1);
  }
  if (pl == 0 && tails) {
    extract_tails<AR>(in, sb_layout ? 3 * (K + 32) : 3 * K, TL);
  }
}

// Fast input extraction for natural-order int16 LLRs [s p0 p1]xK (what srsran_tdec_run_all gets with
// srsran_tdec_force_not_sb): the stream is sub-block major (the 3W LLRs of a sub-block are contiguous) while the
// decoder wants step-major data spread over lanes, so every code block of the wave is staged through LDS in chunks of
// NBK 8-step blocks: the 64 lanes copy the NB contiguous runs of 48*NBK bytes with 8-byte loads (each wave-level load
// covers >= 256 contiguous bytes), then lane (p', g) assembles the blocked dwords of sub-block pair p' for two blocks
// and stores them into the slots of the lane that owns that pair.  Needs W % 4 == 0 and 8-byte aligned code blocks.
template <int LPC, class AR>
__device__ __forceinline__ void extract_input_natural16(const short* in_wave, uint32_t in_stride, int n_cb_left, uint32_t K,
                                                        uint32_t long_sb, uint32_t nblk, int lane, uint32_t* S, uint32_t* P0,
                                                        uint32_t* P1, short* TL_wave, uint2* stage)
{
  constexpr int NB  = 2 * LPC;
  constexpr int CPW = 64 / LPC;
  constexpr int NBK = 256 / NB;  // blocks per chunk: NB runs of 48*NBK bytes = 12 KB of LDS
  constexpr int RS  = 6 * NBK + 1; // run stride in the LDS image, in 8-byte units (+1: spreads the LDS banks)
  const int     pp  = lane % LPC, g = lane / LPC;
  // chunks are (code block, block range) pairs; the loads of the next chunk are in flight while the current one is
  // re-distributed (24 8-byte loads per lane and chunk: NB * 6 * NBK / 64)
  constexpr int NLD = NB * 6 * NBK / 64;
  const uint32_t nchunk = (nblk + NBK - 1) / NBK, total = CPW * nchunk;
  auto chunk_src = [&](uint32_t c, const short*& in, uint32_t& b0, int& nbt) {
    const int cw = (int)(c % CPW); // block range outermost: the 8 code blocks' 128-byte pieces of a 1 KB line are written back to back
    in           = in_wave + (size_t)(cw < n_cb_left ? cw : n_cb_left - 1) * in_stride;
    b0           = (c / CPW) * NBK;
    nbt          = (int)(nblk - b0) < NBK ? (int)(nblk - b0) : NBK;
  };
  auto issue_chunk = [&](uint32_t c, uint2(&rg)[NLD]) {
    const short* in;
    uint32_t     b0;
    int          nbt;
    chunk_src(c, in, b0, nbt);
    if (nbt == NBK) { // full chunk: the run length is a compile-time constant (no integer division by a variable)
      constexpr int rl = 6 * NBK;
#pragma unroll
      for (int t = 0; t < NLD; t++) {
        const int i = t * 64 + lane, d = i / rl, o = i - d * rl;
        rg[t]       = *(reinterpret_cast<const uint2*>(in + 3 * ((size_t)d * long_sb + (size_t)b0 * 8)) + o);
      }
    } else {
      const int rl = 6 * nbt; // run length in 8-byte units
#pragma unroll
      for (int t = 0; t < NLD; t++) {
        const int i = t * 64 + lane;
        if (i < NB * rl) {
          const int d = i / rl, o = i - d * rl;
          rg[t]       = *(reinterpret_cast<const uint2*>(in + 3 * ((size_t)d * long_sb + (size_t)b0 * 8)) + o);
        }
      }
    }
  };
  uint2 rg[NLD];
  issue_chunk(0, rg);
  for (uint32_t c = 0; c < total; c++) {
    const short* in;
    uint32_t     b0;
    int          nbt;
    chunk_src(c, in, b0, nbt);
    const int cw = (int)(c % CPW);
    if (nbt == NBK) {
      constexpr int rl = 6 * NBK;
#pragma unroll
      for (int t = 0; t < NLD; t++) {
        const int i = t * 64 + lane, d = i / rl, o = i - d * rl;
        stage[d * RS + o] = rg[t];
      }
    } else {
      const int rl = 6 * nbt;
#pragma unroll
      for (int t = 0; t < NLD; t++) {
        const int i = t * 64 + lane;
        if (i < NB * rl) {
          const int d = i / rl, o = i - d * rl;
          stage[d * RS + o] = rg[t];
        }
      }
    }
    if (c + 1 < total) {
      issue_chunk(c + 1, rg);
    }
    {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int lb = g * 2 + h; // NBK * LPC / 64 == 2 blocks per lane
        if (lb < nbt) {
          short r[2][24];
#pragma unroll
          for (int dd = 0; dd < 2; dd++) {
            const uint2* q = stage + (2 * pp + dd) * RS + lb * 6;
#pragma unroll
            for (int t = 0; t < 6; t++) {
              const uint2 v    = q[t];
              r[dd][4 * t]     = (short)(v.x & 0xffffu);
              r[dd][4 * t + 1] = (short)(v.x >> 16);
              r[dd][4 * t + 2] = (short)(v.y & 0xffffu);
              r[dd][4 * t + 3] = (short)(v.y >> 16);
            }
          }
          uint32_t sv[8], y0[8], y1[8];
#pragma unroll
          for (int j = 0; j < 8; j++) {
            sv[j] = (uint32_t)(uint16_t)AR::conv_in(r[0][3 * j]) | ((uint32_t)(uint16_t)AR::conv_in(r[1][3 * j]) << 16);
            y0[j] = (uint32_t)(uint16_t)AR::conv_in(r[0][3 * j + 1]) | ((uint32_t)(uint16_t)AR::conv_in(r[1][3 * j + 1]) << 16);
            y1[j] = (uint32_t)(uint16_t)AR::conv_in(r[0][3 * j + 2]) | ((uint32_t)(uint16_t)AR::conv_in(r[1][3 * j + 2]) << 16);
          }
          const uint32_t slot = (b0 + lb) * 64 + cw * LPC + pp;
          store_block_v<AR::kIs8>(S, slot, sv);
          store_block_v<AR::kIs8>(P0, slot, y0);
          store_block_v<AR::kIs8>(P1, slot, y1);
        }
      }
    }
  }
  // tail LLRs: lane cw * LPC of every code block
  if (pp == 0) {
    const short* in = in_wave + (size_t)(g < n_cb_left ? g : n_cb_left - 1) * in_stride;
    extract_tails<AR>(in, 3 * K, TL_wave + 16 * g);
  }
}

// Fast input extraction for the rm_turbo sub-block layout (int16): element (step k, sub-block d) of stream a sits at
// in[a (K+32) + k NB + d], i.e. the 8 steps of a block are 8 * NB contiguous int16 per code block and stream.  The LPC
// lanes of a code block fetch them with two dwordx4 each (128 contiguous bytes per code block and instruction) and the
// [step][sub-block pair] image is turned into "8 steps of pair p" through the 2 KB LDS stage.  Handles the `nblk` full
// 8-step blocks it is given (a ragged last block goes through extract_input); needs 16-byte aligned code blocks.
template <int LPC, class AR>
__device__ __forceinline__ void extract_input_sb16(const short* in, uint32_t K, uint32_t nblk, int lane, int pl, uint32_t* S,
                                                   uint32_t* P0, uint32_t* P1, short* TL, uint32_t* stage)
{
  constexpr int  NB  = 2 * LPC;
  const int      cbw = lane / LPC;
  uint4*         st4 = reinterpret_cast<uint4*>(stage);
  // one stream (systematic / parity 0 / parity 1) of one 8-step block: two 16-byte pieces per lane through the staging image
  auto put = [&](uint32_t* dst, uint32_t b, const uint4& lo, const uint4& hi) {
    st4[cbw * 2 * LPC + pl]       = lo;
    st4[cbw * 2 * LPC + LPC + pl] = hi;
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t w = stage[cbw * 8 * LPC + j * LPC + pl];
      r[j] = (uint32_t)(uint16_t)AR::conv_in((short)(w & 0xffffu)) | ((uint32_t)(uint16_t)AR::conv_in((short)(w >> 16)) << 16);
    }
    store_block_v<AR::kIs8>(dst, b * 64 + lane, r);
  };
  for (uint32_t b = 0; b < nblk; b++) {
    // all six loads of the block are issued before the first use (named registers: an indexed local array ends up in scratch)
    const uint4* q0 = reinterpret_cast<const uint4*>(in + (size_t)b * 8 * NB);
    const uint4* q1 = reinterpret_cast<const uint4*>(in + (size_t)(K + 32) + (size_t)b * 8 * NB);
    const uint4* q2 = reinterpret_cast<const uint4*>(in + (size_t)2 * (K + 32) + (size_t)b * 8 * NB);
    const uint4  s_lo = q0[pl], s_hi = q0[LPC + pl];
    const uint4  y_lo = q1[pl], y_hi = q1[LPC + pl];
    const uint4  z_lo = q2[pl], z_hi = q2[LPC + pl];
    put(S, b, s_lo, s_hi);
    put(P0, b, y_lo, y_hi);
    put(P1, b, z_lo, z_hi);
  }
  if (pl == 0) {
    extract_tails<AR>(in, 3 * (K + 32), TL);
  }
}

} // namespace turbo
} // namespace phyhip
