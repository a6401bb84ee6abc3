// turbo_layout.h -- how the throughput window decoder (turbo_kernels.hip) keeps its per-wave workspace in HBM, and the loads / stores of that
// layout: blocked arrays, row arrays, their 8-bit storage forms and the exchange across the lanes of a code block.  Device code, but for the
// exchange-table entry's encoding, which the host's table builder shares.
#pragma once
#include "turbo_arith.h"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace phyhip {
namespace turbo {

// Non-temporal workspace loads (NT): nothing the fixed-iteration 16-bit decoder reads is read again before several hundred KB per
// wave have passed, so keeping it in L2 only evicts lines that are still being written.  Measured on one box (K = 6144, 65,520 blocks,
// 8 half iterations): 12.03 ms without, 11.81 ms with the systematic / parity operands non-temporal, 11.74 ms with the exchanged rows
// too, 11.58 ms with the check-points as well; non-temporal STORES cost (12.2 ms).  The 8-bit decoders (14.7 -> 15.8 ms) and the
// early-stop mode (-2.5 % on the transport-block benches) lose with it -- their smaller, partly re-touched working sets do hit in L2 --
// so NT = fixed iterations and int16 only.
// One stream of that decoder is read again soon enough: the lowest blocks of the backward main pass, which the forward main pass takes up once the wave has
// turned round.  Those requests use the default policy (WinParams::reuse_blocks; turbo_kernels.hip, the whole-block loop of the backward pass), and the
// second read is in part served by the L2 (2.2 % fewer bytes leave it): 18.79 -> 18.41 ms per step of the headline benchmark.  The exchanged rows alone stored non-temporally: 18.79 -> 19.37 ms.
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 ws_load16(const void* p)
{
  if constexpr (NT) {
    const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const uint4*>(p);
  }
}

// Blocked arrays hold, per 8-step block and lane, 8 dwords.  They are stored as two half-blocks of 4 dwords so
// that each dwordx4 access of a wave covers one contiguous 1 KB (measured: 5.5 TB/s against 4.5 TB/s for a
// 32-byte-per-lane layout where every 128-byte line is touched by two instructions).
template <bool NT = false>
__device__ __forceinline__ void load_block(const uint32_t* arr, uint32_t blk_lane, uint32_t (&r)[8])
{
  const uint32_t blk = blk_lane >> 6, ln = blk_lane & 63u;
  unpack8(ws_load16<NT>(arr + ((size_t)(blk * 2) * 64 + ln) * 4), ws_load16<NT>(arr + ((size_t)(blk * 2 + 1) * 64 + ln) * 4), r);
}

__device__ __forceinline__ void store_block(uint32_t* arr, uint32_t blk_lane, const uint32_t (&r)[8])
{
  const uint32_t blk = blk_lane >> 6, ln = blk_lane & 63u;
  *reinterpret_cast<uint4*>(arr + ((size_t)(blk * 2) * 64 + ln) * 4)     = make_uint4(r[0], r[1], r[2], r[3]);
  *reinterpret_cast<uint4*>(arr + ((size_t)(blk * 2 + 1) * 64 + ln) * 4) = make_uint4(r[4], r[5], r[6], r[7]);
}

// exchange tables: 8 dwords per (block, lane of the code block), contiguous
__device__ __forceinline__ void load_lut(const uint32_t* arr, uint32_t idx, uint32_t (&r)[8])
{
  const uint4* q = reinterpret_cast<const uint4*>(arr + (size_t)idx * 8);
  unpack8(q[0], q[1], r);
}

// Blocked int16 index of trellis step k of sub-block d (LPC lanes per code block)
template <int LPC>
__host__ __device__ __forceinline__ uint32_t elem_index(uint32_t k, uint32_t d)
{
  return ((((k >> 3) * LPC + (d >> 1)) * 8 + (k & 7)) << 1) + (d & 1);
}

// Rows of the 64/LPC code blocks of a wave are interleaved: row k of the wave is 64 contiguous dwords.
// The 8 rows of block b are fetched with TWO dwordx4 per lane (the 2 KB of rows 8b..8b+7 are contiguous): dword-per-lane
// loads top out near 3 TB/s on this part, 16-byte ones reach 5.5 TB/s.  Lane L then holds columns 4(L%16)..+3
// of rows L/16 and 4 + L/16; rows_to_lane() turns that into "8 rows of column L" through a 2 KB LDS image.
template <bool NT = false>
__device__ __forceinline__ void issue_rows(const uint32_t* arr, uint32_t b, int lane, uint32_t (&t)[8])
{
  const uint4* q = reinterpret_cast<const uint4*>(arr + (size_t)(b * 8) * 64) + lane;
  unpack8(ws_load16<NT>(q), ws_load16<NT>(q + 64), t);
}

__device__ __forceinline__ void rows_to_lane(uint32_t* stage, int lane, const uint32_t (&t)[8], uint32_t (&r)[8])
{
  // one wave per workgroup and the LDS pipeline is in order: no barrier between the write and the read
  reinterpret_cast<uint4*>(stage)[lane]      = make_uint4(t[0], t[1], t[2], t[3]);
  reinterpret_cast<uint4*>(stage)[64 + lane] = make_uint4(t[4], t[5], t[6], t[7]);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r[j] = stage[j * 64 + lane];
  }
}

// ---- storage policy.  The 16-bit decoders keep one int16x2 dword per (lane, step) in the workspace.  The 8-bit decoders' values are
// int8 by construction (in registers: value << 8 in each int16 half, low bytes zero -- see Ar8), so their workspace holds ONE 16-bit
// word per (lane, step): half the HBM traffic of a kernel that runs at the HBM ceiling.  S8 = AR::kIs8 selects the layout:
//   blocked arrays (S, P0, P1, check-points): 8 steps of a lane = 16 bytes = ONE dwordx4 (1 KB contiguous per wave instruction)
//   row arrays (A1, A2, D): a row of the wave = 64 x 2 bytes; the 8 rows of a block are 1 KB = ONE dwordx4 per lane
// Loads stay PACKED in the prefetch registers (4 dwords instead of 8 per operand block) and are widened where they are consumed:
// one v_perm_b32 per step puts the two bytes into the high bytes of the halves; one v_perm_b32 packs two steps for a store.
__device__ __forceinline__ uint32_t s8_unpack_lo(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x010c000cu); } // bytes 0, 1
__device__ __forceinline__ uint32_t s8_unpack_hi(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x030c020cu); } // bytes 2, 3
__device__ __forceinline__ uint32_t s8_pack2(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07050301u); } // (a.b1, a.b3, b.b1, b.b3)
__device__ __forceinline__ uint16_t s8_pack1(uint32_t a) { return (uint16_t)__builtin_amdgcn_perm(0u, a, 0x0c0c0301u); }

// raw (as stored) form of one 8-step block of a blocked array: 8 dwords, or 4 with 8-bit storage
template <bool S8, bool NT = false>
__device__ __forceinline__ void load_block_raw(const uint32_t* arr, uint32_t blk_lane, uint32_t (&r)[8])
{
  if constexpr (S8) {
    unpack4(ws_load16<NT>(arr + (size_t)blk_lane * 4), r);
  } else {
    load_block<NT>(arr, blk_lane, r);
  }
}
// raw -> the 8 int16x2 values of the block
template <bool S8>
__device__ __forceinline__ void block_values(const uint32_t (&raw)[8], uint32_t (&v)[8])
{
#pragma unroll
  for (int d = 0; d < 4; d++) {
    v[2 * d]     = S8 ? s8_unpack_lo(raw[d]) : raw[2 * d];
    v[2 * d + 1] = S8 ? s8_unpack_hi(raw[d]) : raw[2 * d + 1];
  }
}
template <bool S8>
__device__ __forceinline__ void store_block_v(uint32_t* arr, uint32_t blk_lane, const uint32_t (&v)[8])
{
  if constexpr (S8) {
    *reinterpret_cast<uint4*>(arr + (size_t)blk_lane * 4) = make_uint4(s8_pack2(v[0], v[1]), s8_pack2(v[2], v[3]), s8_pack2(v[4], v[5]), s8_pack2(v[6], v[7]));
  } else {
    store_block(arr, blk_lane, v);
  }
}
// the 8 rows of block b of a row array, as stored: two dwordx4 per lane, or one with 8-bit storage
template <bool S8, bool NT = false>
__device__ __forceinline__ void issue_rows_raw(const uint32_t* arr, uint32_t b, int lane, uint32_t (&t)[8])
{
  if constexpr (S8) {
    unpack4(ws_load16<NT>(reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(arr) + (size_t)(b * 8) * 64) + lane), t);
  } else {
    issue_rows<NT>(arr, b, lane, t);
  }
}
// ... turned into "8 rows of this lane's column" (int16x2 values) through the LDS stage
template <bool S8>
__device__ __forceinline__ void rows_to_lane_v(uint32_t* stage, int lane, const uint32_t (&t)[8], uint32_t (&r)[8])
{
  if constexpr (S8) {
    reinterpret_cast<uint4*>(stage)[lane] = make_uint4(t[0], t[1], t[2], t[3]); // in-order LDS pipeline, one wave per workgroup: no barrier
    const uint16_t* s16 = reinterpret_cast<const uint16_t*>(stage);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      r[j] = s8_unpack_lo((uint32_t)s16[j * 64 + lane]);
    }
  } else {
    rows_to_lane(stage, lane, t, r);
  }
}
// one element of a row array: (row, lane) <- int16x2 value
template <bool S8>
__device__ __forceinline__ void store_row(uint32_t* arr, size_t row, int lane, uint32_t v)
{
  if constexpr (S8) {
    reinterpret_cast<uint16_t*>(arr)[row * 64 + lane] = s8_pack1(v);
  } else {
    arr[row * 64 + lane] = v;
  }
}

// ---- exchange-table entries: one dword per (trellis step, destination lane of the code block), built once per (K, sub-blocks) by the
// host (turbo_host.cpp) and decoded by every window kernel through the helpers below -- nothing else knows the layout.  Every field sits
// where the instruction that consumes it wants it, so a step's exchange costs no index arithmetic:
//   bit  1      the value for the LOW destination sub-block is the HIGH half of its source lane's dword   } the flag bits of a
//   bit  17     the same for the HIGH destination sub-block                                              } v_perm_b32 selector
//   bits 2..5   4 x the lane (within the code block) holding the source of the low destination sub-block: OR-ed with the byte address of
//               the code block's first lane it is the ds_bpermute address (one v_and_or_b32)
//   byte 1      4 x the lane holding the source of the high destination sub-block, nothing else: one byte-selecting OR
//   bits 22..31 destination row (a shift)
// The other bits are zero.  Sub-block j lives in half j & 1 of lane j >> 1 of the code block.
constexpr uint32_t kXchRowBits = 10, kXchLaneBits = 4; // rows < 1024 (K = 6144 in 8 sub-blocks: 768), at most 16 lanes per code block
__host__ __device__ __forceinline__ uint32_t xch_pack(uint32_t row, uint32_t src_lo, uint32_t src_hi)
{
  return ((src_lo & 1u) << 1) | ((src_lo >> 1) << 2) | ((src_hi >> 1) << 10) | ((src_hi & 1u) << 17) | (row << 22);
}
__host__ __device__ __forceinline__ bool xch_fits(uint32_t rows, uint32_t sub_blocks)
{
  return rows <= (1u << kXchRowBits) && sub_blocks <= (2u << kXchLaneBits);
}
__host__ __device__ __forceinline__ uint32_t xch_row(uint32_t e) { return e >> 22; }
__host__ __device__ __forceinline__ uint32_t xch_lane4_lo(uint32_t e) { return e & 0x3cu; }        // 4 x source lane, low sub-block
__host__ __device__ __forceinline__ uint32_t xch_lane4_hi(uint32_t e) { return (e >> 8) & 0xffu; } // 4 x source lane, high sub-block
__host__ __device__ __forceinline__ uint32_t xch_src_lo(uint32_t e) { return (xch_lane4_lo(e) >> 1) | ((e >> 1) & 1u); } // source sub-blocks,
__host__ __device__ __forceinline__ uint32_t xch_src_hi(uint32_t e) { return (xch_lane4_hi(e) >> 1) | ((e >> 17) & 1u); } // as packed
// a, c: the dwords of the two source lanes -> the chosen half of each, in ONE v_perm_b32 (selector bytes 0|2, 1|3 pick from a, 4|6, 5|7 from c)
__device__ __forceinline__ uint32_t xch_merge(uint32_t a, uint32_t c, uint32_t e)
{
  return __builtin_amdgcn_perm(c, a, (e & 0x00020002u) * 0x101u + 0x05040100u);
}

// byte address (ds_bpermute) of the first lane of this lane's code block
template <int LPC>
__device__ __forceinline__ uint32_t xch_group_base(int lane)
{
  return (uint32_t)(lane & ~(LPC - 1)) << 2;
}
// value for this lane's two destination sub-blocks, fetched from the lanes holding the source sub-blocks
__device__ __forceinline__ uint32_t permute_pair(uint32_t v, uint32_t e, uint32_t group_base)
{
  const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(xch_lane4_lo(e) | group_base), (int)v);
  // (xch_lane4_hi(e) | group_base in one instruction: the compiler forms shift + v_and_or_b32, which has no byte-selecting form)
  uint32_t addr_c;
  asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(addr_c) : "v"(e), "v"(group_base));
  const uint32_t c = (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr_c, (int)v);
  return xch_merge(a, c, e);
}
// one element of a row array, the row taken from an exchange-table entry (own: the early-stop mask of the row index, ~0 without)
template <bool S8>
__device__ __forceinline__ void store_xch_row(uint32_t* arr, uint32_t e, uint32_t own, int lane, uint32_t v)
{
  // a 32-bit byte offset from the (wave-uniform) array: the store takes the array from scalar registers, no 64-bit vector address is formed
  if constexpr (S8) {
    const uint32_t off = ((xch_row(e) & own) << 7) | ((uint32_t)lane << 1);
    *reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(arr) + off) = s8_pack1(v);
  } else {
    const uint32_t off = ((xch_row(e) & own) << 8) | ((uint32_t)lane << 2);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(arr) + off) = v;
  }
}

} // namespace turbo
} // namespace phyhip
