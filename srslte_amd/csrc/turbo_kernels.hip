// turbo_kernels.hip -- LTE turbo decoder (max-log-MAP SISO + QPP interleaver) for gfx950: the window decoders' throughput kernel.
//
// Bit-exact re-design of the decoders srsran_tdec_run_all() dispatches to on an AVX2 host
// (reference: lib/src/phy/fec/turbo/turbodecoder.c:381-408):
//   * window decoder, 16 sub-blocks  (turbodecoder_win.h, WINIMP_IS_AVX16)  K%16==0 && K>800
//   * window decoder,  8 sub-blocks  (turbodecoder_win.h, WINIMP_IS_SSE16)  K%8==0  && K>400
//   * scalar decoder                 (turbodecoder_gen.c)                   otherwise      -> turbo_gen_kernels.hip
//
// MI355X mapping (not the SIMD layout of the reference):
//   * one lane owns TWO adjacent sub-blocks of one code block, packed as int16x2 in one VGPR; all 8
//     trellis states of both live in 8 VGPRs -> the ACS recursion is v_pk_add_i16(clamp)/v_pk_max_i16
//     with no cross-lane traffic; a code block is 8 lanes (16 sub-blocks) or 4 lanes (8 sub-blocks),
//     a wave decodes 8 or 16 code blocks in lock step.
//   * state metrics of the backward recursion are NOT stored for every step (that is 16 B per
//     trellis step, 196 KB of HBM traffic per half iteration at K=6144): the beta pass keeps one
//     check-point per 8 steps and the forward pass re-derives the 7 steps in between into registers
//     (bit-identical because the normalisation schedule is replayed exactly).
//   * per-code-block vectors live in HBM in a blocked layout [step/8][lane][step%8] of int16x2, so a
//     lane fetches 8 trellis steps with two dwordx4 loads and 8 lanes of a block read 256 contiguous
//     bytes.
//   * extrinsic exchange (turbodecoder_iter.h:104-128) is fused into the forward pass: a-priori
//     subtraction on load, QPP scatter on store.
#include <type_traits>

#include "hip_common.h"
#include "turbo_arith.h"
#include "turbo_device.h"
#include "turbo_extract.h"
#include "turbo_layout.h"

namespace phyhip {
namespace turbo {

// one backward step, turbodecoder_win.h:626-652
template <class AR>
__device__ __forceinline__ void beta_step(s2 (&o)[8], s2 x, s2 y)
{
  auto adds = [](s2 a, s2 b) { return AR::add_raw(a, b); };
  s2   xy   = AR::add(x, y);
  s2 n0 = vmax(adds(o[4], xy), o[0]);
  s2 n1 = vmax(o[4], adds(o[0], xy));
  s2 n2 = vmax(adds(o[5], y), adds(o[1], x));
  s2 n3 = vmax(adds(o[5], x), adds(o[1], y));
  s2 n4 = vmax(adds(o[6], x), adds(o[2], y));
  s2 n5 = vmax(adds(o[6], y), adds(o[2], x));
  s2 n6 = vmax(o[7], adds(o[3], xy));
  s2 n7 = vmax(adds(o[7], xy), o[3]);
  o[0] = AR::clean(n0);
  o[1] = AR::clean(n1);
  o[2] = AR::clean(n2);
  o[3] = AR::clean(n3);
  o[4] = AR::clean(n4);
  o[5] = AR::clean(n5);
  o[6] = AR::clean(n6);
  o[7] = AR::clean(n7);
}

// one forward step, turbodecoder_win.h:753-826.  WITH_LLR: also max1-max0 using the beta of the next step.
template <class AR, bool WITH_LLR>
__device__ __forceinline__ s2 alpha_step(s2 (&o)[8], const s2 (&b)[8], s2 x, s2 y)
{
  auto adds = [](s2 a, s2 b) { return AR::add_raw(a, b); };
  s2   xy   = AR::add(x, y);
  s2 m_b[8], nw[8];
  m_b[0] = o[0];
  m_b[1] = adds(o[3], y);
  m_b[2] = adds(o[4], y);
  m_b[3] = o[7];
  m_b[4] = o[1];
  m_b[5] = adds(o[2], y);
  m_b[6] = adds(o[5], y);
  m_b[7] = o[6];
  nw[0] = adds(o[1], xy);
  nw[1] = adds(o[2], x);
  nw[2] = adds(o[5], x);
  nw[3] = adds(o[6], xy);
  nw[4] = adds(o[0], xy);
  nw[5] = adds(o[3], x);
  nw[6] = adds(o[4], x);
  nw[7] = adds(o[7], xy);
  s2 out = splat(0);
  if (WITH_LLR) {
    s2 m0 = adds(b[0], m_b[0]);
    s2 m1 = adds(b[0], nw[0]);
#pragma unroll
    for (int i = 1; i < 8; i++) {
      m0 = vmax(m0, adds(b[i], m_b[i]));
      m1 = vmax(m1, adds(b[i], nw[i]));
    }
    out = AR::llr(AR::clean(m1), AR::clean(m0));
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    o[i] = AR::clean(vmax(m_b[i], nw[i]));
  }
  return out;
}

// The forward warm-up leaves the operands of the last four blocks in this lane's slots of the beta buffer, slot s = 0 ... 3 for blocks
// nblk-4 ... nblk-1; the backward main pass takes them from there (tdec_win_unit says why)
__device__ __forceinline__ void keep_ops(uint4 (&Bl)[8][2][64], uint32_t s, int lane, const s2 (&xs)[8], const s2 (&ys)[8])
{
  Bl[2 * s][0][lane]     = make_uint4(to_u(xs[0]), to_u(xs[1]), to_u(xs[2]), to_u(xs[3]));
  Bl[2 * s][1][lane]     = make_uint4(to_u(xs[4]), to_u(xs[5]), to_u(xs[6]), to_u(xs[7]));
  Bl[2 * s + 1][0][lane] = make_uint4(to_u(ys[0]), to_u(ys[1]), to_u(ys[2]), to_u(ys[3]));
  Bl[2 * s + 1][1][lane] = make_uint4(to_u(ys[4]), to_u(ys[5]), to_u(ys[6]), to_u(ys[7]));
}
__device__ __forceinline__ void kept_ops(const uint4 (&Bl)[8][2][64], uint32_t s, int lane, s2 (&xs)[8], s2 (&ys)[8])
{
  const uint4 x0 = Bl[2 * s][0][lane], x1 = Bl[2 * s][1][lane], y0 = Bl[2 * s + 1][0][lane], y1 = Bl[2 * s + 1][1][lane];
  xs[0] = from_u(x0.x), xs[1] = from_u(x0.y), xs[2] = from_u(x0.z), xs[3] = from_u(x0.w);
  xs[4] = from_u(x1.x), xs[5] = from_u(x1.y), xs[6] = from_u(x1.z), xs[7] = from_u(x1.w);
  ys[0] = from_u(y0.x), ys[1] = from_u(y0.y), ys[2] = from_u(y0.z), ys[3] = from_u(y0.w);
  ys[4] = from_u(y1.x), ys[5] = from_u(y1.y), ys[6] = from_u(y1.z), ys[7] = from_u(y1.w);
}

// What the whole-block bodies of the forward main pass (tdec_win_unit, 16-step form) hand Ar16::normalize_if where a group lies at an end of the sub-block: 0 or
// ~0, the same in every lane, and opaque like sub_x there (a mask known to be 0 or ~0 is turned back into two arms).
__device__ __forceinline__ uint32_t norm_mask(bool on)
{
  uint32_t m = __builtin_amdgcn_readfirstlane(on ? ~0u : 0u); // (an "s" operand wants a value the compiler knows to be uniform)
  asm("" : "+s"(m)); // (not volatile: that would be a barrier for the LDS traffic of the steps around it)
  return m;
}

// Which body of the forward main pass a block takes (tdec_win_unit): the general one, or the whole-block one at place POS of its group of four.
template <bool WHOLE, int POS>
struct FwdBody {
  static constexpr bool value = WHOLE;
  static constexpr int  pos   = POS;
};

// ------------------------------------------------------------------------------------------------
// Windowed decoder kernel: one wave per 64/LPC code blocks, whole srsran_tdec_run_all in one launch.
//
// Per-code-block workspace (dwords, AW = nblk*8*LPC each):
//   S, P0, P1 : systematic / parity LLRs, blocked layout [step/8][lane][step%8]   (read only)
//   A1        : a-priori of decoder 1, ALREADY  app1 - ext1  (turbodecoder_iter.h:108), row layout [step][lane]
//   E1        : ext1 of decoder 1 (after the subtraction of :115 once n >= 2), row layout
//   A2        : input of decoder 2 (interleaved ext1), row layout
//   CK        : backward-recursion check-points, one per 8 steps
// The QPP interleaver is contention free for both directions: the 16 (8) sub-block outputs of one
// trellis step land in ONE row of the destination, permuted.  So the extrinsic exchange is, per step,
// one in-register permutation across the lanes of the code block (ds_bpermute) and one full 32-byte
// row store -- never a 2-byte scatter.
// The arrays' layouts and their loads / stores: turbo_layout.h; phase 0, the input extraction: turbo_extract.h.
// ------------------------------------------------------------------------------------------------

// One unit of work: the CPW = 64 / LPC code blocks wb * CPW ... of the batch, decoded by one wave in the workspace slab wb.
// Bl: re-derived backward metrics of the current 8-step block (8 steps x 8 states x int16x2 per lane) -- and, while the forward main pass
// does not run, the operands the forward warm-up hands to the backward pass, the staging image of the input extraction and the
// hard decision's byte / bit images; Tr: staging image of 8 exchanged rows (rows_to_lane).
// ES: early-stop / descriptor mode (transport-block decoding, sch_host.cpp).  A separate instantiation: the CRC state and
// the per-block descriptors must not cost the fixed-iteration kernel registers (it runs at 2 waves per SIMD).
// CKS: spacing of the backward check-points in trellis steps, 8 or 16 (win_ck_spacing, below, says which instantiation takes which).
template <int LPC, class AR, bool ES, int CKS>
__device__ __forceinline__ void tdec_win_unit(const WinParams& p, const uint32_t wb, const int lane, uint4 (&Bl)[8][2][64],
                                              uint32_t (&Tr)[512])
{
  const uint32_t crc_poly = ES ? p.crc_poly : 0u;
  const CbDesc*  desc     = ES ? p.desc : nullptr;
  constexpr int  NB  = 2 * LPC;
  constexpr int  CPW = 64 / LPC;
  constexpr bool NT  = !ES && !AR::kIs8; // non-temporal workspace loads (see ws_load16)
  static_assert(CKS == 8 || CKS == 16, "check-points every 8 or every 16 steps");
  static_assert(CKS == 8 || !AR::kIs8, "the 16-step form's whole-block bodies use Ar16's masked normalisation");
  // the arithmetic of the whole-block bodies: AR, and where they are discarded (they are generic lambdas' arms) a type that has normalize_if all the same
  using ARW = std::conditional_t<CKS == 16, AR, Ar16>;
  const int     pl   = lane % LPC;
  const uint32_t xbase = xch_group_base<LPC>(lane); // of the exchange across the lanes of a code block (permute_pair)
  const int     cb_raw = (int)wb * CPW + lane / LPC;
  // Lane groups past the end of the batch stay in the wave: the exchanged rows are loaded 16 bytes per lane and
  // re-distributed through LDS (issue_rows / rows_to_lane), which needs all 64 lanes.  They decode a copy of the last
  // code block into their own (allocated) workspace slots and write no output.
  const bool    live = cb_raw < p.n_cb;
  const int     cb   = live ? cb_raw : p.n_cb - 1;
  const uint32_t K       = p.K;
  const uint32_t long_sb = K / NB;
  const uint32_t nblk    = (long_sb + 7) >> 3;
  const uint32_t AW      = nblk * LPC * 8;

  // The workspace of the 64/LPC code blocks of this wave is ONE slab with the blocks interleaved at lane
  // granularity: every wave-level load/store touches one contiguous 256 B (dword) or 1 KB (dwordx4) run,
  // and the per-step row exchange of all the wave's code blocks is a single contiguous 256 B store.
  const uint32_t AWG = AW * CPW; // dwords per array per wave
  uint32_t* ws  = p.ws + (size_t)wb * p.ws_stride * CPW;
  uint32_t* S   = ws;
  uint32_t* P0  = ws + AWG;
  uint32_t* P1  = ws + 2 * AWG;
  uint32_t* A1  = ws + 3 * AWG;
  uint32_t* D   = ws + 4 * AWG; // decision LLRs of the last half iteration of a launch
  uint32_t* A2  = ws + 5 * AWG;
  uint32_t* CK  = ws + 6 * AWG;
  short*    TL  = reinterpret_cast<short*>(CK + (size_t)(nblk + 1) * 64 * 8) + 16 * (lane / LPC); // 12 tail LLRs per block

  // ---- phase 0: input extraction
  if (p.n_begin == 0) {
    // sub-blocks that are a multiple of 4 steps keep every run 8-byte aligned; a ragged last block (K = 5824: 364 = 45 * 8 + 4 steps) is
    // fetched whole -- the 4 steps behind it are the head of the next sub-block or the tail LLRs, inside the code block's
    // 3 K + 12 values, and the decoder never looks at steps >= long_sb
    const bool fast = !desc && !p.in_is8 && !p.sb_layout && (long_sb & 3u) == 0 && ((reinterpret_cast<uintptr_t>(p.input) | (2u * p.in_stride)) & 7u) == 0;
    if (fast) {
      const int first = (int)wb * CPW;
      extract_input_natural16<LPC, AR>(p.input + (size_t)first * p.in_stride, p.in_stride, p.n_cb - first, K, long_sb, nblk, lane,
                                       S, P0, P1, TL - 16 * (lane / LPC), reinterpret_cast<uint2*>(&Bl[0][0][0]));
    } else if (!p.in_is8 && p.sb_layout &&
               __all(((reinterpret_cast<uintptr_t>(p.input) + 2 * (desc ? (size_t)desc[cb].in_off : (size_t)cb * p.in_stride)) & 15u) == 0)) {
      // K = 5824 (the code block size of the largest 20 MHz transport blocks) has sub-blocks of 364 steps: 45 full blocks + 4 steps
      const short* in = p.input + (desc ? (size_t)desc[cb].in_off : (size_t)cb * p.in_stride);
      extract_input_sb16<LPC, AR>(in, K, long_sb >> 3, lane, pl, S, P0, P1, TL, Tr);
      if (long_sb & 7u) {
        extract_input<LPC, AR>(in, 1, K, long_sb, nblk, lane, pl, S, P0, P1, TL, long_sb >> 3, false);
      }
    } else if (p.in_is8) {
      const signed char* in = reinterpret_cast<const signed char*>(p.input) + (desc ? (size_t)desc[cb].in_off : (size_t)cb * p.in_stride);
      extract_input<LPC, AR>(in, p.sb_layout, K, long_sb, nblk, lane, pl, S, P0, P1, TL);
    } else {
      const short* in = p.input + (desc ? (size_t)desc[cb].in_off : (size_t)cb * p.in_stride);
      extract_input<LPC, AR>(in, p.sb_layout, K, long_sb, nblk, lane, pl, S, P0, P1, TL);
    }
  }
  // rows of the exchanged vectors whose subtraction wraps instead of saturating (8-bit only: the ragged
  // tail of srsran_vec_sub_bbb's 32-byte vector loop, vector_simd.c:162-190)
  const uint32_t wrap_row = (AR::kIs8 && (K & 31u)) ? long_sb - 1 : 0xffffffffu;
  __syncthreads();

  // ---- hard decision (turbodecoder.c:370-378 + turbodecoder_win.h:973-993): bit = LLR > 0, MSB first.
  // Source: app1 after an even number of half iterations, else ext1; the last half iteration filed it in D.
  // With a CRC generator the checksum of the K hard bits is formed on the way (sch.c:430-447: zero means the code
  // block is good): every lane runs the bit-serial CRC of its two sub-blocks, the 16 partial checksums are shifted
  // to their place by multiplication with x^(W (NB-1-d)) mod g and XOR-ed across the lanes of the code block.
  uint8_t*       out       = p.output + (desc ? (size_t)desc[cb].out_off : (size_t)cb * p.out_stride);
  const uint32_t out_bytes = desc ? desc[cb].out_bytes : K / 8;
  // Early stop: a code block that has matched its CRC (or a lane group behind the end of the batch) stays in the wave until
  // the wave's last block is done, but its vectors are dead.  Its block / row indices are masked to 0 so that it keeps
  // re-touching one cached line per array instead of streaming its workspace through HBM: m_own covers the accesses a lane
  // makes for its own sub-blocks, m_row the 16-byte row pieces it fetches for the lane group that owns those columns.
  uint32_t m_own_v = ~0u, m_row_v = ~0u;
  auto     set_masks = [&](bool dead) {
    const unsigned long long dm = __ballot(dead);
    // first lane of the group owning the columns this lane fetches in issue_rows: 4 (lane % 16) .. + 3, or 8 (lane % 8) .. + 7 with 8-bit storage
    const int                og = AR::kIs8 ? ((8 * (lane & 7)) / LPC) * LPC : ((4 * (lane & 15)) / LPC) * LPC;
    m_own_v                     = dead ? 0u : ~0u;
    m_row_v                     = ((dm >> og) & 1ull) ? 0u : ~0u;
  };
  if (ES) {
    set_masks(!live);
  }
  auto m_own = [&]() -> uint32_t { return ES ? m_own_v : ~0u; }; // (without early stop both fold to "no mask")
  auto m_row = [&]() -> uint32_t { return ES ? m_row_v : ~0u; };
  // A launch that completes the run (WinParams::final_run) files, in its last half iteration, one sign bit per value instead: row k
  // of the wave is 16 bytes at D + 4 k dwords, the 64-bit masks (one bit per lane) of the low and of the high sub-block.
  const bool bit_rows = !ES && p.final_run && !p.dec_llr && p.n_end > p.n_begin;
  auto decide = [&](bool write, bool final_try) -> uint32_t {
    short*         o16   = (p.dec_llr && live && write) ? p.dec_llr + (size_t)cb * K : nullptr;
    const bool     whole = (long_sb & 7) == 0;
    const uint32_t bps   = long_sb >> 3; // bytes per sub-block
    const uint32_t poly  = crc_poly & 0xffffffu;
    uint32_t       c0 = 0, c1 = 0;
    // ragged sub-blocks (long_sb not a multiple of 8): the hard bits of every sub-block are first packed MSB first into a
    // byte image in LDS (the beta buffer is idle between half iterations), sub-block d at sbuf[d][.] with a zero byte
    // behind it, and the natural-order bytes are cut out of that image afterwards
    const uint32_t sbs  = nblk + 1;
    uint8_t*       sbuf = reinterpret_cast<uint8_t*>(&Bl[0][0][0]) + (size_t)(lane / LPC) * NB * sbs;
    static_assert(sizeof(Bl) >= 64 / LPC * 2 * LPC * (6144 / (2 * LPC) / 8 + 2), "byte image does not fit");
    if (!whole) {
      sbuf[(2 * pl) * sbs + nblk]     = 0;
      sbuf[(2 * pl + 1) * sbs + nblk] = 0;
    }
    // the filed sign bits: the whole image of the wave (16 bytes x long_sb) comes into the beta buffer with coalesced 16-byte loads,
    // behind the byte image of ragged sub-blocks (turbo_device.h: win_final_fits); every lane then picks its own bit of both masks
    uint4* img = &Bl[0][0][0] + (whole ? 0u : (CPW * NB * sbs + 15u) / 16u);
    if (bit_rows) {
      for (uint32_t k = lane; k < long_sb; k += 64) {
        img[k] = ws_load16<NT>(D + (size_t)k * 4);
      }
      __syncthreads();
    }
    {
      const bool wide = whole && ((bps & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 3) == 0) && out_bytes == K / 8;
      uint32_t   w0 = 0, w1 = 0;
      uint32_t   t[8], tn[8];
      if (!bit_rows) {
        issue_rows_raw<AR::kIs8, NT>(D, 0, lane, t);
      }
      for (uint32_t b = 0; b < nblk; b++) {
        if (!bit_rows && b + 1 < nblk) {
          issue_rows_raw<AR::kIs8, NT>(D, (b + 1) & m_row(), lane, tn);
        }
        uint32_t r[8];
        if (bit_rows) {
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const uint32_t k = b * 8 + j < long_sb ? b * 8 + j : long_sb - 1;
            const uint4    m = img[k];
            // (a positive int16 in each half stands for the bit: the code below only looks at the signs)
            r[j] = (uint32_t)(((((uint64_t)m.y << 32) | m.x) >> lane) & 1u) | ((uint32_t)(((((uint64_t)m.w << 32) | m.z) >> lane) & 1u) << 16);
          }
        } else {
          rows_to_lane_v<AR::kIs8>(Tr, lane, t, r);
        }
        uint32_t b0 = 0, b1 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          if (b * 8 + j < long_sb) {
            const s2       v  = from_u(r[j]);
            const uint32_t x0 = v.x > 0 ? 1u : 0u, x1 = v.y > 0 ? 1u : 0u;
            b0 |= (x0 << 7) >> j;
            b1 |= (x1 << 7) >> j;
            if (crc_poly) { // crc.c:92-140, MSB first, zero initial state
              c0 = ((c0 << 1) & 0xffffffu) ^ ((((c0 >> 23) ^ x0) & 1u) ? poly : 0u);
              c1 = ((c1 << 1) & 0xffffffu) ^ ((((c1 >> 23) ^ x1) & 1u) ? poly : 0u);
            }
            if (o16 && whole) { // parity aid: decision LLRs in natural order
              o16[(2 * pl) * long_sb + b * 8 + j]     = AR::out16(v.x);
              o16[(2 * pl + 1) * long_sb + b * 8 + j] = AR::out16(v.y);
            }
          }
        }
        if (!whole) {
          sbuf[(2 * pl) * sbs + b]     = (uint8_t)b0;
          sbuf[(2 * pl + 1) * sbs + b] = (uint8_t)b1;
        }
        if (whole && write && live) {
          if (wide) {
            w0 |= b0 << (8 * (b & 3));
            w1 |= b1 << (8 * (b & 3));
            if ((b & 3) == 3) {
              *reinterpret_cast<uint32_t*>(out + (2 * pl) * bps + (b & ~3u))     = w0;
              *reinterpret_cast<uint32_t*>(out + (2 * pl + 1) * bps + (b & ~3u)) = w1;
              w0 = w1 = 0;
            }
          } else {
            if ((2 * pl) * bps + b < out_bytes) {
              out[(2 * pl) * bps + b] = (uint8_t)b0;
            }
            if ((2 * pl + 1) * bps + b < out_bytes) {
              out[(2 * pl + 1) * bps + b] = (uint8_t)b1;
            }
          }
        }
        if (!bit_rows) {
#pragma unroll
          for (int j = 0; j < 8; j++) {
            t[j] = tn[j];
          }
        }
      }
    }
    uint32_t crc = 0;
    if (crc_poly) {
      auto mulmod = [&](uint32_t a, uint32_t m) { // a(x) m(x) mod g(x), all below x^24
        uint32_t r = 0;
#pragma unroll 4
        for (int i = 23; i >= 0; i--) {
          r = ((r << 1) & 0xffffffu) ^ (((r >> 23) & 1u) ? poly : 0u);
          r ^= ((m >> i) & 1u) ? a : 0u;
        }
        return r;
      };
      crc = mulmod(c0, p.crc_mult[2 * pl]) ^ mulmod(c1, p.crc_mult[2 * pl + 1]);
#pragma unroll
      for (int off = LPC / 2; off > 0; off >>= 1) {
        crc ^= __shfl_xor(crc, off, LPC);
      }
    }
    // ragged sub-blocks: with early stop the bytes are cut out only when the block has just passed its CRC or on the last
    // half iteration allowed (earlier attempts would be overwritten anyway)
    __syncthreads();
    if (!whole && write && (!crc_poly || crc == 0 || final_try)) {
      const uint32_t nbytes = K / 8;
      const uint32_t lim    = out_bytes < nbytes ? out_bytes : nbytes;
      const bool     al     = (reinterpret_cast<uintptr_t>(out) & 3) == 0;
      for (uint32_t w = pl; w * 4 < nbytes; w += LPC) {
        uint32_t d = (w * 32) / long_sb, k = w * 32 - d * long_sb;
        uint32_t word = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (w * 4 + t < nbytes) {
            // 8 bits of sub-block d from step k (zeros past its end), completed from the head of sub-block d + 1
            const uint8_t* q = sbuf + d * sbs + (k >> 3);
            uint32_t       v = ((((uint32_t)q[0] << 8) | q[1]) >> (8 - (k & 7))) & 0xffu;
            if (k + 8 > long_sb && d + 1 < (uint32_t)NB) {
              v |= (uint32_t)sbuf[(d + 1) * sbs] >> (long_sb - k);
            }
            word |= v << (8 * t);
          }
          k += 8;
          if (k >= long_sb) {
            k -= long_sb;
            d++;
          }
        }
        if (live) {
          if (al && w * 4 + 3 < lim) {
            *reinterpret_cast<uint32_t*>(out + 4 * w) = word;
          } else {
#pragma unroll
            for (int t = 0; t < 4; t++) {
              if (w * 4 + t < lim) {
                out[w * 4 + t] = (uint8_t)(word >> (8 * t));
              }
            }
          }
        }
      }
      if (o16) { // parity aid: decision LLRs in natural order
        const short* sd = reinterpret_cast<const short*>(D);
        for (uint32_t nn = pl; nn < K; nn += LPC) {
          const uint32_t d = nn / long_sb, k = nn % long_sb;
          const uint32_t e = (k * 64 + (lane / LPC) * LPC + (d >> 1)) * 2 + (d & 1);
          o16[nn] = AR::kIs8 ? (short)reinterpret_cast<const signed char*>(D)[e] : sd[e]; // (8-bit storage holds the plain int8 values)
        }
      }
    }
    __syncthreads();
    return crc;
  };
  bool     done = false; // early stop: the CRC of this code block has matched
  uint32_t noi  = 0;     // half iterations run for this code block in this launch (sch.c:424: cb_noi)

  // ---- half iterations (turbodecoder_iter.h:72-141)
  for (uint32_t n = p.n_begin; n < p.n_end; n++) {
    const bool      dec1    = !(n & 1);
    const bool      has_app = dec1 && n > 0;
    const uint32_t* Y       = dec1 ? P0 : P1;
    const short*    xt      = dec1 ? TL : TL + 6;
    const short*    yt      = dec1 ? TL + 3 : TL + 9;

    // operands of 8 consecutive steps of this lane's two sub-blocks: x (systematic + a-priori), y (parity).
    // issue() only starts the loads (software pipelining: the next block is requested before the current
    // one is computed, so HBM latency hides behind a few hundred VALU instructions); prep() consumes them.
    struct Ops {
      uint32_t x[8], y[8], a[8];
    };
    // ok = false: there is no block b (the pipeline runs out at the end of a pass).
    // The 16-step form requests without a branch, always six loads.  A branch around a request merges an arm without loads into the path, and
    // the compiler's wait for anything requested before the branch becomes a wait for everything (it counts the most conservative arm); two
    // arms that load the same registers from different arrays cost a wait for the first arm's loads in the second.  So: the systematic block
    // of decoder 1 and the exchanged rows of decoder 2 are the same bytes of their arrays (a block of a blocked array and the 8 rows of a block
    // of a row array are one contiguous run of the wave's slab, 16 bytes per lane and half), only the array differs; and a request that is not
    // needed (no block b, no a-priori array in this half iteration) goes, from every lane, to the first 16 bytes of the array.
    // nt: the cache policy of the request (16-step form).  kStream, the kernel's NT, for every request that is the bytes' last use before they are
    // rewritten -- all but those of the backward main pass's lowest blocks, which the forward main pass reads again soon enough (kReuse: there).
    constexpr std::integral_constant<bool, NT>    kStream{};
    constexpr std::integral_constant<bool, false> kReuse{};
    const uint32_t* X = dec1 ? S : A2;
    auto issue = [&](auto nt, uint32_t b, Ops& q, bool ok = true) {
      if constexpr (CKS == 16) {
        static_assert(!ES, "the early-stop masks differ between blocked and row arrays");
        const bool oka = ok && has_app;
        uint32_t   bb = ok ? b : 0u, ba = oka ? b : 0u;
        int        ln = ok ? lane : 0, la = oka ? lane : 0;
        // (opaque: the addresses of the requests whose block index is the same in every half iteration -- the first ones of each pass -- are
        // otherwise all formed once in front of the half-iteration loop and held across it, in registers the forward main pass does not have)
        asm volatile("" : "+v"(ln), "+v"(la));
        issue_rows_raw<AR::kIs8, nt.value>(X, bb, ln, q.x);
        issue_rows_raw<AR::kIs8, nt.value>(Y, bb, ln, q.y);
        issue_rows_raw<AR::kIs8, nt.value>(A1, ba, la, q.a);
      } else {
        if (dec1) {
          load_block_raw<AR::kIs8, NT>(S, (b & m_own()) * 64 + lane, q.x);
        } else {
          issue_rows_raw<AR::kIs8, NT>(A2, b & m_row(), lane, q.x);
        }
        load_block_raw<AR::kIs8, NT>(Y, (b & m_own()) * 64 + lane, q.y);
        if (has_app) {
          issue_rows_raw<AR::kIs8, NT>(A1, b & m_row(), lane, q.a);
        }
      }
    };
    auto prep = [&](const Ops& q, s2(&xs)[8], s2(&ys)[8], s2(&ap)[8]) {
      uint32_t xr[8], ar[8], yr[8];
      if (dec1) {
        block_values<AR::kIs8>(q.x, xr);
      } else {
        rows_to_lane_v<AR::kIs8>(Tr, lane, q.x, xr);
      }
      if (has_app) {
        rows_to_lane_v<AR::kIs8>(Tr, lane, q.a, ar);
      }
      block_values<AR::kIs8>(q.y, yr);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        xs[j] = from_u(xr[j]);
        ys[j] = from_u(yr[j]);
        ap[j] = splat(0);
        if (has_app) {
          ap[j] = from_u(ar[j]);
          xs[j] = AR::add(ap[j], xs[j]);
        }
      }
    };
    // "the values of this set are taken": a compiler-level use of every register issue() loads.  Where the values are only renamed on their way
    // to their use (block_values of int16 storage), the wait for them would otherwise sink below loads requested later.
    auto taken = [&](const Ops& q) {
      asm volatile("" ::"v"(q.x[0]), "v"(q.x[1]), "v"(q.x[2]), "v"(q.x[3]), "v"(q.x[4]), "v"(q.x[5]), "v"(q.x[6]), "v"(q.x[7]));
      asm volatile("" ::"v"(q.y[0]), "v"(q.y[1]), "v"(q.y[2]), "v"(q.y[3]), "v"(q.y[4]), "v"(q.y[5]), "v"(q.y[6]), "v"(q.y[7]));
      if (has_app || CKS == 16) { // (the 16-step form always loads all three)
        asm volatile("" ::"v"(q.a[0]), "v"(q.a[1]), "v"(q.a[2]), "v"(q.a[3]), "v"(q.a[4]), "v"(q.a[5]), "v"(q.a[6]), "v"(q.a[7]));
      }
    };
    // The two main passes keep at least TWO blocks in flight behind the one they work on: HBM latency under load exceeds one block of
    // compute.  Four sets whose roles rotate (the loops are unrolled by hand over four blocks): a set-to-set copy would wait for the set
    // that was just requested.
    Ops cur, nxt, nx2, nx3;
    // The turn from the backward to the forward main pass (16-step form, sub-blocks of 8 blocks or more: the backward pass's bottom group is a
    // whole-block one).  The backward pass ends on block 0 and the forward pass starts there, so what it starts from never leaves the registers:
    // the raw operands of blocks 0, 1 and 2 stay in their sets and the check-point at boundary 2 in ck2.  The same in every lane.
    const bool turned = CKS == 16 && nblk >= 8;
    uint32_t   ck2[8];

    // ================= forward warm-up (turbodecoder_win.h:684-750): the last 40 steps of every sub-block, all states unknown.
    // It needs nothing the backward recursion produces and runs FIRST: the backward main pass starts with the very blocks it
    // ends with, so the operands (x: systematic + a-priori, already summed; y: parity) of its last four blocks -- whole blocks,
    // also where the window starts inside one or the last one is ragged -- stay in this lane's slots of the beta buffer, which is
    // idle until the forward main pass, and are not fetched from HBM a second time.  fw[]: the start metrics the main pass takes over.
    s2 fw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      fw[i] = splat(-AR::kInf);
    }
    {
      const uint32_t w0 = long_sb - TD_WIN_OVERLAP;
      const uint32_t bl = nblk - 1;
      issue(kStream, w0 >> 3, cur);
      for (uint32_t b = w0 >> 3; b <= bl; b++) {
        issue(kStream, b < bl ? b + 1 : TD_WIN_OVERLAP / 8 - 1, nxt); // after the warm-up the backward warm-up starts at the end of the head window
        s2 xs[8], ys[8], ap[8];
        prep(cur, xs, ys, ap);
        if (b + 4 > bl) {
          keep_ops(Bl, b + 3 - bl, lane, xs, ys);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
          uint32_t k = b * 8 + j;
          if (k >= w0 && k < long_sb) {
            alpha_step<AR, false>(fw, fw, xs[j], ys[j]);
            uint32_t kk = k - w0;
            if (AR::norm_at(kk)) {
              AR::normalize(fw);
            }
          }
        }
        cur = nxt;
      }
    }
    // hand every estimate to the next sub-block; the first one starts in state 0
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint32_t u   = to_u(fw[i]);
      uint32_t prv = __shfl_up(u, 1, LPC);
      uint32_t lo  = (pl == 0) ? (uint32_t)(uint16_t)(short)(i ? -AR::kInf : 0) : (prv >> 16);
      uint32_t hi  = u & 0xffffu;
      fw[i]        = from_u(lo | (hi << 16));
    }

    s2 o[8];
    // ================= backward recursion (turbodecoder_win.h:551-681)
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[i] = splat(-AR::kInf);
    }
    // pass 0: 40 steps on the head of every sub-block, all states unknown
    for (int b = TD_WIN_OVERLAP / 8 - 1; b >= 0; b--) {
      if (b > 0) {
        issue(kStream, b - 1, nxt); // (pass 1 starts with the four blocks the forward warm-up left in the beta buffer)
      }
      s2 xs[8], ys[8], ap[8];
      prep(cur, xs, ys, ap);
#pragma unroll
      for (int j = 7; j >= 0; j--) {
        beta_step<AR>(o, xs[j], ys[j]);
        uint32_t k = b * 8 + j;
        if (AR::norm_at(k)) {
          AR::normalize(o);
        }
      }
      cur = nxt;
    }
    // hand every estimate to the previous sub-block; the last one starts from the tail trellis
    {
      short tr[8];
      tail_trellis<AR>(xt, yt, tr);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        uint32_t u   = to_u(o[i]);
        uint32_t nbr = __shfl_down(u, 1, LPC);
        uint32_t lo  = u >> 16;
        uint32_t hi  = (pl == LPC - 1) ? (uint32_t)(uint16_t)tr[i] : (nbr & 0xffffu);
        o[i]         = from_u(lo | (hi << 16));
      }
      uint32_t ck[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        ck[i] = to_u(o[i]);
      }
      store_block_v<AR::kIs8>(CK, (nblk & m_own()) * 64 + lane, ck);
    }
    // pass 1: whole sub-block, keep a check-point at every block boundary (CKS = 16: at every even one, the odd slots of CK stay unused).
    // Blocks nblk-1 ... nblk-4 come from the beta buffer; the first one fetched from HBM is `top` = nblk-5 (a sub-block has more than 40
    // steps: nblk >= 6).
    if constexpr (CKS == 16) {
      // Every block requests, once it has taken its own operands, the block THREE below it, so two requests stay in flight behind the one a
      // block waits for.  Block b lives in set b mod 4 (cur, nxt, nx2, nx3): block 0 ends up in `cur`, where the forward main pass expects
      // it.  The loop goes over four blocks by hand and has ONE way in and one way out: it starts at the multiple of four above the last
      // block, and a block that does not exist only makes its request.  (Leaving the loop where the blocks end -- a `break` behind each
      // block -- the compiler routes every exit through the loop's latch, and the waits at the loop's top are counted as if a block's own
      // request could still be open there.)  The blocks from the beta buffer run in the same loop: their requests are blocks top ... top-2.
      const int top = (int)nblk - 5;
      auto      block = [&](int b, const Ops& c, Ops& tgt) {
        s2 xs[8], ys[8], ap[8];
        if (b > top) {
          kept_ops(Bl, (uint32_t)(b < (int)nblk ? b : (int)nblk - 1) + 4 - nblk, lane, xs, ys);
        } else {
          taken(c);
          prep(c, xs, ys, ap);
        }
        issue(kStream, b - 3, tgt, b >= 3 && b - 3 <= top);
        if (b < (int)nblk) {
#pragma unroll
          for (int j = 7; j >= 0; j--) {
            uint32_t k = b * 8 + j;
            if (k < long_sb) {
              beta_step<AR>(o, xs[j], ys[j]);
              if (j == 0 && b > 0 && !(b & 1)) {
                uint32_t ck[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                  ck[i] = to_u(o[i]);
                }
                store_block_v<AR::kIs8>(CK, ((uint32_t)b & m_own()) * 64 + lane, ck);
              }
              if (AR::norm_at(k)) {
                AR::normalize(o);
              }
            }
          }
        }
      };
      // The whole-block body: a block of a group of four whose top block b (b = 3 mod 4) has 7 <= b <= nblk - 5.  Every block of such a group
      // is a whole one fetched from HBM (b <= top) and so is the block it requests (b - 3 >= 1), so the schedule of the normalisation is the
      // step's position in the block; the check-point is stored by the even blocks, second and fourth of the group.
      auto whole_block = [&](auto nt, auto ck_store, int b, const Ops& c, Ops& tgt) {
        s2 xs[8], ys[8], ap[8];
        taken(c);
        prep(c, xs, ys, ap);
        issue(nt, b - 3, tgt);
#pragma unroll
        for (int j = 7; j >= 0; j--) {
          beta_step<AR>(o, xs[j], ys[j]);
          if constexpr (ck_store.value) {
            if (j == 0) {
              uint32_t ck[8];
#pragma unroll
              for (int i = 0; i < 8; i++) {
                ck[i] = to_u(o[i]);
              }
              store_block_v<AR::kIs8>(CK, ((uint32_t)b & m_own()) * 64 + lane, ck);
            }
          }
          if (AR::norm_in_block(j)) {
            AR::normalize(o);
          }
        }
      };
      // The bottom group (blocks 3 ... 0) where it is a whole-block one: straight-line code behind the loops, because it is where the pass turns.  Block b
      // lives in set b mod 4, so the raw operands of blocks 0, 1 and 2 are, or will be, in `cur`, `nxt` and `nx2` -- the sets the forward main pass calls
      // q0, q1 and q2 and starts from.  Block 3 makes the group's only request (block 0, the bytes' last use before they are rewritten); nothing is
      // requested for blocks that are not there, so `nxt` and `nx2` keep what arrived.  Block 2 leaves its check-point, the one the forward pass starts
      // from, in ck2 instead of slot 2 of CK.  Blocks 1 and 0 have no steps at all: all the backward pass ever made of them was the check-point at
      // boundary 0, which no pass reads (the forward pass derives the values inside its first pair from boundary 2), and their operands are
      // taken by the forward pass's first pair.
      auto turn_block = [&](auto first, const Ops& c) {
        s2 xs[8], ys[8], ap[8];
        taken(c);
        prep(c, xs, ys, ap);
        if constexpr (first.value) {
          issue(kStream, 0, cur);
        }
#pragma unroll
        for (int j = 7; j >= 0; j--) {
          beta_step<AR>(o, xs[j], ys[j]);
          if (!first.value && j == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
              ck2[i] = to_u(o[i]);
            }
          } else if (AR::norm_in_block(j)) {
            AR::normalize(o);
          }
        }
      };
      constexpr std::integral_constant<bool, true>  kStore{};
      constexpr std::integral_constant<bool, false> kNoStore{};
      // Two bodies, each emitted once, never two arms of one loop trip (at a merge the compiler counts the arm with the fewest loads in
      // flight): the general loop runs the groups that hold a block from the beta buffer or a ragged one (a sub-block has more than 40 steps, so
      // nblk >= 6 and there is at least one), the whole-block loop every group below them down to blocks 7 ... 4, the straight-line bottom group
      // blocks 3 ... 0 (nblk >= 8; a shorter sub-block's bottom group holds a block from the beta buffer and is the general loop's last trip).  The
      // way into either loop and into the bottom group carries what a back edge carries: the requests of the next three blocks.
      int b = ((int)nblk - 1) | 3;
#pragma nounroll
      for (; b > top; b -= 4) {
        block(b, nx3, cur);
        block(b - 1, nx2, nx3);
        block(b - 2, nxt, nx2);
        block(b - 3, cur, nxt);
      }
      // The whole-block loop is itself two copies of one body, one behind the other, that differ in the policy of their requests.  The forward main
      // pass reads block b again once the wave has gone down to block 0 and come back up: the lower the block, the fewer bytes the chip moves
      // between its two reads, and below p.reuse_blocks a good part of the lines is still in the L2 when it is wanted again -- if the first read left it there.
      // So the groups that request only blocks >= reuse_blocks keep the non-temporal policy, the groups below them (a group whose top block is b
      // requests blocks b - 3 ... b - 6) request with the default one.  The bound is the same in every lane and a run-time value (WinParams);
      // the way from the first copy into the second carries the three requests its back edge carries.  reuse_blocks = 0: no trip of the second copy.
      const int b_reuse = p.reuse_blocks ? (int)p.reuse_blocks + 6 : 7;
#pragma nounroll
      for (; b >= b_reuse; b -= 4) {
        whole_block(kStream, kNoStore, b, nx3, cur);
        whole_block(kStream, kStore, b - 1, nx2, nx3);
        whole_block(kStream, kNoStore, b - 2, nxt, nx2);
        whole_block(kStream, kStore, b - 3, cur, nxt);
      }
#pragma nounroll
      for (; b >= 7; b -= 4) {
        whole_block(kReuse, kNoStore, b, nx3, cur);
        whole_block(kReuse, kStore, b - 1, nx2, nx3);
        whole_block(kReuse, kNoStore, b - 2, nxt, nx2);
        whole_block(kReuse, kStore, b - 3, cur, nxt);
      }
      if (turned) { // (b = 3 here; where the general loop ran the bottom group, b = -1)
        turn_block(std::true_type{}, nx3);
        turn_block(std::false_type{}, nx2);
      }
    } else {
      // (8-step check-points: the 8-bit and the early-stop kernels.  With four rotating sets the int16 early-stop kernels spill -- their forward
      // main pass double-buffers check-point and table entries on top of the CRC state -- so they all keep three sets, copied set to set, two blocks ahead)
      for (int b = (int)nblk - 1; b >= 0; b--) {
        const bool ahead = b + 3 <= (int)nblk; // block b - 2 is one of those
        if (b > 1 && ahead) {
          issue(kStream, b - 2, nx2);
        }
        s2 xs[8], ys[8], ap[8];
        if (b + 4 >= (int)nblk) {
          kept_ops(Bl, (uint32_t)b + 4 - nblk, lane, xs, ys);
        } else {
          prep(cur, xs, ys, ap);
        }
#pragma unroll
        for (int j = 7; j >= 0; j--) {
          uint32_t k = b * 8 + j;
          if (k < long_sb) {
            beta_step<AR>(o, xs[j], ys[j]);
            if (j == 0 && b > 0 && (CKS == 8 || !(b & 1))) {
              uint32_t ck[8];
#pragma unroll
              for (int i = 0; i < 8; i++) {
                ck[i] = to_u(o[i]);
              }
              store_block_v<AR::kIs8>(CK, ((uint32_t)b & m_own()) * 64 + lane, ck);
            }
            if (AR::norm_at(k)) {
              AR::normalize(o);
            }
          }
        }
        if (b > 0 && ahead) { // (block 0 stays in `cur`: the forward main pass starts with it)
          cur = nxt;
          nxt = nx2;
        }
      }
    }
    __syncthreads(); // orders this lane's check-point stores before its loads below

    // ================= forward recursion + LLR (turbodecoder_win.h:751-832), from the warm-up's metrics
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[i] = fw[i];
    }

    const uint32_t* lut = dec1 ? p.deint : p.inter; // per (step, destination lane): row and source sub-blocks (turbo_layout.h: xch_pack)
    uint32_t*       dst = dec1 ? A2 : A1;
    // The subtractions of the NEXT half iteration (turbodecoder_iter.h:108,115) are applied on the way out:
    //   decoder 1: ext1 -= app1 (the a-priori it just used) before the interleaved copy goes to A2
    //   decoder 2: app1 = ext2 - ext1 ... and the ext1 value an output pairs with after de-interleaving is the very
    //              A2 value it had as systematic input at the same step and lane (app2[i] = ext1[inter[i]]), so the
    //              difference is formed before the permutation and no ext1 array is exchanged at all.
    // The raw SISO output is only needed by the hard decision: the LAST half iteration of a launch files it in D.
    const bool fuse = dec1 && n >= 2;
    // int16: that subtraction wraps, and ap[] is zero wherever no a-priori array is loaded, so every output has ONE subtrahend without a decision per
    // step: ap[j] | (xs[j] & sub_x) -- decoder 1 subtracts its a-priori value (zero in the first half iteration), decoder 2 its systematic input.
    // (The 8-bit decoders saturate except in the rows that wrap, and the two modes compare different rows: they keep their arms.)
    uint32_t sub_x = dec1 ? 0u : ~0u;
    asm volatile("" : "+s"(sub_x)); // (opaque: a mask known to be 0 or ~0 is turned back into the two arms)
    const bool last = (n + 1 == p.n_end) || crc_poly; // with early stop every half iteration may be the last
    // ... and the last half iteration of a complete run files sign bits only: the next a-priori array would never be read
    const bool sign_rows = bit_rows && n + 1 == p.n_end;

    // The forward main pass has two bodies.  The general one takes any block: ragged, one that is not there.  The whole-block one (16-step form only) takes
    // a whole block of a group of four whole blocks: its length is 8, so the schedule of the normalisation is the step's position in the block and a block's
    // steps are straight-line code; the three normalisations that an end of the sub-block takes out of that schedule are masked (below, at the loops).
    // (a whole block carries its place in its group of four: it says which of its normalisations can fall on an end of the sub-block and is masked)
    constexpr FwdBody<false, -1> kGeneral{};
    constexpr FwdBody<true, 0>   kWhole0{};
    constexpr FwdBody<true, 1>   kWhole1{};
    constexpr FwdBody<true, 2>   kWhole2{};
    constexpr FwdBody<true, 3>   kWhole3{};
    // one block of the main pass, in two parts (between them the 16-step form requests its next check-point).
    // rederive: beta[8b+1 .. 8b+len] (the stored, pre-normalisation values) from the value at the block's upper boundary into
    // this lane's private LDS slots (registers are needed for the prefetched operands)
    // in two steps: once the start value is taken, the 16-step form requests its next check-point into the same registers
    auto rederive_start = [&](int len, const uint32_t(&ckv)[8], s2(&st)[8]) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        st[i] = from_u(ckv[i]);
      }
      const int top = CKS == 16 ? (len - 1) & 7 : len - 1; // (len = 0: a block of the 16-step form that is not there)
      Bl[top][0][lane] = make_uint4(ckv[0], ckv[1], ckv[2], ckv[3]);
      Bl[top][1][lane] = make_uint4(ckv[4], ckv[5], ckv[6], ckv[7]);
    };
    auto rederive_rest = [&](auto whole, uint32_t b, int len, const s2(&xs)[8], const s2(&ys)[8], s2(&st)[8]) {
#pragma unroll
      for (int j = 6; j >= 0; j--) {
        if (whole.value || j <= len - 2) {
          uint32_t idx = b * 8 + j + 2; // index of the stored value we start from
          if constexpr (whole.pos == 3) {
            if (j == 6) { // the group's last block may be the sub-block's: the value at its end is not normalised
              ARW::normalize_if(st, norm_mask(idx != long_sb));
            } else if (AR::norm_in_block(j + 2)) {
              AR::normalize(st);
            }
          } else if (whole.value ? AR::norm_in_block(j + 2) : (idx != long_sb && AR::norm_at(idx))) {
            AR::normalize(st);
          }
          beta_step<AR>(st, xs[j + 1], ys[j + 1]);
          Bl[j][0][lane] = make_uint4(to_u(st[0]), to_u(st[1]), to_u(st[2]), to_u(st[3]));
          Bl[j][1][lane] = make_uint4(to_u(st[4]), to_u(st[5]), to_u(st[6]), to_u(st[7]));
        }
      }
    };
    // emit: the forward steps, their outputs, the exchange
    auto emit = [&](auto whole, uint32_t b, int len, const s2(&xs)[8], const s2(&ys)[8], const s2(&ap)[8], const uint32_t(&tr)[8], auto&& ck_taken) {
      uint32_t outv[8], rawv[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        outv[j] = 0;
        rawv[j] = 0;
        if (whole.value || j < len) {
          const uint4 b0 = Bl[j][0][lane], b1 = Bl[j][1][lane];
          const s2    B[8] = {from_u(b0.x), from_u(b0.y), from_u(b0.z), from_u(b0.w),
                              from_u(b1.x), from_u(b1.y), from_u(b1.z), from_u(b1.w)};
          s2       llr = alpha_step<AR, true>(o, B, xs[j], ys[j]);
          uint32_t k   = b * 8 + j;
          if constexpr (whole.pos == 0) {
            if (j == 0) { // the group's first block may be block 0: step 0 is not followed by a normalisation
              ARW::normalize_if(o, norm_mask(k != 0));
            } else if (AR::norm_in_block(j)) {
              AR::normalize(o);
            }
          } else if (whole.value ? AR::norm_in_block(j) : AR::norm_at(k)) {
            AR::normalize(o);
          }
          s2 proc = llr;
          if constexpr (!AR::kIs8) {
            proc = AR::ex_sub(llr, from_u(to_u(ap[j]) | (to_u(xs[j]) & sub_x)), false);
          } else if (fuse) {
            proc = AR::ex_sub(llr, ap[j], k == wrap_row);
          } else if (!dec1) {
            proc = AR::ex_sub(llr, xs[j], xch_row(tr[j]) == wrap_row); // wrap flag: row of the DESTINATION element
          }
          outv[j] = to_u(proc);
          rawv[j] = to_u(llr);
        }
      }
      if constexpr (CKS == 16) {
        // every entry counts as used here, also those behind a ragged block's end: a register that a load may still be writing makes
        // the compiler wait, before its next write, for whatever has been requested since -- the next block's operands
        asm volatile("" ::"v"(tr[0]), "v"(tr[1]), "v"(tr[2]), "v"(tr[3]), "v"(tr[4]), "v"(tr[5]), "v"(tr[6]), "v"(tr[7]));
        // ... and so does the check-point an odd block has requested for the next pair, just before its operand request: here the count that
        // retires it is exact.  At the next block's top it is not: the row stores below sit in conditional arms, the compiler counts the
        // arm with the fewest, and what it leaves in flight there are the last stores, not the operand loads.
        ck_taken();
      }
      // the hot store phase: per step the exchange and one row store, nothing else
      if (!sign_rows) {
        if constexpr (whole.value) {
          // all of the block's exchanges are requested before the first one is waited for: one LDS round trip per block, not one per step
          uint32_t xv[8];
#pragma unroll
          for (int j = 0; j < 8; j++) {
            xv[j] = permute_pair(outv[j], tr[j], xbase);
          }
#pragma unroll
          for (int j = 0; j < 8; j++) {
            store_xch_row<AR::kIs8>(dst, tr[j], m_own(), lane, xv[j]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) {
            if (j < len) {
              store_xch_row<AR::kIs8>(dst, tr[j], m_own(), lane, permute_pair(outv[j], tr[j], xbase));
            }
          }
        }
      }
      // ... and what only the last half iteration of a launch files, behind ONE decision per block
      if (last) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
          if (whole.value || j < len) {
            if (sign_rows) {
              // the values tdec_decision_byte reads (below), reduced to "> 0": one 16-byte row per step, stored by one lane
              const s2       v  = from_u(dec1 ? rawv[j] : permute_pair(rawv[j], tr[j], xbase));
              const uint64_t mx = __ballot(v.x > 0), my = __ballot(v.y > 0);
              if (lane == 0) {
                *reinterpret_cast<uint4*>(D + (size_t)(dec1 ? b * 8 + j : xch_row(tr[j]) & m_own()) * 4) =
                    make_uint4((uint32_t)mx, (uint32_t)(mx >> 32), (uint32_t)my, (uint32_t)(my >> 32));
              }
            } else if (dec1) {
              // what tdec_decision_byte reads (turbodecoder.c:370-378), in natural order: ext1 after decoder 1,
              // the de-interleaved ext2 (= app1 before the subtraction) after decoder 2
              store_row<AR::kIs8>(D, (b * 8 + j) & m_own(), lane, rawv[j]);
            } else {
              store_xch_row<AR::kIs8>(D, tr[j], m_own(), lane, permute_pair(rawv[j], tr[j], xbase));
            }
          }
        }
      }
    };

    if constexpr (CKS == 8) {
      uint32_t ck[8], tr[8], ckn[8], trn[8];
      load_block_raw<AR::kIs8, NT>(CK, (1u & m_own()) * 64 + lane, ck);
      load_lut(lut, pl, tr);
      if (nblk > 1) {
        issue(kStream, 1, nxt);
      }
      for (uint32_t b = 0; b < nblk; b++) {
        const int len = (long_sb - b * 8) < 8 ? (int)(long_sb - b * 8) : 8;
        s2        xs[8], ys[8], ap[8];
        if (b + 2 < nblk) {
          issue(kStream, b + 2, nx2);
        }
        if (b + 1 < nblk) {
          load_block_raw<AR::kIs8, NT>(CK, ((b + 2) & m_own()) * 64 + lane, ckn);
          load_lut(lut, (b + 1) * LPC + pl, trn);
        }
        prep(cur, xs, ys, ap);
        uint32_t ckv[8];
        block_values<AR::kIs8>(ck, ckv);
        s2 st[8];
        rederive_start(len, ckv, st);
        rederive_rest(kGeneral, b, len, xs, ys, st);
        emit(kGeneral, b, len, xs, ys, ap, tr, [] {});
        cur = nxt;
        nxt = nx2;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          ck[i] = ckn[i];
          tr[i] = trn[i];
        }
      }
    } else {
      // Check-points at the even block boundaries only.  Blocks go in pairs (b even, b + 1): both start from the check-point at
      // boundary b + 2 (the last pair: at the sub-block's end, slot nblk).  The odd block re-derives its betas from it as above; the even
      // block first walks it back through block b + 1 -- whose operands are here one block early: FOUR operand sets, block b + 3 is
      // requested while block b runs, so two blocks stay in flight behind the held one -- replaying the normalisation schedule of the
      // backward pass: what comes out is the pre-normalisation value at boundary b + 1, the check-point that was not stored.
      // The check-point is loaded in place (once per pair, right after its last use, a whole block of forward steps before the next
      // one) and so are the exchange-table entries (requested at the top of the block, used at its end): no second copy of either.
      // The four sets keep their registers (the loop is unrolled by hand over four blocks instead of copying set to set: a copy of
      // a set that was just requested waits for it), and a block requests nothing before it has taken what it needs from earlier
      // requests, so no wait reaches into the loads of its own block -- the exchange entries apart, behind which the odd block's
      // check-point load is unconditional for that reason (the last block of an even count re-loads slot nblk for nothing).
      Ops&     q0 = cur;
      Ops&     q1 = nxt;
      Ops&     q2 = nx2;
      Ops&     q3 = nx3;
      uint32_t(&ck)[8] = ck2;
      uint32_t tr[8];
      // Behind the backward pass's straight-line bottom group (`turned`) everything the first pair needs is here: blocks 0 ... 2 in q0 ... q2, the
      // check-point of boundary 2 in ck.  Nothing is requested, and the first thing that touches memory is block 0's own table load.  Elsewhere
      // only block 0 is here.  (An arm with requests next to a way without: the waits inside the loop are counted for the arm and are what they
      // were; the way without has nothing in flight.  The two ways leave the sets in different registers, and the copies that settle it behind the
      // merge wait for block 2 on the arm's way as well: once per half iteration of a sub-block of 7 blocks or fewer)
      if (!turned) {
        load_block_raw<AR::kIs8, NT>(CK, ((nblk < 2 ? nblk : 2u) & m_own()) * 64 + lane, ck);
        issue(kStream, 1, q1, nblk > 1);
        // The loop is entered with no more than its back edge brings: one request in flight, everything before it taken.  The waits at the top of
        // the loop are counted for the worst of the ways in; with all of these requests still open on this one, the count that suits it
        // would, on the back edge, reach into the last block's request.  (Once per half iteration: block 1's operands are waited for here.)
        asm volatile("" ::"v"(ck[0]), "v"(ck[1]), "v"(ck[2]), "v"(ck[3]), "v"(ck[4]), "v"(ck[5]), "v"(ck[6]), "v"(ck[7]));
        taken(q1);
        issue(kStream, 2, q2, nblk > 2);
      } else {
        // (block 0 was requested two blocks of steps ago, by block 3: waited for here, not at the loop's top, where the count would hold on the back edge too)
        taken(q1);
        taken(q2);
        taken(q0);
      }
      // b may lie behind the last block (the loop below goes over four blocks whatever the count): such a block has no steps, len = 0.  It makes
      // its requests and goes the same way as every other: an arm of its own, or one around the others' work, is a way on which the compiler
      // sees the table entries and the check-point still open, and its wait for them, placed behind the row stores, reaches into the request.
      // (whole: the block is one of a whole-block group.  What stays clamped there: the block that is requested and the check-point of the next pair may
      // lie behind the last block, b + 6 against b + 5 <= nblk.)
      auto block = [&](auto whole, auto even, uint32_t b, const Ops& c, const Ops& held, Ops& tgt) {
        const int rem = (int)long_sb - (int)b * 8;
        const int len = whole.value ? 8 : rem < 0 ? 0 : rem < 8 ? rem : 8;
        s2         xs[8], ys[8], ap[8], st[8];
        uint32_t   ckv[8];
        auto       ck_taken = [&] { asm volatile("" ::"v"(ck[0]), "v"(ck[1]), "v"(ck[2]), "v"(ck[3]), "v"(ck[4]), "v"(ck[5]), "v"(ck[6]), "v"(ck[7])); };
        ck_taken();
        block_values<AR::kIs8>(ck, ckv);
        load_lut(lut, (whole.value || b < nblk ? b : nblk - 1) * LPC + pl, tr);
        taken(c);
        if constexpr (even.value) {
          taken(held); // (also where there is no block b + 1: the set was requested all the same)
          issue(kStream, b + 3, tgt, b + 3 < nblk);
        } else {
          // the check-point's last use is the copy at the start of the re-derivation: the next pair's is requested there, ahead of the operands
          prep(c, xs, ys, ap);
          rederive_start(len, ckv, st);
          const uint32_t bn = b + 3 < nblk ? b + 3 : nblk;
          load_block_raw<AR::kIs8, NT>(CK, (bn & m_own()) * 64 + lane, ck);
          issue(kStream, b + 3, tgt, b + 3 < nblk);
        }
        {
          if constexpr (even.value) {
            const bool paired = whole.value || b + 1 < nblk;
            s2        x1[8], y1[8], a1[8];
            if (paired) {
              prep(held, x1, y1, a1);
            }
            prep(c, xs, ys, ap);
            if (paired) {
              const int len1 = whole.value ? 8 : (long_sb - (b + 1) * 8) < 8 ? (int)(long_sb - (b + 1) * 8) : 8;
#pragma unroll
              for (int i = 0; i < 8; i++) {
                st[i] = from_u(ckv[i]);
              }
#pragma unroll
              for (int j = 7; j >= 0; j--) {
                if (whole.value || j < len1) {
                  uint32_t idx = (b + 1) * 8 + j + 1; // index of the value we start from
                  if constexpr (whole.pos == 2) {
                    if (j == 7) { // the group's second pair may start from the check-point at the sub-block's end, which is not normalised
                      AR::normalize_if(st, norm_mask(idx != long_sb));
                    } else if (AR::norm_in_block(j + 1)) {
                      AR::normalize(st);
                    }
                  } else if (whole.value ? AR::norm_in_block(j + 1) : (idx != long_sb && AR::norm_at(idx))) {
                    AR::normalize(st);
                  }
                  beta_step<AR>(st, x1[j], y1[j]);
                }
              }
#pragma unroll
              for (int i = 0; i < 8; i++) {
                ckv[i] = to_u(st[i]);
              }
            }
            rederive_start(len, ckv, st);
          }
          rederive_rest(whole, b, len, xs, ys, st);
          emit(whole, b, len, xs, ys, ap, tr, ck_taken);
        }
      };
      constexpr std::integral_constant<bool, true>  kEven{};
      constexpr std::integral_constant<bool, false> kOdd{};
      // (one way out, at the bottom: a `break` behind each block is routed through the loop's latch, and the waits at the loop's top are
      // then counted as if a block's own request could still be open there; a block skipped as a whole is an arm without requests)
      // A group of four starting at b takes the whole-block body when its blocks b ... b + 3 are whole ones: b + 5 <= nblk where the last block may be
      // ragged or the group behind it is not complete, b + 4 <= nblk where the sub-block is a multiple of 32 steps (wl).  Three normalisations of a group can
      // then fall on an end of the sub-block, where the schedule leaves them out, and are masked instead of branched around (AR::normalize_if): the one behind
      // step 0 in the first block, and in the second pair -- whose check-point is then the sub-block's end, slot nblk -- the first one of the even block's
      // walk and of the odd block's re-derivation.  What runs off the end (block b + 3 ... b + 6, the next pair's check-point) is clamped in both bodies.
      // As in the backward pass the two bodies are two loops, each emitted once.  The general loop runs blocks 0 ... 3 in the first trip of the outer loop
      // only where the whole-block loop cannot take them (never with nblk >= 6) and the groups behind the whole-block range in the second; the whole-block
      // loop has groups only in the first.  Every way into either loop carries one request in flight, as its back edge does.  (One loop behind the other,
      // without the outer one, is the same schedule with 3 more registers and 45 more vector instructions per whole-block group: the compiler then forms the
      // row addresses of the last half iteration's stores differently.)
      uint32_t       b  = 0;
      const uint32_t wl = (long_sb & 31u) ? 5u : 4u;
#pragma nounroll
      for (int trip = 0; trip < 2; trip++) {
        const uint32_t gend = trip == 0 ? (wl <= nblk ? 0u : 4u) : nblk;
#pragma nounroll
        for (; b < gend; b += 4) {
          block(kGeneral, kEven, b, q0, q1, q3);
          block(kGeneral, kOdd, b + 1, q1, q2, q0);
          block(kGeneral, kEven, b + 2, q2, q3, q1);
          block(kGeneral, kOdd, b + 3, q3, q0, q2);
        }
#pragma nounroll
        for (; b + wl <= nblk; b += 4) {
          block(kWhole0, kEven, b, q0, q1, q3);
          block(kWhole1, kOdd, b + 1, q1, q2, q0);
          block(kWhole2, kEven, b + 2, q2, q3, q1);
          block(kWhole3, kOdd, b + 3, q3, q0, q2);
        }
      }
    }
    __syncthreads();
    if (crc_poly) {
      // decode_tb_cb (sch.c:420-454): hard bits + CRC after every half iteration; a code block stops at its first
      // match (its bits are written then and never again), the wave stops when all its code blocks have
      const bool     last_try = n + 1 == p.n_end;
      const bool     wr       = !done; // bits of the last half iteration THIS code block took part in
      const uint32_t crc      = decide(wr, last_try);
      if (!done) {
        noi++;
        done = crc == 0;
      }
      set_masks(done || !live);
      __syncthreads();
      if (__all(done || !live) || last_try) {
        break;
      }
    }
  }

  if (!crc_poly) {
    decide(true, true);
  } else if (p.noi && live && pl == 0) {
    p.noi[cb_raw]    = (int)noi;
    p.crc_ok[cb_raw] = done ? 1 : 0;
  }
}

// The product kernel: one workgroup (= one wave) per unit, two waves per SIMD.
// Check-point spacing: 16 steps where the kernel is bound by its HBM traffic (int16, fixed iterations: a quarter of it was check-points),
// 8 where the extra re-derivation can only cost (the 8-bit decoders are bound by VALU issue) or the working set partly hits in L2 (early stop).
template <class AR, bool ES>
constexpr int win_ck_spacing = (!AR::kIs8 && !ES) ? 16 : 8;

template <int LPC, class AR, bool ES, int CKS = win_ck_spacing<AR, ES>>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void tdec_win_kernel(const WinParams p)
{
  __shared__ uint4    Bl[8][2][64];
  __shared__ uint32_t Tr[512];
  tdec_win_unit<LPC, AR, ES, CKS>(p, blockIdx.x, threadIdx.x, Bl, Tr);
}

// ------------------------------------------------------------------------------------------------ launchers

template <bool ES>
static hipError_t launch_win_es(int nb, bool arith8, const WinParams& p, hipStream_t stream)
{
  const int lpc = nb / 2;
  dim3      grid(ceil_div(p.n_cb, 64 / lpc));
  if (!arith8 && nb == 16) {
    hipLaunchKernelGGL((tdec_win_kernel<8, Ar16, ES>), grid, dim3(64), 0, stream, p);
  } else if (!arith8 && nb == 8) {
    hipLaunchKernelGGL((tdec_win_kernel<4, Ar16, ES>), grid, dim3(64), 0, stream, p);
  } else if (arith8 && nb == 16) {
    hipLaunchKernelGGL((tdec_win_kernel<8, Ar8, ES>), grid, dim3(64), 0, stream, p);
  } else if (arith8 && nb == 32) {
    hipLaunchKernelGGL((tdec_win_kernel<16, Ar8, ES>), grid, dim3(64), 0, stream, p);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_win(int nb, bool arith8, const WinParams& p, hipStream_t stream)
{
  return (p.crc_poly || p.desc) ? launch_win_es<true>(nb, arith8, p, stream) : launch_win_es<false>(nb, arith8, p, stream);
}

uint32_t win_elem_index(int nb, uint32_t k, uint32_t d)
{
  return nb == 32 ? elem_index<16>(k, d) : (nb == 16 ? elem_index<8>(k, d) : elem_index<4>(k, d));
}

} // namespace turbo
} // namespace phyhip
