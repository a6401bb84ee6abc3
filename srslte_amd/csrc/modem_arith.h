// modem_arith.h -- the device functions the demodulating kernels share (modem_kernels.hip, nr_chan_kernels.hip, txdiv_kernels.hip): the integer soft-bit
// arithmetic of demod_soft.c as the x86 reference evaluates it, the transmit-diversity combiner, the Gold-sequence chips of one wave, sign flips and the
// soft-bit stores.  Device code only.
#pragma once
#include "hip_common.h"
#include "modem_device.h"

namespace phyhip {
namespace modem {

namespace {

__device__ __forceinline__ int cvt_rn(float v) // _mm_cvtps_epi32
{
  return (v >= -2147483648.0f && v < 2147483648.0f) ? __float2int_rn(v) : (int)0x80000000;
}
__device__ __forceinline__ int cvt_tr(float v) // _mm_cvttps_epi32 / cvttss2si
{
  return (v >= -2147483648.0f && v < 2147483648.0f) ? __float2int_rz(v) : (int)0x80000000;
}
__device__ __forceinline__ int cvt_tr_d(double v)
{
  return (v >= -2147483648.0 && v < 2147483648.0) ? __double2int_rz(v) : (int)0x80000000;
}
__device__ __forceinline__ int sat16(int v)
{
  return min(max(v, -32768), 32767);
}
__device__ __forceinline__ int sat8(int v)
{
  return min(max(v, -128), 127);
}

template <typename T>
struct Lim; // integer soft-bit types: wrap to the type, saturate like the packs instructions, scale constants
template <>
struct Lim<int16_t> {
  static __device__ __forceinline__ int wrap(int v) { return (int)(int16_t)v; }
  static __device__ __forceinline__ int sat(int v) { return sat16(v); }
  static constexpr int                  S_BPSK = 100, S16 = 400, S64 = 700, S256 = 1000;
  static constexpr int                  GROUP = 4; // symbols per SIMD iteration of the 16/64-QAM bodies
};
template <>
struct Lim<int8_t> {
  static __device__ __forceinline__ int wrap(int v) { return (int)(int8_t)v; }
  static __device__ __forceinline__ int sat(int v) { return sat8(sat16(v)); }
  static constexpr int                  S_BPSK = 20, S16 = 30, S64 = 40, S256 = 50;
  static constexpr int                  GROUP = 8;
};

// ---- one symbol -> QM soft bits (integer types) ------------------------------------------------------------------------
template <typename T, int MOD>
__device__ __forceinline__ void demod_int(float re, float im, uint32_t idx, uint32_t n, const Consts& k, int* v)
{
  using L            = Lim<T>;
  constexpr bool B   = sizeof(T) == 1;
  const float    x[2] = {re, im};
  if (MOD == 0) {
    v[0] = L::wrap(cvt_tr_d((double)((float)(-L::S_BPSK) * (re + im)) * 0.70710678118654752440));
  } else if (MOD == 1) {
    // vector_simd.c:436-472 / 524-589: 16 values per iteration saturate, the scalar remainder wraps
    const uint32_t len = 2 * n, body = len - len % 16;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int t = cvt_tr(x[c] * (B ? k.qpsk_b : k.qpsk_s));
      v[c]        = (2 * idx + c < body) ? L::sat(t) : L::wrap(t);
    }
  } else if (MOD == 2) {
    const bool body = idx < n - n % L::GROUP;
    const int  off  = B ? k.o16_b : k.o16_s;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      if (body) {
        const int t = L::sat(cvt_rn(x[c] * (float)(-L::S16)));
        v[c]        = t;
        v[2 + c]    = L::wrap(L::wrap(abs(t)) - off);
      } else {
        const int y = L::wrap(cvt_tr((float)L::S16 * x[c]));
        v[c]        = L::wrap(-y);
        v[2 + c]    = L::wrap(cvt_tr((float)abs(y) - (B ? k.t16_tail_b : k.t16_tail_s)));
      }
    }
  } else if (MOD == 3) {
    const bool body = idx < n - n % L::GROUP;
    const int  o1 = B ? k.o64a_b : k.o64a_s, o2 = B ? k.o64b_b : k.o64b_s;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      int t, s;
      if (body) {
        t = L::sat(cvt_rn(x[c] * (float)(-L::S64)));
        s = t;
      } else {
        t = L::wrap(cvt_tr((float)L::S64 * x[c]));
        s = L::wrap(-t);
      }
      const int a1 = L::wrap(L::wrap(abs(t)) - o1);
      v[c]         = s;
      v[2 + c]     = a1;
      v[4 + c]     = L::wrap(L::wrap(abs(a1)) - o2);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 2; c++) {
      float f  = -x[c];
      v[c]     = L::wrap(cvt_tr((float)L::S256 * f));
      f        = __fsub_rn(fabsf(f), k.c8);
      v[2 + c] = L::wrap(cvt_tr((float)L::S256 * f));
      f        = __fsub_rn(fabsf(f), k.c4);
      v[4 + c] = L::wrap(cvt_tr((float)L::S256 * f));
      f        = __fsub_rn(fabsf(f), k.c2);
      v[6 + c] = L::wrap(cvt_tr((float)L::S256 * f));
    }
  }
}

// ---- transmit-diversity (SFBC) combining: srsran_predecoding_diversity_csi (mimo/precoding.c:673-778), the one arithmetic of the per-stage kernel and
// the fused front end (txdiv_kernels.hip).  One RE pair (r0, r1 on neighbouring sub-carriers k, k + 1) carries two layer symbols:
//   x0 += conj(ha) r0 + hb conj(r1)      x1 += conj(hd) r1 - hc conj(r0)      g0 += |ha|^2 + |hb|^2      g1 += |hd|^2 + |hc|^2      per receive antenna
// with, for the port pair (a, b), ha = h[a][k], hb = h[b][k + 1], hc = h[b][k], hd = h[a][k + 1].  2 ports: (a, b) = (0, 1), ONE gain g0 for both
// symbols, replaced by 1e-4 inside the antenna loop when it is 0 (:699-701); 4 ports: (0, 2) on the first pair of a quad and (1, 3) on the second,
// each symbol with its own gain.  Operation order (ours): every product and sum rounded by itself (nothing contracts); per antenna the two complex
// products of a symbol are formed, added to each other, then to the accumulator; a gain's four squares are summed left to right, then added.
struct Sfbc {
  float x0r = 0.f, x0i = 0.f, x1r = 0.f, x1i = 0.f, g0 = 0.f, g1 = 0.f;
};
template <int PORTS>
__device__ __forceinline__ void sfbc_add(Sfbc& a, float2 ha, float2 hb, float2 hc, float2 hd, float2 r0, float2 r1)
{
  const float p0r = __fadd_rn(__fmul_rn(ha.x, r0.x), __fmul_rn(ha.y, r0.y)); // conj(ha) r0
  const float p0i = __fsub_rn(__fmul_rn(ha.x, r0.y), __fmul_rn(ha.y, r0.x));
  const float p1r = __fadd_rn(__fmul_rn(hb.x, r1.x), __fmul_rn(hb.y, r1.y)); // hb conj(r1)
  const float p1i = __fsub_rn(__fmul_rn(hb.y, r1.x), __fmul_rn(hb.x, r1.y));
  const float q0r = __fadd_rn(__fmul_rn(hd.x, r1.x), __fmul_rn(hd.y, r1.y)); // conj(hd) r1
  const float q0i = __fsub_rn(__fmul_rn(hd.x, r1.y), __fmul_rn(hd.y, r1.x));
  const float q1r = __fadd_rn(__fmul_rn(hc.x, r0.x), __fmul_rn(hc.y, r0.y)); // hc conj(r0)
  const float q1i = __fsub_rn(__fmul_rn(hc.y, r0.x), __fmul_rn(hc.x, r0.y));
  a.x0r           = __fadd_rn(a.x0r, __fadd_rn(p0r, p1r));
  a.x0i           = __fadd_rn(a.x0i, __fadd_rn(p0i, p1i));
  a.x1r           = __fadd_rn(a.x1r, __fsub_rn(q0r, q1r));
  a.x1i           = __fadd_rn(a.x1i, __fsub_rn(q0i, q1i));
  a.g0 = __fadd_rn(a.g0, __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(ha.x, ha.x), __fmul_rn(ha.y, ha.y)), __fmul_rn(hb.x, hb.x)), __fmul_rn(hb.y, hb.y)));
  if (PORTS == 2) {
    a.g0 = a.g0 == 0.f ? 1e-4f : a.g0;
  } else {
    a.g1 = __fadd_rn(a.g1, __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(hd.x, hd.x), __fmul_rn(hd.y, hd.y)), __fmul_rn(hc.x, hc.x)), __fmul_rn(hc.y, hc.y)));
  }
}
// x / den * M_SQRT2 as the C expression evaluates it: float quotient, product in double, rounded once to float
__device__ __forceinline__ float sfbc_quot(float v, float den)
{
  return __double2float_rn(__dmul_rn((double)__fdiv_rn(v, den), 1.41421356237309504880));
}
// the pair's two symbols and the two csi values the reference files for its REs.  2 ports: division by g0 scaling, csi = g0; 4 ports: the gains are
// scaled first, csi = scaled gain / nof_rx
template <int PORTS>
__device__ __forceinline__ void sfbc_finish(const Sfbc& a, float scaling, float nof_rx, float2& x0, float2& x1, float2& csi)
{
  const float d0 = __fmul_rn(a.g0, scaling), d1 = PORTS == 2 ? d0 : __fmul_rn(a.g1, scaling);
  x0  = make_float2(sfbc_quot(a.x0r, d0), sfbc_quot(a.x0i, d0));
  x1  = make_float2(sfbc_quot(a.x1r, d1), sfbc_quot(a.x1i, d1));
  csi = PORTS == 2 ? make_float2(a.g0, a.g0) : make_float2(__fdiv_rn(d0, nof_rx), __fdiv_rn(d1, nof_rx));
}

// ---- scrambling chips of one tile -> LDS --------------------------------------------------------------------------------
// register = x(n)..x(n+30) in bits 0..30; 16 chips per step (the feedback taps reach back at most 3 chips)
__device__ __forceinline__ uint32_t step16_x2(uint32_t s)
{
  return (s >> 16) | ((((s >> 3) ^ (s >> 2) ^ (s >> 1) ^ s) & 0xffffu) << 15);
}

__device__ __forceinline__ void wave_sync_lds()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// chips bit0 .. bit0 + nbits - 1 (bit0 a multiple of 128, nbits <= MODEM_TILE_BITS / 4) of the sequence -> the wave's LDS strip, packed.
// One lane per 128 chips: x2 register at the chunk start = XOR of the table columns the seed selects, 8 steps of 16
// chips; the seed-independent x1 chips come packed from a table.  Waves work independently (no workgroup barrier): while
// one runs its shift registers the others stream.
__device__ __forceinline__ void make_chips(const uint32_t* x1_bits, const uint32_t* x2_cols, uint32_t seed, uint32_t bit0, uint32_t nbits, uint32_t* cbw)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nch  = (nbits + MODEM_SEQ_CHUNK - 1) / MODEM_SEQ_CHUNK;
  if (lane < nch) {
    const uint32_t  j   = bit0 / MODEM_SEQ_CHUNK + lane;
    const uint32_t* col = x2_cols + (size_t)j * 31;
    const uint4     c1  = *(const uint4*)(x1_bits + (size_t)j * (MODEM_SEQ_CHUNK / 32));
    uint32_t        s2  = 0;
#pragma unroll
    for (int i = 0; i < 31; i++) {
      s2 ^= ((seed >> i) & 1u) ? col[i] : 0u;
    }
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t lo = s2 & 0xffffu;
      s2                = step16_x2(s2);
      const uint32_t hi = s2 & 0xffffu;
      s2                = step16_x2(s2);
      w[k]              = lo | (hi << 16);
    }
    *(uint4*)(cbw + lane * 4) = make_uint4(w[0] ^ c1.x, w[1] ^ c1.y, w[2] ^ c1.z, w[3] ^ c1.w);
  }
  wave_sync_lds();
}

__device__ __forceinline__ uint32_t chips_at(const uint32_t* cb, uint32_t off) // 32 chips starting at tile bit `off`
{
  const uint32_t w = off >> 5, sh = off & 31u;
  const uint64_t two = (uint64_t)cb[w] | ((uint64_t)cb[w + 1] << 32);
  return (uint32_t)(two >> sh);
}

template <typename T>
__device__ __forceinline__ T flip(T v, uint32_t bit)
{
  return bit ? (T)(-(int)v) : v;
}
template <>
__device__ __forceinline__ float flip<float>(float v, uint32_t bit)
{
  return __uint_as_float(__float_as_uint(v) ^ (bit << 31));
}

// ---- stores ---------------------------------------------------------------------------------------------------------------
template <typename T, int QM>
__device__ __forceinline__ void store_bits(T* dst, const T* v, bool aligned)
{
  constexpr int BYTES = QM * (int)sizeof(T);
  if (!aligned || BYTES < 4) {
#pragma unroll
    for (int i = 0; i < QM; i++) {
      dst[i] = v[i];
    }
    return;
  }
  uint32_t w[(BYTES + 3) / 4];
#pragma unroll
  for (int i = 0; i < (BYTES + 3) / 4; i++) {
    w[i] = 0;
  }
  if (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < QM; i++) {
      w[i] = __float_as_uint((float)v[i]);
    }
  } else if (sizeof(T) == 2) {
#pragma unroll
    for (int i = 0; i < QM; i++) {
      w[i / 2] |= ((uint32_t)(uint16_t)(int)v[i]) << (16 * (i & 1));
    }
  } else {
#pragma unroll
    for (int i = 0; i < QM; i++) {
      w[i / 4] |= ((uint32_t)(uint8_t)(int)v[i]) << (8 * (i & 3));
    }
  }
  if (BYTES == 4) {
    *(uint32_t*)dst = w[0];
  } else if (BYTES == 6) { // int8 64-QAM: 2-byte aligned
    uint16_t* d = (uint16_t*)dst;
    d[0]        = (uint16_t)w[0];
    d[1]        = (uint16_t)(w[0] >> 16);
    d[2]        = (uint16_t)w[1];
  } else if (BYTES == 8) {
    *(uint2*)dst = make_uint2(w[0], w[1]);
  } else if (BYTES == 12) {
    uint32_t* d = (uint32_t*)dst;
    d[0]        = w[0];
    d[1]        = w[1];
    d[2]        = w[2];
  } else if (BYTES == 16) {
    *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
  } else if (BYTES == 24) {
    uint2* d = (uint2*)dst;
    d[0]     = make_uint2(w[0], w[1]);
    d[1]     = make_uint2(w[2], w[3]);
    d[2]     = make_uint2(w[4], w[5]);
  } else if (BYTES == 32) {
    uint4* d = (uint4*)dst;
    d[0]     = make_uint4(w[0], w[1], w[2], w[3]);
    d[1]     = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// Soft bits of 64 consecutive symbols whose size per symbol is not a power of two (6, 12, 24 bytes): the lanes' pieces go
// through a wave-private LDS strip (word stride 3 or 6: conflict-free) and leave as 16-byte stores, contiguous over the wave.
template <typename T, int QM>
__device__ __forceinline__ void store_bits_staged(T* wave_dst, const T* v, uint32_t* strip)
{
  constexpr int  BYTES = QM * (int)sizeof(T);
  const uint32_t lane  = threadIdx.x & 63u;
  if (BYTES == 6) {
    uint16_t* h = (uint16_t*)strip + lane * 3;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      h[i] = (uint16_t)((uint32_t)(uint8_t)(int)v[2 * i] | ((uint32_t)(uint8_t)(int)v[2 * i + 1] << 8));
    }
  } else {
    constexpr int W = BYTES / 4;
    uint32_t*     d = strip + lane * W;
#pragma unroll
    for (int i = 0; i < W; i++) {
      if (sizeof(T) == 4) {
        d[i] = __float_as_uint((float)v[i]);
      } else {
        d[i] = (uint32_t)(uint16_t)(int)v[2 * i] | ((uint32_t)(uint16_t)(int)v[2 * i + 1] << 16);
      }
    }
  }
  wave_sync_lds();
  constexpr int NQ = 64 * BYTES / 16;
#pragma unroll
  for (int k = 0; k < (NQ + 63) / 64; k++) {
    const uint32_t q = k * 64 + lane;
    if (q < NQ) {
      ((uint4*)wave_dst)[q] = ((const uint4*)strip)[q];
    }
  }
  __builtin_amdgcn_wave_barrier();
}
} // namespace

} // namespace modem
} // namespace phyhip
