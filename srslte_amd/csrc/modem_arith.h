// modem_arith.h -- the device functions the demodulating kernels share (modem_kernels.hip, nr_chan_kernels.hip, txdiv_kernels.hip, spmux_kernels.hip): the
// integer soft-bit arithmetic of demod_soft.c as the x86 reference evaluates it, the transmit-diversity combiner, the 2x2 spatial-multiplexing / CDD
// equalisers and precoders, the Gold-sequence chips of one wave, sign flips, the soft-bit stores and the scrambled constellation point.  Device code only.
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
// The two gains are what the grant calls file as the codeword's CSI (txdiv_front_kernel<T, true>) and what srsran_predecoding_diversity_multi files
// (txdiv_eq_kernel): they go through rn_mul / rn_add (defined with the 2x2 section below: contraction off), so that the two kernels agree on them bit for
// bit whatever the compiler fuses elsewhere -- with the plain operators the 4-port, 2-antenna sums came out one unit apart between the two kernels.
__device__ __forceinline__ float rn_mul(float a, float b);
__device__ __forceinline__ float rn_add(float a, float b);
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
  a.g0 = rn_add(a.g0, rn_add(rn_add(rn_add(rn_mul(ha.x, ha.x), rn_mul(ha.y, ha.y)), rn_mul(hb.x, hb.x)), rn_mul(hb.y, hb.y)));
  if (PORTS == 2) {
    a.g0 = a.g0 == 0.f ? 1e-4f : a.g0;
  } else {
    a.g1 = rn_add(a.g1, rn_add(rn_add(rn_add(rn_mul(hd.x, hd.x), rn_mul(hd.y, hd.y)), rn_mul(hc.x, hc.x)), rn_mul(hc.y, hc.y)));
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

// ---- four ports WITHOUT CSI: srsran_predecoding_diversity_gen_ (mimo/precoding.c:465-498), the body srsran_predecoding_diversity_multi runs when csi is
// NULL -- which the PDSCH never does and the PDCCH always does (pdcch.c:473; pdcch_kernels.hip).  It is NOT the formula above: one quad of REs (r0 .. r3 on
// sub-carriers 4i .. 4i + 3) reads ports 0 and 2 at 4i (h0, h2) and ports 1 and 3 at 4i + 2 (h1, h3) for all four layers, and each pair of layers shares
// one gain:
//   x0 += conj(h0) r0 + h2 conj(r1)   x1 += -h2 conj(r0) + conj(h0) r1   g02 += |h0|^2 + |h2|^2
//   x2 += conj(h1) r2 + h3 conj(r3)   x3 += -h3 conj(r2) + conj(h1) r3   g13 += |h1|^2 + |h3|^2      per receive antenna,
// then x / (g scaling) * M_SQRT2 (sfbc_quot).  No replacement value: a quad whose gain is 0 gives what the formula gives.  Operation order as written there,
// every product, sum and quotient rounded by itself: the two complex products of a symbol are formed, added to each other, then to the accumulator; a gain's
// four squares are summed left to right, then added.
__device__ __forceinline__ float rn_sub(float a, float b);
struct Sfbc4 {
  float2 x[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  float  g02 = 0.f, g13 = 0.f;
};
__device__ __forceinline__ void sfbc4_pair(float2& xa, float2& xb, float& g, float2 hp, float2 hq, float2 ra, float2 rb)
{
  const float ar = rn_add(rn_mul(hp.x, ra.x), rn_mul(hp.y, ra.y)); // conj(hp) ra
  const float ai = rn_sub(rn_mul(hp.x, ra.y), rn_mul(hp.y, ra.x));
  const float br = rn_add(rn_mul(hq.x, rb.x), rn_mul(hq.y, rb.y)); // hq conj(rb)
  const float bi = rn_sub(rn_mul(hq.y, rb.x), rn_mul(hq.x, rb.y));
  const float cr = rn_add(rn_mul(hp.x, rb.x), rn_mul(hp.y, rb.y)); // conj(hp) rb
  const float ci = rn_sub(rn_mul(hp.x, rb.y), rn_mul(hp.y, rb.x));
  const float dr = rn_add(rn_mul(hq.x, ra.x), rn_mul(hq.y, ra.y)); // hq conj(ra)
  const float di = rn_sub(rn_mul(hq.y, ra.x), rn_mul(hq.x, ra.y));
  xa             = make_float2(rn_add(xa.x, rn_add(ar, br)), rn_add(xa.y, rn_add(ai, bi)));
  xb             = make_float2(rn_add(xb.x, rn_sub(cr, dr)), rn_add(xb.y, rn_sub(ci, di)));
  g              = rn_add(g, rn_add(rn_add(rn_add(rn_mul(hp.x, hp.x), rn_mul(hp.y, hp.y)), rn_mul(hq.x, hq.x)), rn_mul(hq.y, hq.y)));
}
__device__ __forceinline__ void sfbc4_add(Sfbc4& a, float2 h0, float2 h1, float2 h2, float2 h3, float2 r0, float2 r1, float2 r2, float2 r3)
{
  sfbc4_pair(a.x[0], a.x[1], a.g02, h0, h2, r0, r1);
  sfbc4_pair(a.x[2], a.x[3], a.g13, h1, h3, r2, r3);
}
__device__ __forceinline__ void sfbc4_finish(const Sfbc4& a, float scaling, float2* x)
{
  const float d02 = rn_mul(a.g02, scaling), d13 = rn_mul(a.g13, scaling);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const float d = l < 2 ? d02 : d13;
    x[l]          = make_float2(sfbc_quot(a.x[l].x, d), sfbc_quot(a.x[l].y, d));
  }
}

// ---- 2x2 spatial multiplexing and large-delay CDD on 2 ports, 2 receive antennas (mimo/precoding.c:841-1812 receive, :2044-2203 transmit; utils/mat.c:63-109):
// the one arithmetic of the per-stage kernels and the fused kernels of spmux_kernels.hip.  Operation order: that of the reference's scalar loop bodies
// (the `for (; i < nof_symbols; ...)` tails, the _csi variants), a complex product evaluated as C does ((ar br - ai bi) + j (ar bi + ai br)), every
// product, sum and quotient rounded by itself (rn_mul / rn_add / rn_sub / rn_div below: nothing contracts); a multiplication by +-j is a swap and a sign.  No replacement value anywhere: a
// singular channel gives what the formula gives (inf / NaN).
// One rounding per operation, kept HERE and not in a build flag: to this compiler __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn are the plain operators
// (__clang_hip_math.h), which hipcc's default contraction fuses into FMAs -- differently in different kernels: the per-stage and the fused kernel of
// spmux_kernels.hip once differed by one unit in 2 of 9600 soft bits.  The pragma takes the contract flag off these operations wherever they are inlined.
__device__ __forceinline__ float rn_mul(float a, float b)
{
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b)
{
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b)
{
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float rn_div(float a, float b)
{
#pragma clang fp contract(off)
  return a / b;
}
__device__ __forceinline__ float2 lo(const float4 v)
{
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ float2 hi(const float4 v)
{
  return make_float2(v.z, v.w);
}
__device__ __forceinline__ float2 cx_add(float2 a, float2 b)
{
  return make_float2(rn_add(a.x, b.x), rn_add(a.y, b.y));
}
__device__ __forceinline__ float2 cx_sub(float2 a, float2 b)
{
  return make_float2(rn_sub(a.x, b.x), rn_sub(a.y, b.y));
}
__device__ __forceinline__ float2 cx_mul(float2 a, float2 b)
{
  return make_float2(rn_sub(rn_mul(a.x, b.x), rn_mul(a.y, b.y)), rn_add(rn_mul(a.x, b.y), rn_mul(a.y, b.x)));
}
__device__ __forceinline__ float2 cx_conj(float2 a)
{
  return make_float2(a.x, -a.y);
}
__device__ __forceinline__ float2 cx_neg(float2 a)
{
  return make_float2(-a.x, -a.y);
}
__device__ __forceinline__ float2 cx_scale(float2 a, float s)
{
  return make_float2(rn_mul(a.x, s), rn_mul(a.y, s));
}

// one column of a 2-port codebook applied to the channel of one receive antenna (a: port 0, b: port 1).  kind (modem_device.h) 0: a + b, 1: a - b,
// 2: a + j b, 3: a - j b
__device__ __forceinline__ float2 pre_column(float2 a, float2 b, uint32_t kind)
{
  switch (kind) {
    case PRE_PLUS:
      return cx_add(a, b);
    case PRE_MINUS:
      return cx_sub(a, b);
    case PRE_PLUS_J:
      return make_float2(rn_sub(a.x, b.y), rn_add(a.y, b.x));
    default:
      return make_float2(rn_add(a.x, b.y), rn_sub(a.y, b.x));
  }
}
// the effective channel of two layers, Heff[rx][layer], from h[port][rx] (a0 = h[0][0], b0 = h[1][0], a1 = h[0][1], b1 = h[1][1]).
// pre (modem_device.h) 0: identity (codebook 0); 1: columns (+, -) (codebook 1, CDD on an even RE); 2: (+j, -j) (codebook 2); 3: (-, +) (CDD on an odd RE)
struct Heff {
  float2 h00, h01, h10, h11;
};
__device__ __forceinline__ Heff mimo2x2_heff(float2 a0, float2 b0, float2 a1, float2 b1, uint32_t pre)
{
  if (pre == HEFF_IDENT) {
    return Heff{a0, b0, a1, b1};
  }
  const uint32_t k0 = pre == HEFF_PM ? PRE_PLUS : pre == HEFF_J ? PRE_PLUS_J : PRE_MINUS;
  const uint32_t k1 = pre == HEFF_PM ? PRE_MINUS : pre == HEFF_J ? PRE_MINUS_J : PRE_PLUS;
  return Heff{pre_column(a0, b0, k0), pre_column(a0, b0, k1), pre_column(a1, b1, k0), pre_column(a1, b1, k1)};
}
// zero forcing (precoding.c:905-909, :1324-1328): det = h00 h11 - h01 h10, d = conj(det) (norm / |det|^2), x0 = (h11 y0 - h01 y1) d, x1 = (-h10 y0 + h00 y1) d
__device__ __forceinline__ void mimo2x2_zf(float2 y0, float2 y1, const Heff& h, float norm, float2& x0, float2& x1)
{
  const float2 det = cx_sub(cx_mul(h.h00, h.h11), cx_mul(h.h01, h.h10));
  const float  q   = rn_div(norm, rn_add(rn_mul(det.x, det.x), rn_mul(det.y, det.y)));
  const float2 d   = cx_scale(cx_conj(det), q);
  x0               = cx_mul(cx_sub(cx_mul(h.h11, y0), cx_mul(h.h01, y1)), d);
  x1               = cx_mul(cx_add(cx_mul(cx_neg(h.h10), y0), cx_mul(h.h00, y1)), d);
}
// MMSE, srsran_mat_2x2_mmse_csi_gen (utils/mat.c:63-109): A = H^H H + noise I, B = norm A^-1, W = B H^H, x = W y, csi_k = 1 / Re(B_kk)
__device__ __forceinline__ void mimo2x2_mmse(float2 y0, float2 y1, const Heff& h, float noise, float norm, float2& x0, float2& x1, float& csi0, float& csi1)
{
  const float2 c00 = cx_conj(h.h00), c01 = cx_conj(h.h01), c10 = cx_conj(h.h10), c11 = cx_conj(h.h11);
  float2       a00 = cx_add(cx_mul(c00, h.h00), cx_mul(c10, h.h10));
  const float2 a01 = cx_add(cx_mul(c00, h.h01), cx_mul(c10, h.h11));
  const float2 a10 = cx_add(cx_mul(c01, h.h00), cx_mul(c11, h.h10));
  float2       a11 = cx_add(cx_mul(c01, h.h01), cx_mul(c11, h.h11));
  a00.x            = rn_add(a00.x, noise);
  a11.x            = rn_add(a11.x, noise);
  const float2 det = cx_sub(cx_mul(a00, a11), cx_mul(a01, a10));
  const float  dn  = rn_add(rn_mul(det.x, det.x), rn_mul(det.y, det.y));
  const float2 nr  = cx_scale(make_float2(rn_div(det.x, dn), rn_div(-det.y, dn)), norm);
  const float2 b00 = cx_mul(a11, nr), b01 = cx_mul(cx_neg(a01), nr), b10 = cx_mul(cx_neg(a10), nr), b11 = cx_mul(a00, nr);
  const float2 w00 = cx_add(cx_mul(b00, c00), cx_mul(b01, c01)), w01 = cx_add(cx_mul(b00, c10), cx_mul(b01, c11));
  const float2 w10 = cx_add(cx_mul(b10, c00), cx_mul(b11, c01)), w11 = cx_add(cx_mul(b10, c10), cx_mul(b11, c11));
  x0               = cx_add(cx_mul(y0, w00), cx_mul(y1, w01));
  x1               = cx_add(cx_mul(y0, w10), cx_mul(y1, w11));
  csi0             = rn_div(1.0f, b00.x);
  csi1             = rn_div(1.0f, b11.x);
}
// one layer, maximum-ratio combining over the two receive antennas (precoding.c:1805-1809): g = |h0|^2 + |h1|^2, x = (conj(h0) y0 + conj(h1) y1) (norm / g),
// csi = g / norm * (float)M_SQRT1_2
__device__ __forceinline__ void mrc2(float2 y0, float2 y1, float2 h0, float2 h1, float norm, float2& x, float& csi)
{
  const float g = rn_add(rn_add(rn_add(rn_mul(h0.x, h0.x), rn_mul(h0.y, h0.y)), rn_mul(h1.x, h1.x)), rn_mul(h1.y, h1.y));
  x             = cx_scale(cx_add(cx_mul(cx_conj(h0), y0), cx_mul(cx_conj(h1), y1)), rn_div(norm, g));
  csi           = rn_mul(rn_div(g, norm), 0.70710678118654752440f);
}
// one RE of the receive side: `layers` 2 with `pre` a HEFF_* value, or 1 with `pre` a PRE_* value (codebook_idx); x1 / c1 are written with two layers only
__device__ __forceinline__ void mimo_equalise(uint32_t layers, uint32_t pre, bool mmse, float2 y0, float2 y1, float2 a0, float2 b0, float2 a1, float2 b1, float norm,
                                              float noise, float2& x0, float2& x1, float& c0, float& c1)
{
  if (layers == 1) {
    mrc2(y0, y1, pre_column(a0, b0, pre), pre_column(a1, b1, pre), norm, x0, c0);
  } else {
    const Heff h = mimo2x2_heff(a0, b0, a1, b1, pre);
    if (mmse) {
      mimo2x2_mmse(y0, y1, h, noise, norm, x0, x1, c0, c1);
    } else {
      mimo2x2_zf(y0, y1, h, norm, x0, x1);
      c0 = c1 = 1.0f;
    }
  }
}
// one RE of the transmit side (precoding.c:2044-2053, :2097-2195): layer symbols x0, x1 -> port symbols y0, y1; `s` is the reference's float factor (host
// evaluated: scaling / 2, or (float)(scaling * M_SQRT1_2) for one layer and for codebook 0).  kind (modem_device.h): TXPRE_CDD + (RE index & 1),
// TXPRE_MUX2 + codebook_idx (two layers), TXPRE_MUX1 + codebook_idx (one layer, x1 unused)
__device__ __forceinline__ void mimo_precode(uint32_t kind, float2 x0, float2 x1, float s, float2& y0, float2& y1)
{
  switch (kind) {
    case TXPRE_CDD + 1: // odd RE: y1 = (-x0 + x1) s
      y0 = cx_scale(cx_add(x0, x1), s);
      y1 = cx_scale(cx_add(cx_neg(x0), x1), s);
      break;
    case TXPRE_MUX2: // codebook 0: the identity
      y0 = cx_scale(x0, s);
      y1 = cx_scale(x1, s);
      break;
    case TXPRE_MUX2 + 2: { // y1 = j (x0 - x1) s
      const float2 d = cx_sub(x0, x1);
      y0             = cx_scale(cx_add(x0, x1), s);
      y1             = cx_scale(make_float2(-d.y, d.x), s);
    } break;
    case TXPRE_MUX1:
      y0 = y1 = cx_scale(x0, s);
      break;
    case TXPRE_MUX1 + 1:
      y0 = cx_scale(x0, s);
      y1 = cx_scale(x0, -s);
      break;
    case TXPRE_MUX1 + 2:
      y0 = cx_scale(x0, s);
      y1 = make_float2(-y0.y, y0.x);
      break;
    case TXPRE_MUX1 + 3:
      y0 = cx_scale(x0, s);
      y1 = make_float2(y0.y, -y0.x);
      break;
    default: // TXPRE_CDD on an even RE, TXPRE_MUX2 + 1: y1 = (x0 - x1) s
      y0 = cx_scale(cx_add(x0, x1), s);
      y1 = cx_scale(cx_sub(x0, x1), s);
      break;
  }
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
// ---- transmit (txdiv_kernels.hip, spmux_kernels.hip).  Symbol s of the codeword (ls: counted from the wave's first): its Qm packed bits (mod_tile of
// modem_kernels.hip), scrambled with the wave's chips, as a constellation point
template <int MOD>
__device__ __forceinline__ float2 mod_point(const uint8_t* bits, uint32_t nbytes, const float2* tab, uint32_t s, uint32_t ls, const uint32_t* cbw)
{
  constexpr int  QM = MOD == 0 ? 1 : 2 * MOD;
  const uint32_t b = s * QM, by = b >> 3;
  const uint32_t hi8 = bits[by], lo8 = by + 1 < nbytes ? bits[by + 1] : 0u;
  uint32_t       v   = (((hi8 << 8) | lo8) >> (16 - QM - (b & 7u))) & ((1u << QM) - 1u); // bit 0 of the symbol = MSB of v
  const uint32_t c   = chips_at(cbw, ls * QM);                                           // chip i of the symbol in bit i
#pragma unroll
  for (int i = 0; i < QM; i++) {
    v ^= ((c >> i) & 1u) << (QM - 1 - i);
  }
  return tab[v];
}
} // namespace

} // namespace modem
} // namespace phyhip
