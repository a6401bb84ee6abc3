// pucch_kernels.hip -- PUCCH receive for gfx950: srsran_chest_ul_estimate_pucch (chest_ul.c:406-578) and srsran_pucch_decode (pucch.c:625-728, :797-872)
// for every job of a call in ONE launch.
//
// One job is one wave; a workgroup carries four jobs that never meet: there is no workgroup barrier, a wave's stages are separated by wave barriers on its
// own LDS strip (about 5.5 KB), and a wave whose job index is behind the call's last leaves at once.  A job is at most 14 x 12 points: what bounds it is the
// length of the dependent chain of stages, not any throughput, so every stage is spread over as many lanes as it has independent pieces and no further.
//
// Sums.  A sum over a row of 12 is formed by ONE lane, k = 0 .. 11 in order; a sum over rows is formed from the rows' sums in row order, by every lane
// alike.  No atomics and no cross-lane arithmetic but the argmax of the CQI search, whose order is total (larger metric, then smaller word): the bits are
// the same on every run and do not depend on which jobs share the call.
//
// Arithmetic.  The arguments of the generated sequences are the reference's float expressions (a float phi pi / 4, the float alpha n, the float cover
// arguments from the host).  From there the estimator and the correlations run in double and are rounded to float where the reference stores a float
// (pilot estimates, the slot rows, z, the measurements): the recorded tolerances are a few float roundings wide, and double against float is not measured.
// The equaliser is the float formula of srsran_predecoding_single with one rounding per operation (modem_arith.h), the demodulator and the descrambler
// are the integer arithmetic of srsran_demod_soft_demodulate_s / srsran_scrambling_s_offset, the CQI metric is the int16 product and int sum of
// srsran_vec_dot_prod_sss over 20 values (its first 16 products wrap to int16 as the SIMD lanes do).
#include "hip_common.h"
#include "modem_arith.h"
#include "pucch_device.h"

#include <cfloat>

namespace phyhip {
namespace pucch {
namespace {

constexpr uint32_t kRows = 2 * kMaxRs; // pilot rows
constexpr uint32_t kParts = 10;        // rows of any row-wise sum: 2 x 5 data symbols at most

struct Strip { // one wave's LDS
  float2  rx[2 * kMaxSymb * kNre];
  float2  pe[kRows][kNre];
  float2  ce[2][kNre];
  float2  z[kMaxZ];
  double2 ref[kMaxZ];
  double  part[kParts][4];
  int     llr[kBits2];
};

__device__ __forceinline__ bool is_normal(float v)
{
  const float a = fabsf(v);
  return a >= FLT_MIN && a <= FLT_MAX;
}

// cexp(j (phi_arg + alpha k)) cexp(j w): the argument is the reference's float expression (zc_sequence.c:270-275, one fused multiply-add), the rest double
__device__ __forceinline__ double2 seq_point(float phi_arg, float alpha, uint32_t k, float w)
{
  const float arg = fmaf(alpha, (float)k, phi_arg);
  double      sa, ca, sw, cw;
  sincos((double)arg, &sa, &ca);
  sincos((double)w, &sw, &cw);
  return make_double2(ca * cw - sa * sw, ca * sw + sa * cw);
}

// conj(z_m_1) v for hypothesis i of srsran_pucch_format2ab_mod_bits: 2A: 1, -1; 2B: 1, j, -j, -1 (bits[0] = i % 2, bits[1] = i / 2)
__device__ __forceinline__ double2 unrotate(double2 v, uint32_t i, bool f2a)
{
  if (i == 0) {
    return v;
  }
  if (f2a || i == 3) {
    return make_double2(-v.x, -v.y);
  }
  return i == 1 ? make_double2(v.y, -v.x) : make_double2(-v.y, v.x);
}

__device__ __forceinline__ uint32_t code_of(const Params& p, uint32_t w)
{
  uint32_t c = 0;
#pragma unroll
  for (uint32_t n = 0; n < kWordBits; n++) {
    c ^= ((w >> (kWordBits - 1 - n)) & 1u) ? p.basis[n] : 0u;
  }
  return c;
}

__global__ __launch_bounds__(64 * kJobsPerBlock) void pucch_kernel(const Params p)
{
  __shared__ Strip strips[kJobsPerBlock];
  const uint32_t   wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t   job  = __builtin_amdgcn_readfirstlane(blockIdx.x * kJobsPerBlock + wave);
  if (job >= p.n_jobs) {
    return;
  }
  Strip&     s = strips[wave];
  const Job& j = p.jobs[job];
  Record     rec = {};
  // every index the job carries is checked before it is used (uniform over the wave)
  bool ok = j.format <= 5 && (j.nsymb == 6 || j.nsymb == 7) && j.n_rs >= 1 && j.n_rs <= kMaxRs && j.nof_uci_bits < kWordBits && (j.filter_len == 0 || j.filter_len == 3);
  ok = ok && (j.format < 4 || j.n_rs == 2); // the 2A / 2B hypothesis sits on the second of two reference symbols
  for (uint32_t sl = 0; ok && sl < 2; sl++) {
    ok = j.N_sf[sl] >= 1 && j.N_sf[sl] <= (j.format <= 2 ? 4u : kMaxSf) && (j.format <= 2 || j.N_sf[sl] == kMaxSf) && j.col[sl] < p.n_cols;
    for (uint32_t i = 0; ok && i < j.N_sf[sl]; i++) {
      ok = j.sym[sl][i] < j.nsymb;
    }
    for (uint32_t i = 0; ok && i < j.n_rs; i++) {
      ok = j.dmrs_sym[sl][i] < j.nsymb;
    }
  }
  if (!ok) {
    if (lane == 0) {
      rec.bad    = 1;
      p.rec[job] = rec;
    }
    return;
  }
  const uint32_t n_rs = j.n_rs, R = 2 * n_rs, slot_pts = j.nsymb * kNre, N_sf0 = j.N_sf[0], n_sym = N_sf0 + j.N_sf[1], nof_re = n_sym * kNre;
  const bool     f1 = j.format <= 2;

  for (uint32_t e = lane; e < 2 * slot_pts; e += 64) {
    const uint32_t sl = e >= slot_pts ? 1u : 0u;
    s.rx[sl * kMaxSymb * kNre + (e - sl * slot_pts)] = p.cols[(size_t)j.col[sl] * slot_pts + (e - sl * slot_pts)];
  }
  modem::wave_sync_lds();

  // ---- least-squares estimates: rx conj(known pilot), z_m_1 = 1
  for (uint32_t e = lane; e < R * kNre; e += 64) {
    const uint32_t r = e / kNre, k = e % kNre, sl = r / n_rs, m = r % n_rs;
    const double2  kn = seq_point(j.phi_arg[sl][k], j.dmrs_alpha[sl][m], k, j.w_dmrs[sl][m]);
    const float2   y  = s.rx[sl * kMaxSymb * kNre + j.dmrs_sym[sl][m] * kNre + k];
    s.pe[r][k]        = make_float2((float)((double)y.x * kn.x + (double)y.y * kn.y), (float)((double)y.y * kn.x - (double)y.x * kn.y));
  }
  modem::wave_sync_lds();

  // ---- formats 2A / 2B: the hypothesis of the second reference symbol (chest_ul.c:450-474): last maximum of |sum|
  if (j.format >= 4) {
    if (lane < R) {
      double2 a = make_double2(0.0, 0.0);
      for (uint32_t k = 0; k < kNre; k++) {
        a.x += (double)s.pe[lane][k].x;
        a.y += (double)s.pe[lane][k].y;
      }
      s.part[lane][0] = a.x;
      s.part[lane][1] = a.y;
    }
    modem::wave_sync_lds();
    double2 S0 = make_double2(0.0, 0.0), S1 = make_double2(0.0, 0.0);
    for (uint32_t r = 0; r < R; r++) {
      double2& t = (r % n_rs) == 1 ? S1 : S0;
      t.x += s.part[r][0];
      t.y += s.part[r][1];
    }
    const bool f2a = j.format == 4;
    float      mx  = -1e9f;
    for (uint32_t i = 0; i < (f2a ? 2u : 4u); i++) {
      const double2 u = unrotate(S1, i, f2a);
      const float   x = (float)hypot(S0.x + u.x, S0.y + u.y);
      if (x >= mx) {
        mx      = x;
        rec.drs = i;
      }
    }
    modem::wave_sync_lds();
    if (lane < 2 * kNre) {
      float2&       v = s.pe[(lane / kNre) * n_rs + 1][lane % kNre];
      const double2 u = unrotate(make_double2((double)v.x, (double)v.y), rec.drs, f2a); // a rotation by a multiple of pi / 2: exact
      v               = make_float2((float)u.x, (float)u.y);
    }
    modem::wave_sync_lds();
  }

  // ---- power and time alignment on the raw estimates (chest_ul.c:482-521)
  if (lane < R) {
    double2 a = make_double2(0.0, 0.0), t = make_double2(0.0, 0.0);
    double  q = 0.0;
    for (uint32_t k = 0; k < kNre; k++) {
      const double x = (double)s.pe[lane][k].x, y = (double)s.pe[lane][k].y;
      a.x += x;
      a.y += y;
      q += x * x + y * y;
      if (k > 0) {
        const double px = (double)s.pe[lane][k - 1].x, py = (double)s.pe[lane][k - 1].y;
        t.x += x * px + y * py;
        t.y += y * px - x * py;
      }
    }
    s.part[lane][0] = a.x;
    s.part[lane][1] = a.y;
    s.part[lane][2] = q;
    s.part[lane][3] = 0.0;
    p.rec[job].ta[lane][0] = (float)t.x;
    p.rec[job].ta[lane][1] = (float)t.y;
  }
  modem::wave_sync_lds();
  {
    double ax = 0.0, ay = 0.0, q = 0.0;
    for (uint32_t r = 0; r < R; r++) {
      ax += s.part[r][0];
      ay += s.part[r][1];
      q += s.part[r][2];
    }
    rec.pe_sum[0] = (float)ax;
    rec.pe_sum[1] = (float)ay;
    rec.epre      = (float)(q / (double)(R * kNre));
  }
  modem::wave_sync_lds();

  // ---- the slot average, in place into the slot's first row (:527-538), then the 3-tap filter with srsran_conv_same_cf's end rule
  if (lane < 2 * kNre) {
    const uint32_t sl = lane / kNre, k = lane % kNre;
    double         x = 0.0, y = 0.0;
    for (uint32_t i = 0; i < n_rs; i++) {
      x += (double)s.pe[sl * n_rs + i][k].x;
      y += (double)s.pe[sl * n_rs + i][k].y;
    }
    const double w      = (double)(1.0f / (float)n_rs);
    s.pe[sl * n_rs][k] = make_float2((float)(x * w), (float)(y * w));
  }
  modem::wave_sync_lds();
  if (lane < 2 * kNre) {
    const uint32_t sl = lane / kNre, k = lane % kNre;
    const float2*  in = s.pe[sl * n_rs];
    float2         o  = in[k];
    if (j.filter_len == 3) {
      float2 a, b;
      if (k > 0) {
        a = in[k - 1];
      } else {
        a = make_float2((float)(3.0 * (double)in[1].x - 2.0 * (double)in[0].x), (float)(3.0 * (double)in[1].y - 2.0 * (double)in[0].y));
      }
      if (k + 1 < kNre) {
        b = in[k + 1];
      } else {
        b = make_float2((float)(3.0 * (double)in[kNre - 1].x - 2.0 * (double)in[kNre - 2].x), (float)(3.0 * (double)in[kNre - 1].y - 2.0 * (double)in[kNre - 2].y));
      }
      const double f0 = (double)j.filter[0], f1c = (double)j.filter[1], f2 = (double)j.filter[2];
      o = make_float2((float)((double)a.x * f0 + (double)o.x * f1c + (double)b.x * f2), (float)((double)a.y * f0 + (double)o.y * f1c + (double)b.y * f2));
    }
    s.ce[sl][k] = o;
  }
  modem::wave_sync_lds();

  // ---- noise (estimate_noise_pilots_pucch, :406-431): every pilot row against its slot's row, AFTER the in-place average
  if (lane < R) {
    const uint32_t sl = lane / n_rs;
    double         q  = 0.0;
    for (uint32_t k = 0; k < kNre; k++) {
      const double dx = (double)modem::rn_sub(s.ce[sl][k].x, s.pe[lane][k].x), dy = (double)modem::rn_sub(s.ce[sl][k].y, s.pe[lane][k].y);
      q += dx * dx + dy * dy;
    }
    s.part[lane][3] = q / (double)kNre;
  }
  modem::wave_sync_lds();
  float noise;
  {
    double power = 0.0;
    for (uint32_t r = 0; r < R; r++) {
      power += s.part[r][3];
    }
    power /= (double)R;
    if (j.filter_len == 3) {
      const float w = j.filter[0];
      const float a = (float)(7.419 * w * w + 0.1117 * w - 0.005387);
      noise         = (float)(power / (a * 0.8));
    } else {
      noise = (float)power;
    }
    if (noise == 0.0f) {
      noise = FLT_MIN;
    }
    rec.noise_estimate = noise;
  }

  Dbg* dbg = p.dbg ? p.dbg + job : nullptr;
  if (dbg) {
    for (uint32_t e = lane; e < kRows * kNre; e += 64) {
      dbg->pe[e / kNre][e % kNre] = e < R * kNre ? s.pe[e / kNre][e % kNre] : make_float2(0.f, 0.f);
    }
    if (lane < 2 * kNre) {
      dbg->ce[lane / kNre][lane % kNre] = s.ce[lane / kNre][lane % kNre];
    }
    if (lane < kBits2) {
      dbg->llr[lane] = 0;
    }
  }

  // ---- pucch_get of data and ce, srsran_predecoding_single with the job's own noise estimate
  if (j.decode) {
    for (uint32_t e = lane; e < nof_re; e += 64) {
      const uint32_t si = e / kNre, k = e % kNre, sl = si >= N_sf0 ? 1u : 0u, m = si - sl * N_sf0;
      const float2   y = s.rx[sl * kMaxSymb * kNre + j.sym[sl][m] * kNre + k], h = s.ce[sl][k];
      float          c = modem::rn_add(modem::rn_mul(h.x, h.x), modem::rn_mul(h.y, h.y));
      if (noise > 0.f) {
        c = modem::rn_add(c, noise);
      }
      s.z[e] = make_float2(modem::rn_div(modem::rn_add(modem::rn_mul(y.x, h.x), modem::rn_mul(y.y, h.y)), c),
                           modem::rn_div(modem::rn_sub(modem::rn_mul(y.y, h.x), modem::rn_mul(y.x, h.y)), c));
      s.ref[e] = seq_point(j.phi_arg[sl][k], j.alpha[sl][m], k, f1 ? j.w_data[sl][m] : 0.0f);
    }
    modem::wave_sync_lds();
    if (dbg) {
      for (uint32_t e = lane; e < kMaxZ; e += 64) {
        dbg->z[e] = e < nof_re ? s.z[e] : make_float2(0.f, 0.f);
      }
    }
  } else if (dbg) {
    for (uint32_t e = lane; e < kMaxZ; e += 64) {
      dbg->z[e] = make_float2(0.f, 0.f);
    }
  }

  // ---- the DMRS detection ratio (pucch.c:828-840) on the first 12 points of the extracted ce: slot 0's row
  if (j.decode && j.dmrs_detection) {
    double ax = 0.0, ay = 0.0, q = 0.0;
    for (uint32_t k = 0; k < kNre; k++) {
      const double x = (double)s.ce[0][k].x, y = (double)s.ce[0][k].y;
      ax += x;
      ay += y;
      q += x * x + y * y;
    }
    ax /= (double)kNre;
    ay /= (double)kNre;
    rec.dmrs_correlation = (float)((ax * ax + ay * ay) / (q / (double)kNre));
    if (!is_normal(rec.dmrs_correlation) || rec.dmrs_correlation < j.threshold_dmrs) {
      rec.early = 1;
    }
  }

  if (j.decode && !rec.early && f1) {
    // ---- formats 1 / 1A / 1B: every candidate is the regenerated signal times d in {1, -1, j, -j}: one complex correlation serves them all
    if (lane < n_sym) {
      double cx = 0.0, cy = 0.0, sx = 0.0, sy = 0.0;
      for (uint32_t k = 0; k < kNre; k++) {
        const float2  z = s.z[lane * kNre + k];
        const double2 r = s.ref[lane * kNre + k];
        cx += (double)z.x * r.x + (double)z.y * r.y; // z conj(ref)
        cy += (double)z.y * r.x - (double)z.x * r.y;
        sx += (double)z.x * (double)z.x + (double)z.y * (double)z.y;
        sy += r.x * r.x + r.y * r.y;
      }
      s.part[lane][0] = cx;
      s.part[lane][1] = cy;
      s.part[lane][2] = sx;
      s.part[lane][3] = sy;
    }
    modem::wave_sync_lds();
    double cx = 0.0, cy = 0.0, sx = 0.0, sy = 0.0;
    for (uint32_t r = 0; r < n_sym; r++) {
      cx += s.part[r][0];
      cy += s.part[r][1];
      sx += s.part[r][2];
      sy += s.part[r][3];
    }
    const double len = (double)nof_re, den = sqrt((sx / len) * (sy / len));
    // cov of candidate d: Re(conj(d) C).  1A: b = 0, 1 -> d = 1, -1; 1B: (b, b2) = 00, 01, 10, 11 -> d = 1, -j, j, -1
    const double cov[4]  = {cx, j.format == 1 ? -cx : -cy, cy, -cx};
    const uint32_t n_cand = j.format == 0 ? 1u : j.format == 1 ? 2u : 4u;
    float          best   = -1e9f;
    for (uint32_t c = 0; c < n_cand; c++) {
      const float corr = (float)((cov[c] / len) / den);
      if (j.format == 0) {
        best = corr;
      } else if (corr > best) {
        best     = corr;
        rec.word = c;
      }
    }
    rec.correlation = best;
  } else if (j.decode && !rec.early) {
    // ---- formats 2 / 2A / 2B: the 12 products of a symbol averaged, QPSK to int16, descrambled (pucch.c:690-715)
    if (lane < 2 * kMaxSf) {
      double x = 0.0, y = 0.0;
      for (uint32_t k = 0; k < kNre; k++) {
        const float2  z = s.z[lane * kNre + k];
        const double2 r = s.ref[lane * kNre + k];
        x += (double)z.x * r.x + (double)z.y * r.y;
        y += (double)z.y * r.x - (double)z.x * r.y;
      }
      const float d[2] = {(float)(x / (double)kNre), (float)(y / (double)kNre)};
#pragma unroll
      for (uint32_t c = 0; c < 2; c++) {
        const uint32_t i = 2 * lane + c;
        const int      t = modem::cvt_tr(modem::rn_mul(d[c], p.qpsk_s));
        int            v = i < 16 ? modem::sat16(t) : (int)(int16_t)t; // vector_simd.c: 16 values per iteration saturate, the scalar remainder wraps
        if ((j.scramble >> i) & 1u) {
          v = (int)(int16_t)(-v);
        }
        s.llr[i] = v;
      }
    }
    modem::wave_sync_lds();
    int   llr[kBits2], neg[kBits2];
    float acc = 0.f;
#pragma unroll
    for (uint32_t i = 0; i < kBits2; i++) {
      llr[i]        = s.llr[i];
      neg[i]        = i < 16 ? (int)(int16_t)(-llr[i]) : -llr[i];
      const float t = (float)llr[i];
      acc           = fmaf(t, t, acc); // srsran_vec_avg_power_sf
    }
    rec.llr_pow = modem::rn_div(acc, (float)kBits2);
    if (dbg && lane < kBits2) {
      dbg->llr[lane] = (int16_t)s.llr[lane];
    }
    // srsran_uci_decode_cqi_pucch: lanes over words; word j << sh, j = 64 q + lane: its code is the lane's part xor the round's part
    const uint32_t sh = kWordBits - j.nof_uci_bits, nw = 1u << j.nof_uci_bits;
    const uint32_t c_lane = code_of(p, (lane << sh) & 0x1fffu);
    int            best   = INT32_MIN;
    uint32_t       best_w = 0;
    for (uint32_t q = 0; q * 64 < nw; q++) {
      const uint32_t idx = q * 64 + lane, c = c_lane ^ code_of(p, ((q * 64) << sh) & 0x1fffu);
      int            corr = 0;
#pragma unroll
      for (uint32_t i = 0; i < kBits2; i++) {
        corr += ((c >> i) & 1u) ? llr[i] : neg[i];
      }
      if (idx < nw && corr > best) {
        best   = corr;
        best_w = idx << sh;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int      ob = __shfl_xor(best, off);
      const uint32_t ow = (uint32_t)__shfl_xor((int)best_w, off);
      if (ob > best || (ob == best && ow < best_w)) {
        best   = ob;
        best_w = ow;
      }
    }
    rec.max_corr = best;
    rec.word     = best_w;
  }

  if (lane == 0) { // (ta[][] was filed by the rows' lanes)
    Record* o           = p.rec + job;
    o->noise_estimate   = rec.noise_estimate;
    o->epre             = rec.epre;
    o->pe_sum[0]        = rec.pe_sum[0];
    o->pe_sum[1]        = rec.pe_sum[1];
    o->correlation      = rec.correlation;
    o->dmrs_correlation = rec.dmrs_correlation;
    o->llr_pow          = rec.llr_pow;
    o->max_corr         = rec.max_corr;
    o->word             = rec.word;
    o->drs              = rec.drs;
    o->early            = rec.early;
    o->bad              = 0;
  }
  if (lane >= R && lane < kRows) {
    p.rec[job].ta[lane][0] = 0.f;
    p.rec[job].ta[lane][1] = 0.f;
  }
}

} // namespace

hipError_t launch(const Params& p, hipStream_t stream)
{
  if (p.n_jobs == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pucch_kernel, dim3((p.n_jobs + kJobsPerBlock - 1) / kJobsPerBlock), dim3(64 * kJobsPerBlock), 0, stream, p);
  return hipGetLastError();
}

} // namespace pucch
} // namespace phyhip
