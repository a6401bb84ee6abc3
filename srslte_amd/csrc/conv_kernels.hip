// conv_kernels.hip -- the reference's 16-bit 64-state Viterbi decoder (viterbi37_avx2_16bit.c, decode37_avx2_16bit) with one WAVE per frame and one lane
// per trellis state, and the PDCCH candidate decode (srsran_pdcch_dci_decode: rate de-matcher, quantiser, decoder, CRC) in front of it.  gfx950, wave64.
//
// Forward pass, per step: the three symbols are wave-uniform LDS reads; lane s (new state s) fetches the metrics of its predecessors s >> 1 and
// (s >> 1) + 32 with two ds_bpermute, forms the branch metric of butterfly s >> 1 from its own sign bits, adds, compares and selects in 16-bit wrap
// arithmetic, and the 64 decisions are one ballot word -- bit s is state s, which is the mapping the reference's pack / movemask / byte swap comes to
// (tests/conv_model.py: step_intrinsics against step).  Nothing is normalised and the start metrics are all 0, as in the reference.
//
// Decision words live in LDS, stored by lane 0, and only those the chain-back reads: with tail biting steps L + 6 .. 3 L - 1 (the chain-back reads word
// nbits + 6 and its output stops at bit L), without it steps 6 .. L + 5.  The chain-back takes 64 words per LDS round trip -- lane j loads word base + j --
// and walks them with readlane on a wave-uniform state, so a step is a handful of scalar instructions and never waits on LDS; the 64 bits of a block are
// written by 64 lanes at once.  It starts from state 0 at the last step: the reference's chain-back first reads the six zeroed words past the end, which
// shift any best state out (conv_model.py).
#include "conv_device.h"

#include <climits>

namespace phyhip {
namespace conv {
namespace {

constexpr uint32_t kPoly[3] = {0x6D, 0x4F, 0x57};

__device__ __forceinline__ uint32_t uniform(uint32_t v) // a value every lane holds alike, made known as such
{
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t sign_of(uint32_t butterfly, uint32_t poly) // Branchtab37_sse2[k].c[i]
{
  return (__builtin_popcount((2u * butterfly) & poly) & 1) ? 0xFFFFu : 0u;
}

// the branch metric of butterfly (sg0, sg1, sg2) on the three symbols at sym[p]: avg(avg(t0 ^ s0, t1 ^ s1), t2 ^ s2) >> 3, avg = (a + b + 1) >> 1
__device__ __forceinline__ uint32_t branch_metric(const uint16_t* sym, uint32_t p, uint32_t sg0, uint32_t sg1, uint32_t sg2)
{
  const uint32_t x0 = sg0 ^ sym[p], x1 = sg1 ^ sym[p + 1], x2 = sg2 ^ sym[p + 2];
  return ((((x0 + x1 + 1) >> 1) + x2 + 1) >> 1) >> 3;
}

// One frame on the calling wave (all 64 lanes, block of 64; L and tail wave-uniform).  sym: LDS, 3 L symbols (tail biting: laid out three times by
// wrapping) or 3 (L + 6); words: LDS, nof_words(L, tail) of them; out: L bits, one per byte (global); bits: nullptr or an LDS copy of them.
__device__ __forceinline__ void viterbi_wave(const uint16_t* sym, uint32_t L, bool tail, uint64_t* words, uint8_t* out, uint8_t* bits)
{
  const uint32_t lane = threadIdx.x, bf = lane >> 1, odd = lane & 1;
  const uint32_t sg0 = sign_of(bf, kPoly[0]), sg1 = sign_of(bf, kPoly[1]), sg2 = sign_of(bf, kPoly[2]);
  const int      a0 = (int)(bf * 4), a1 = (int)((bf + 32) * 4);
  const uint32_t nsteps = tail ? 3 * L : L + 6, t_lo = (tail ? L : 0) + 6, n3 = 3 * L;
  uint32_t       m = 0, p = 0;
  uint32_t       metric = branch_metric(sym, 0, sg0, sg1, sg2);
  for (uint32_t t = 0; t < nsteps; t++) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute(a0, (int)m), c = (uint32_t)__builtin_amdgcn_ds_bpermute(a1, (int)m);
    // the next step's branch metric does not wait for the exchange
    p += 3;
    if (tail && p == n3) {
      p = 0;
    }
    const uint32_t next     = t + 1 < nsteps ? branch_metric(sym, p, sg0, sg1, sg2) : 0u;
    const uint32_t m_metric = 8191u - metric;
    const uint32_t x = (a + (odd ? m_metric : metric)) & 0xFFFFu, y = (c + (odd ? metric : m_metric)) & 0xFFFFu;
    const bool     dec = (int16_t)(uint16_t)(x - y) > 0;
    m                  = dec ? y : x;
    metric             = next;
    const uint64_t w   = __ballot(dec);
    if (t >= t_lo && lane == 0) {
      words[t - t_lo] = w;
    }
  }
  __syncthreads();
  const uint32_t nw = nsteps > t_lo ? nsteps - t_lo : 0, span = nw > L ? nw : L;
  uint32_t       state = 0;
  for (int blk = (int)((span + 63) / 64) - 1; blk >= 0; blk--) {
    const uint32_t idx = (uint32_t)blk * 64 + lane;
    const uint64_t w   = idx < nw ? words[idx] : 0; // past the steps that ran: the zeros the reference's clear left
    const int      wlo = (int)(uint32_t)w, whi = (int)(uint32_t)(w >> 32);
    uint64_t       km  = 0;
#pragma unroll
    for (int j = 63; j >= 0; j--) {
      const uint64_t ww = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(whi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane(wlo, j);
      const uint32_t k  = (uint32_t)(ww >> state) & 1u;
      state             = (state >> 1) | (k << 5);
      km |= (uint64_t)k << j;
    }
    if (idx < L) {
      const uint8_t bit = (uint8_t)((km >> lane) & 1u);
      out[idx]          = bit;
      if (bits) {
        bits[idx] = bit;
      }
    }
  }
}

// srsran_vec_quant_fus as the reference's compiler left it: one fused multiply-add, truncation, clamps.  cvttss2si gives INT_MIN outside int32 (and on NaN).
__device__ __forceinline__ uint16_t quant_fus(float gain, float x)
{
  const float v = __builtin_fmaf(gain, x, 32767.5f);
  int         q = (v > -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN;
  q             = q < 0 ? 0 : q;
  q             = q > 65535 ? 65535 : q;
  return (uint16_t)q;
}

__device__ __forceinline__ float wave_max(float v)
{
  for (int o = 32; o > 0; o >>= 1) {
    v = fmaxf(v, __shfl_xor(v, o));
  }
  return v;
}

__global__ __launch_bounds__(64) void viterbi_kernel(const uint8_t* __restrict__ in, const VitJob* __restrict__ jobs, uint8_t* __restrict__ out, uint32_t tail,
                                                     uint32_t words_cap)
{
  extern __shared__ uint64_t dyn[];
  uint64_t*      words = dyn;
  uint16_t*      sym   = reinterpret_cast<uint16_t*>(dyn + words_cap);
  VitJob         job   = jobs[blockIdx.x];
  job.L                = uniform(job.L);
  job.kind             = uniform(job.kind);
  job.o_in             = uniform(job.o_in);
  job.o_out            = uniform(job.o_out);
  const uint32_t lane = threadIdx.x, nsym = 3 * (job.L + (tail ? 0 : 6));
  if (job.kind == IN_US) {
    const uint16_t* src = reinterpret_cast<const uint16_t*>(in + job.o_in);
    for (uint32_t i = lane; i < nsym; i += 64) {
      sym[i] = src[i];
    }
  } else { // srsran_viterbi_decode_f's front end
    const float* src = reinterpret_cast<const float*>(in + job.o_in);
    float        mx  = 1e-9f;
    for (uint32_t i = lane; i < nsym; i += 64) {
      mx = fmaxf(mx, fabsf(src[i]));
    }
    const float gain = job.gain_quant / wave_max(mx);
    for (uint32_t i = lane; i < nsym; i += 64) {
      sym[i] = quant_fus(gain, src[i]);
    }
  }
  __syncthreads();
  viterbi_wave(sym, job.L, tail != 0, words, out + job.o_out, nullptr);
}

__constant__ uint8_t kPermCC[32]    = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
__constant__ uint8_t kPermCCInv[32] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14, 17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};

// what one candidate's decode keeps in LDS
struct DciLds {
  uint64_t words[2 * kDciBits];
  float    rm[kDciSyms];
  uint16_t sym[kDciSyms];
  uint8_t  bits[kDciBits];
};

// One candidate on the calling wave (block of 64): e: its job.E soft bits; row: kDciBits payload bytes, crc_rem (2 bytes, low first), 2 zero bytes;
// dbg_rm / dbg_sym: nullptr or the candidate's kDciSyms-value rows.
__device__ __forceinline__ void dci_wave(const float* __restrict__ e, const DciJob& job, DciLds& s, uint8_t* __restrict__ row, float* __restrict__ dbg_rm,
                                         uint16_t* __restrict__ dbg_sym)
{
  uint64_t* const words = s.words;
  float* const    rm    = s.rm;
  uint16_t* const sym   = s.sym;
  uint8_t* const  bits  = s.bits;
  const uint32_t  lane = threadIdx.x, L = job.nof_bits + 16, n3 = 3 * L;
  // (a) srsran_rm_conv_rx: the lane that owns an output position walks the inputs that land on it in increasing k -- the sum order of the reference's one
  // pass over the input.  The position's first input is its rank among the non-dummy places of the circular buffer; the others follow every 3 L inputs.
  const uint32_t nrows = (L - 1) / 32 + 1, K_p = nrows * 32, ndummy = K_p - L; // ndummy < 32: the dummies are the first ndummy places of row 0
  uint32_t       dmask = 0;                                                    // columns (after the permutation) whose row 0 is a dummy
  for (uint32_t c = 0; c < 32; c++) {
    dmask |= (kPermCC[c] < ndummy ? 1u : 0u) << c;
  }
  float mx = 1e-9f;
  for (uint32_t o = lane; o < n3; o += 64) {
    const uint32_t i = o / 3, s = o - 3 * i, row = (i + ndummy) >> 5, col = kPermCCInv[(i + ndummy) & 31];
    const uint32_t dummies = s * ndummy + __builtin_popcount(dmask & ((1u << col) - 1u)) + ((row > 0 && ((dmask >> col) & 1u)) ? 1u : 0u);
    float          t       = 10000.f; // SRSRAN_RX_NULL, and its comparisons as written
    for (uint32_t k = K_p * s + col * nrows + row - dummies; k < job.E; k += n3) {
      const float v = e[k];
      if (t == 10000.f) {
        t = v;
      } else if (v != 10000.f) {
        t += v;
      }
    }
    t     = t == 10000.f ? 0.f : t;
    rm[o] = t;
    mx    = fmaxf(mx, fabsf(t));
  }
  // (b) srsran_viterbi_decode_f's quantiser with the default gain (pdcch.c never sets another)
  const float gain = 1000.f / wave_max(mx);
  for (uint32_t o = lane; o < kDciSyms; o += 64) {
    const uint16_t q = o < n3 ? quant_fus(gain, rm[o]) : (uint16_t)0;
    if (o < n3) {
      sym[o] = q;
    }
    if (dbg_rm) {
      dbg_rm[o] = o < n3 ? rm[o] : 0.f;
    }
    if (dbg_sym) {
      dbg_sym[o] = q;
    }
  }
  __syncthreads();
  // (c) the decoder over nof_bits + 16 bits with tail biting
  viterbi_wave(sym, L, true, words, row, bits);
  for (uint32_t i = L + lane; i < kDciBits; i += 64) {
    row[i] = 0;
  }
  __syncthreads();
  // (d) crc_rem = the 16 bits after the payload, MSB first, xor the CRC (0x11021) of the payload
  if (lane == 0) {
    uint32_t crc = 0, p_bits = 0;
    for (uint32_t i = 0; i < job.nof_bits; i++) {
      crc = ((crc << 1) ^ ((((crc >> 15) ^ bits[i]) & 1u) ? 0x1021u : 0u)) & 0xFFFFu;
    }
    for (uint32_t i = 0; i < 16; i++) {
      p_bits = (p_bits << 1) | bits[job.nof_bits + i];
    }
    const uint32_t rem = p_bits ^ crc;
    row[kDciBits]      = (uint8_t)(rem & 0xFFu);
    row[kDciBits + 1]  = (uint8_t)(rem >> 8);
    row[kDciBits + 2]  = 0;
    row[kDciBits + 3]  = 0;
  }
}

__device__ __forceinline__ DciJob uniform_job(const DciJob* jobs)
{
  DciJob job   = jobs[blockIdx.x];
  job.first    = uniform(job.first);
  job.E        = uniform(job.E);
  job.nof_bits = uniform(job.nof_bits);
  return job;
}

__global__ __launch_bounds__(64) void pdcch_dci_kernel(const float* __restrict__ llr, const DciJob* __restrict__ jobs, uint8_t* __restrict__ out,
                                                       float* __restrict__ dbg_rm, uint16_t* __restrict__ dbg_sym)
{
  __shared__ DciLds s;
  const DciJob      job = uniform_job(jobs);
  dci_wave(llr + job.first, job, s, out + (size_t)blockIdx.x * kDciOutRow, dbg_rm ? dbg_rm + (size_t)blockIdx.x * kDciSyms : nullptr,
           dbg_sym ? dbg_sym + (size_t)blockIdx.x * kDciSyms : nullptr);
}

// The form behind the device front end (pdcch_kernels.hip): the soft bits are where that kernel left them, EVERY candidate of the search has a wave, and the
// rule of srsran_pdcch_decode_msg (pdcch.c:388-393) runs here: mean = (double sum of |soft bit| in index order) / E, decoded = mean > 0.3 -- bit for bit what
// srsran_hip_pdcch_dci_decode_multi computes on the host (conv_host.cpp).  The 64 lanes widen the candidate's |soft bits| into LDS; lane 0 adds them in index
// order (at most 576 dependent additions: the order is the result).  A candidate that is skipped leaves a zero row (and zero _dbg rows) with its mean.
// out: one kDciResRow-byte row per candidate in the layout of srsran_hip_pdcch_res_t.  With sel.cfi the wave picks its list by the CFI in device memory
// (conv_device.h: DciSel) and leaves, writing nothing, when that list is shorter than its number.
__global__ __launch_bounds__(64) void pdcch_dci_sf_kernel(const float* __restrict__ llr, const DciJob* __restrict__ jobs, uint8_t* __restrict__ out,
                                                          float* __restrict__ dbg_rm, uint16_t* __restrict__ dbg_sym, const DciSel sel)
{
  __shared__ DciLds s;
  __shared__ double mag[kDciMaxE];
  __shared__ double mean_s;
  if (sel.cfi) {
    const uint32_t c = min(uniform(*sel.cfi) - 1u, 2u);
    if (blockIdx.x >= sel.n[c]) {
      return;
    }
    jobs += sel.first[c];
  }
  const DciJob      job  = uniform_job(jobs);
  const uint32_t    lane = threadIdx.x;
  const float*      e    = llr + job.first;
  uint8_t*          row  = out + (size_t)blockIdx.x * kDciResRow;
  for (uint32_t k = lane; k < job.E; k += 64) {
    mag[k] = (double)fabsf(e[k]);
  }
  __syncthreads();
  if (lane == 0) {
    double sum = 0;
    for (uint32_t k = 0; k < job.E; k++) {
      sum = __dadd_rn(sum, mag[k]);
    }
    mean_s = __ddiv_rn(sum, (double)job.E);
  }
  __syncthreads();
  const double mean    = mean_s;
  const bool   decoded = mean > 0.3;
  float*       rm_row  = dbg_rm ? dbg_rm + (size_t)blockIdx.x * kDciSyms : nullptr;
  uint16_t*    sym_row = dbg_sym ? dbg_sym + (size_t)blockIdx.x * kDciSyms : nullptr;
  if (decoded) { // (wave-uniform)
    dci_wave(e, job, s, row, rm_row, sym_row);
  } else {
    for (uint32_t i = lane; i < kDciBits + 4; i += 64) {
      row[i] = 0;
    }
    for (uint32_t o = lane; o < kDciSyms; o += 64) {
      if (rm_row) {
        rm_row[o] = 0.f;
      }
      if (sym_row) {
        sym_row[o] = 0;
      }
    }
  }
  if (lane == 0) { // behind dci_wave's own stores of lane 0 to bytes kDciBits .. kDciBits + 3
    row[kDciBits + 2]                                   = decoded ? 1 : 0;
    row[kDciBits + 3]                                   = 0;
    *reinterpret_cast<float*>(row + kDciBits + 4)       = (float)mean;
  }
}

} // namespace

hipError_t launch_viterbi(const uint8_t* in, const VitJob* jobs, uint8_t* out, uint32_t n, uint32_t Lmax, bool tail_biting, hipStream_t st)
{
  if (n == 0) {
    return hipSuccess;
  }
  if (Lmax == 0 || Lmax > kMaxFrame) {
    return hipErrorInvalidValue;
  }
  const uint32_t words_cap = nof_words(Lmax, tail_biting);
  hipLaunchKernelGGL(viterbi_kernel, dim3(n), dim3(64), lds_bytes(Lmax, tail_biting), st, in, jobs, out, tail_biting ? 1u : 0u, words_cap);
  return hipGetLastError();
}

hipError_t launch_pdcch_dci(const float* llr, const DciJob* jobs, uint8_t* out, float* dbg_rm, uint16_t* dbg_sym, uint32_t n, hipStream_t st)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pdcch_dci_kernel, dim3(n), dim3(64), 0, st, llr, jobs, out, dbg_rm, dbg_sym);
  return hipGetLastError();
}

hipError_t launch_pdcch_dci_sf(const float* llr, const DciJob* jobs, uint8_t* out, float* dbg_rm, uint16_t* dbg_sym, uint32_t n, hipStream_t st, const DciSel* sel)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pdcch_dci_sf_kernel, dim3(n), dim3(64), 0, st, llr, jobs, out, dbg_rm, dbg_sym, sel ? *sel : DciSel{});
  return hipGetLastError();
}

} // namespace conv
} // namespace phyhip
