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
#include "conv_wave.h"

namespace phyhip {
namespace conv {
namespace {

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
  // (a) srsran_rm_conv_rx on the candidate's soft bits (conv_wave.h)
  const float mx = rm_conv_wave([e](uint32_t k) { return e[k]; }, job.E, L, rm);
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
    const uint32_t rem = crc_rem(bits, job.nof_bits);
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
