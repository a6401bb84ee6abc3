// conv_device.h -- what conv_host.cpp and conv_kernels.hip share: the jobs of the Viterbi and PDCCH kernels and their launches.
#pragma once
#include "hip_common.h"
#include "srsran_amd/phy_conv_abi.h"

namespace phyhip {
namespace conv {

constexpr uint32_t kMaxFrame  = 2048; // SRSRAN_HIP_VITERBI_MAX_FRAMEBITS
constexpr uint32_t kDciBits   = 144;  // SRSRAN_HIP_DCI_MAX_BITS + 16
constexpr uint32_t kDciSyms   = 3 * kDciBits;
constexpr uint32_t kDciOutRow = kDciBits + 4; // payload, crc_rem (uint16), two bytes of padding
constexpr uint32_t kDciResRow = kDciBits + 8; // srsran_hip_pdcch_res_t: payload, crc_rem, decoded (uint16), mean (float)
constexpr uint32_t kDciMaxE   = 576;          // soft bits of a candidate at aggregation level 3

enum : uint32_t { IN_US = 0, IN_F32 = 1 };

struct VitJob { // one frame, one wave
  uint32_t o_in;  // byte offset of the frame's symbols in the input image: uint16 (IN_US) or float (IN_F32), 3 L with tail biting, 3 (L + 6) without
  uint32_t L;     // frame bits, 1 .. kMaxFrame
  uint32_t o_out; // byte offset of the L decoded bits (one per byte) in the output image
  uint32_t kind;
  float    gain_quant; // IN_F32
};

struct DciJob { // one candidate, one wave
  uint32_t first;    // index of the candidate's first soft bit in the region
  uint32_t E;        // soft bits: 72 << L
  uint32_t nof_bits; // 1 .. 128
};
// host side: nullptr, or why a candidate is refused in a region of nof_llr soft bits (`past`: the caller's sentence for a location outside it)
inline const char* dci_cand_invalid(const srsran_hip_pdcch_cand_t& c, uint64_t nof_llr, const char* past = "a location past the end of the control region")
{
  if (c.L > 3) {
    return "aggregation level above 3";
  }
  if ((uint64_t)c.ncce * 72 + (72u << c.L) > nof_llr) {
    return past;
  }
  if (c.nof_bits == 0 || c.nof_bits > SRSRAN_HIP_DCI_MAX_BITS) {
    return "nof_bits outside 1 .. 128";
  }
  return nullptr;
}
inline DciJob dci_job(const srsran_hip_pdcch_cand_t& c) // of a candidate that has passed
{
  return DciJob{c.ncce * 72, 72u << c.L, c.nof_bits};
}

// decision words a frame keeps in LDS: with tail biting those of steps L + 6 .. 3 L - 1, without those of steps 6 .. L + 5
inline uint32_t nof_words(uint32_t L, bool tail_biting)
{
  return tail_biting ? (2 * L > 6 ? 2 * L - 6 : 0) : L;
}
inline size_t lds_bytes(uint32_t Lmax, bool tail_biting) // of a launch whose longest frame has Lmax bits
{
  return (size_t)nof_words(Lmax, tail_biting) * 8 + (size_t)3 * (Lmax + 6) * 2;
}

// in / out: device images the jobs' offsets refer to; n waves
hipError_t launch_viterbi(const uint8_t* in, const VitJob* jobs, uint8_t* out, uint32_t n, uint32_t Lmax, bool tail_biting, hipStream_t st);
// out: n rows of kDciOutRow bytes; dbg_rm / dbg_sym: nullptr or n rows of kDciSyms values
hipError_t launch_pdcch_dci(const float* llr, const DciJob* jobs, uint8_t* out, float* dbg_rm, uint16_t* dbg_sym, uint32_t n, hipStream_t st);
// a search whose CFI a kernel ahead on the stream leaves in device memory (ctrl_kernels.hip): `jobs` holds the lists of CFI 1, 2 and 3 one behind the other,
// the launch has max(n[]) waves, a wave reads *cfi (1 .. 3), takes job first[cfi - 1] + its number of that list and leaves when the list is shorter
struct DciSel {
  const uint32_t* cfi; // nullptr: one list, every wave has a job
  uint32_t        first[3], n[3];
};
// the form with the mean rule on the device: a wave per candidate of the search, skipped or not; out: n rows of kDciResRow bytes (srsran_hip_pdcch_res_t)
hipError_t launch_pdcch_dci_sf(const float* llr, const DciJob* jobs, uint8_t* out, float* dbg_rm, uint16_t* dbg_sym, uint32_t n, hipStream_t st,
                               const DciSel* sel = nullptr);

} // namespace conv
} // namespace phyhip
