// pucch_device.h -- what pucch_kernels.hip and pucch_host.cpp share: the device job (built by pucch_map.h from the plan), the record a job leaves, the
// intermediates of the _dbg and estimator calls, the parameter block and the launcher.  Plain C++ but for the stream type.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace phyhip {
namespace pucch {

constexpr uint32_t kNre      = 12;
constexpr uint32_t kMaxRs    = 3;   // reference symbols per slot
constexpr uint32_t kMaxSf    = 5;   // data symbols per slot
constexpr uint32_t kMaxSymb  = 7;   // symbols per slot
constexpr uint32_t kMaxZ     = 2 * kMaxSf * kNre; // SRSRAN_PUCCH_MAX_SYMBOLS
constexpr uint32_t kBits2    = 20;  // SRSRAN_PUCCH2_NOF_BITS
constexpr uint32_t kWordBits = 13;  // SRSRAN_UCI_MAX_CQI_LEN_PUCCH
constexpr uint32_t kJobsPerBlock = 4; // one wave per job

// A column block: the nsymb x 12 points of one slot at one PRB, row by row.  Jobs that share a PRB share its block.
struct Job {
  uint32_t format;           // srsran_pucch_format_t: 0 .. 5
  uint32_t nsymb;            // 7 or 6
  uint32_t n_rs;
  uint32_t N_sf[2];
  uint32_t col[2];           // column block of each slot
  uint32_t sym[2][kMaxSf];   // data symbols of the slot
  uint32_t dmrs_sym[2][kMaxRs];
  float    alpha[2][kMaxSf]; // the reference's float: (float)(2 pi n_cs / 12)
  float    dmrs_alpha[2][kMaxRs];
  float    w_data[2][kMaxSf]; // formats 1x: w_n_oc[N_sf == 3][n_oc % 3][m] + S_ns, the float sum
  float    w_dmrs[2][kMaxRs]; // w_arg[m]
  float    phi_arg[2][kNre];  // phi(u) (float)M_PI_4, the float product
  uint32_t scramble;          // formats 2x: chip i of srsran_sequence_pucch in bit i, i < 20
  uint32_t nof_uci_bits;
  uint32_t filter_len;        // 0 or 3
  float    filter[3];
  float    threshold_dmrs;
  uint32_t dmrs_detection;    // isnormal(threshold_dmrs_detection)
  uint32_t decode;            // 0: the estimator stage alone
};

struct Record {
  float    noise_estimate; // calibrated, FLT_MIN for zero
  float    epre;
  float    pe_sum[2];      // srsran_vec_acc_cc over all pilot estimates
  float    ta[2 * kMaxRs][2]; // per reference row: sum pe[k] conj(pe[k - 1]), k >= 1
  float    correlation;    // formats 1x: the winning candidate's; formats 2x: filled by the host from llr_pow and max_corr
  float    dmrs_correlation;
  float    llr_pow;
  int32_t  max_corr;
  uint32_t word;           // 1A: b; 1B: b << 1 | b2; formats 2x: the best word
  uint32_t drs;            // i_max of the 2A / 2B hypotheses
  uint32_t early;          // the DMRS detection returned early
  uint32_t bad;            // the job was not run: an index outside its bounds
};

struct Dbg {
  float2  ce[2][kNre];
  float2  pe[2 * kMaxRs][kNre];
  float2  z[kMaxZ];
  int16_t llr[kBits2];
};

struct Params {
  const Job*    jobs;
  const float2* cols;    // [n_cols][nsymb][12]
  Record*       rec;     // [n_jobs]
  Dbg*          dbg;     // [n_jobs] or nullptr
  uint32_t      n_jobs, n_cols;
  uint32_t      basis[kWordBits]; // bit i of basis[n]: basis[n][i]
  float         qpsk_s;           // (float)(-100 * M_SQRT2), as the host compiler evaluates it
};

hipError_t launch(const Params& p, hipStream_t stream);

} // namespace pucch
} // namespace phyhip
