/*
 * phy_prach_abi.h -- random-access detection of a cell in one device call (libsrsran_phy_hip.so).
 *
 * srsran_prach_detect_offset (lib/src/phy/phch/prach.c:871-914, with srsran_prach_process at :772-869) restated as written, quirks included: one upload,
 * two launches (a pruned first stage that keeps 839 of the N_ifft_prach bins, one correlator workgroup per occasion and searched root), one download and
 * one host wait.  The decisions (threshold, detection list, time offsets) are the reference's float expressions, applied on the host to what came down.
 *
 * NOT taken: successive cancellation (a host-decided loop over whole detections, and the reference itself switches it off unless zero_corr_zone == 0);
 * preamble format 4 (detect_offset computes `begin` with the long formats' K = 12 even there, :897, and would read outside the transform; the reference
 * takes the format as config_idx / 16 and refuses config_idx >= 64, so its set_cell_ never selects it, and neither do plan and create); the transmit side srsran_prach_gen; the TTI-opportunity helpers (a few host integer lines, the caller's); NR.
 */
#ifndef SRSRAN_AMD_PHY_PRACH_ABI_H
#define SRSRAN_AMD_PHY_PRACH_ABI_H

#include "srsran_amd/phy_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_HIP_PRACH_N_ZC 839
#define SRSRAN_HIP_PRACH_MAX_ROOTS 64 /* roots a cell can use, and search */
#define SRSRAN_HIP_PRACH_MAX_OCC 8    /* occasions of one srsran_hip_prach_detect_multi */
#define SRSRAN_HIP_PRACH_MAX_DET 128  /* detections an occasion of _multi reports */

/* srsran_prach_cfg_t plus the cell width; 32 bytes */
typedef struct {
  uint32_t nof_prb; /* 6, 15, 25, 50, 75, 100: N_ifft_ul = srsran_symbol_sz(nof_prb) */
  uint32_t config_idx;
  uint32_t root_seq_idx;
  uint32_t zero_corr_zone;
  uint32_t num_ra_preambles;        /* as the reference reads it (:602, :787): the number of ROOTS searched; < 4 or > N_roots selects N_roots */
  uint32_t hs_flag;                 /* restricted set */
  uint32_t freq_domain_offset_calc; /* t_offsets from the phase of the cross sum (:750-760) instead of the peak position (:742-746) */
  float    detect_factor;           /* 0 selects the reference's 18 */
} srsran_hip_prach_cfg_t;

/* what srsran_prach_set_cell_ (:528-654) and srsran_prach_gen_seqs (:359-460) leave in srsran_prach_t; 548 bytes */
typedef struct {
  uint32_t N_zc;
  uint32_t N_cs;
  uint32_t N_ifft_ul;
  uint32_t N_ifft_prach;
  uint32_t N_seq;
  uint32_t N_cp;
  uint32_t N_roots;
  uint32_t n_wins;          /* N_zc / N_cs, or 1 */
  uint32_t num_ra_preambles; /* after the clamp at :602: the number of roots searched */
  uint32_t root_seqs_idx[SRSRAN_HIP_PRACH_MAX_ROOTS]; /* first preamble of each used root */
  uint32_t root_u[SRSRAN_HIP_PRACH_MAX_ROOTS];        /* physical root of each used root */
} srsran_hip_prach_info_t;

/* one occasion of srsran_hip_prach_detect_multi; 16 bytes */
typedef struct {
  uint32_t    freq_offset;
  uint32_t    sig_len;
  const cf_t* signal;
} srsran_hip_prach_occ_t;

/* 1540 bytes */
typedef struct {
  uint32_t n_indices;
  uint32_t indices[SRSRAN_HIP_PRACH_MAX_DET];
  float    t_offsets[SRSRAN_HIP_PRACH_MAX_DET];
  float    peak_to_avg[SRSRAN_HIP_PRACH_MAX_DET];
} srsran_hip_prach_res_t;

/* the intermediates of srsran_hip_prach_detect_offset_dbg; any pointer may be NULL.  r < num_ra_preambles (the roots searched), j < n_wins. */
typedef struct {
  cf_t*     prach_bins;   /* [839] */
  float*    corr;         /* [r][839] */
  float*    corr_ave;     /* [r] */
  cf_t*     cross_sum;    /* [r]: the sum over `cross` (:792, :753) */
  float*    peak_values;  /* [r][n_wins] */
  uint32_t* peak_offsets; /* [r][n_wins]; 0 where the window's peak stayed 0 */
} srsran_hip_prach_dbg_t;

typedef struct srsran_hip_prach srsran_hip_prach_t;

/* The order of the 838 physical roots by logical index (TS 36.211 Table 5.7.2-4) is NOT part of the library: the application hands it in once per process,
 * before the first plan or create (an srsRAN build has it as `uint32_t prach_zc_roots[838]`).  It is copied; it must be a permutation of 1 .. 838
 * (SRSRAN_ERROR_INVALID_INPUTS otherwise, the table in force stays).  NULL takes the table away again. */
SRSRAN_API int srsran_hip_prach_set_root_order(const uint32_t order[838]);

/* Pure host code, needs no device.  SRSRAN_ERROR_INVALID_INPUTS (one line on stderr, *info zeroed) for what srsran_prach_set_cell_ refuses, for a cell
 * width other than the six standard ones, and while the root order has not been set. */
SRSRAN_API int srsran_hip_prach_plan(const srsran_hip_prach_cfg_t* cfg, srsran_hip_prach_info_t* info);

/* The handle keeps, on the device of the calling thread, the spectrum of each searched root: the table sequence of prach_cexp (:73-100) through the
 * forward 839-point DFT with norm (get_precoded_dft, :346-357).  It is used from one thread at a time. */
SRSRAN_API int  srsran_hip_prach_create(srsran_hip_prach_t** h, const srsran_hip_prach_cfg_t* cfg);
SRSRAN_API void srsran_hip_prach_destroy(srsran_hip_prach_t* h);
SRSRAN_API int  srsran_hip_prach_info(const srsran_hip_prach_t* h, srsran_hip_prach_info_t* info);
SRSRAN_API int  srsran_hip_prach_root_spectrum(srsran_hip_prach_t* h, uint32_t i, cf_t out[SRSRAN_HIP_PRACH_N_ZC]);

/* srsran_prach_detect_offset plus max_det, the capacity of indices / t_offsets / peak_to_avg (the last two may be NULL).  Detections come in the
 * reference's order (root by root, window by window) with its index i * n_wins + j, which may exceed 63 when the last root is only partly used.  Only the
 * first max_det are written and *n_indices is that capped count.  Only the first N_ifft_prach samples of `signal` are read. */
SRSRAN_API int srsran_hip_prach_detect_offset(srsran_hip_prach_t* h, uint32_t freq_offset, const cf_t* signal, uint32_t sig_len, uint32_t* indices,
                                              float* t_offsets, float* peak_to_avg, uint32_t max_det, uint32_t* n_indices);
SRSRAN_API int srsran_hip_prach_detect_offset_dbg(srsran_hip_prach_t* h, uint32_t freq_offset, const cf_t* signal, uint32_t sig_len, uint32_t* indices,
                                                  float* t_offsets, float* peak_to_avg, uint32_t max_det, uint32_t* n_indices,
                                                  const srsran_hip_prach_dbg_t* dbg);
/* n <= SRSRAN_HIP_PRACH_MAX_OCC occasions of one handle (the frequency-multiplexed occasions of a TDD subframe on one signal, several receive buffers)
 * with the launch count of one; res[o] equals what the single call gives for occ[o], bit for bit. */
SRSRAN_API int srsran_hip_prach_detect_multi(srsran_hip_prach_t* h, uint32_t n, const srsran_hip_prach_occ_t* occ, srsran_hip_prach_res_t* res);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PHY_PRACH_ABI_H */
