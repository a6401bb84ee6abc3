/*
 * phy_conv_abi.h -- the LTE convolutional code on the device: the reference's 16-bit 64-state Viterbi decoder behind its own handle API, and the PDCCH
 * blind search's decodes in one device call.
 *
 * Reference (paths relative to the reference tree):
 *   lib/include/srsran/phy/fec/convolutional/viterbi.h:37-75   srsran_viterbi_t and the srsran_viterbi_* calls
 *   lib/src/phy/fec/convolutional/viterbi.c:129-157, 474-617   decode37_avx2_16bit, the front ends (what srsran_viterbi_init selects on an AVX2 host)
 *   lib/src/phy/fec/convolutional/viterbi37_avx2_16bit.c       the arithmetic that is reproduced bit for bit
 *   lib/src/phy/phch/pdcch.c:335-419                           srsran_pdcch_dci_decode, srsran_pdcch_decode_msg (the mean rule)
 *   lib/src/phy/ue/ue_dl.c:416-470                             dci_blind_search: one srsran_pdcch_decode_msg per location and format
 *
 * What the decoder does is what the reference's does, quirks included (tests/conv_model.py restates them, tests/golden/conv_ref.npz records them): start
 * metrics all 0, 16-bit wrap arithmetic without normalisation, with tail biting 3 L steps over the frame laid out three times and the middle L bits of a
 * chain-back that starts from state 0 at the last step (the six zeroed decision words past the end make the best state moot), without tail biting L + 6
 * steps and a chain-back from state 0.
 *
 *   lib/src/phy/phch/regs.c:66-146, 249-373, 492-523, 590-781  the REG map of the control region (srsran_regs_init_opts and what it calls)
 *   lib/src/phy/phch/pdcch.c:424-487                           srsran_pdcch_extract_llr: REG gather, equaliser, QPSK demodulator, descrambler
 *   lib/src/phy/mimo/precoding.c:182-305, 428-503              the equaliser bodies the PDCCH runs (no CSI)
 *
 *   lib/src/phy/phch/pcfich.c:118-137, 156-222; phich.c:147-171, 181-312   srsran_pcfich_decode and srsran_phich_decode (ctrl_kernels.hip)
 *   lib/src/phy/ue/ue_dl.c:315-343                             estimate_pdcch_pcfich: estimator, PCFICH, PDCCH front end -- srsran_hip_pdcch_search_est
 *
 * NOT taken: srsran_viterbi_init_sse / _avx2 / _neon (the 8-bit decoders); the transmit side (srsran_pcfich_encode, srsran_phich_encode, srsran_pdcch_encode,
 * srsran_regs_*_put); srsran_phich_calc (the resource of a grant: the caller's); more than 2 receive antennas; the 0 / 1A format differentiation and the RNTI
 * match (they need dci_cfg: the caller's); the NR polar PDCCH.
 */
#ifndef SRSRAN_AMD_PHY_CONV_ABI_H
#define SRSRAN_AMD_PHY_CONV_ABI_H

#include "srsran_amd/phy_abi.h"
#include "srsran_amd/phy_chan_abi.h"  /* srsran_hip_chest_dl_t and its state and result (srsran_hip_pdcch_search_est) */
#include "srsran_amd/phy_modem_abi.h" /* cf_t, SRSRAN_MAX_PORTS */

#ifdef __cplusplus
extern "C" {
#endif

/* viterbi.h:37-55: 96 bytes.  The pointer fields the reference fills with its own buffers and functions stay NULL (nothing is allocated on the host);
 * ptr is non-NULL on an initialised handle. */
typedef enum { SRSRAN_VITERBI_27 = 0, SRSRAN_VITERBI_29, SRSRAN_VITERBI_37, SRSRAN_VITERBI_39 } srsran_viterbi_type_t;

typedef struct SRSRAN_API {
  void*    ptr;
  uint32_t R;
  uint32_t K;
  uint32_t framebits;
  bool     tail_biting;
  float    gain_quant;
  int16_t  gain_quant_s;
  int (*decode)(void*, uint8_t*, uint8_t*, uint32_t);
  int (*decode_s)(void*, uint16_t*, uint8_t*, uint32_t);
  int (*decode_f)(void*, float*, uint8_t*, uint32_t);
  void (*free)(void*);
  uint8_t*  tmp;
  uint16_t* tmp_s;
  uint8_t*  symbols_uc;
  uint16_t* symbols_us;
} srsran_viterbi_t;

#define SRSRAN_HIP_VITERBI_MAX_FRAMEBITS 2048 /* the decision words of a frame live in LDS */

/* Only SRSRAN_VITERBI_37 with the polynomials (0x6D, 0x4F, 0x57) of the LTE code; max_frame_length above SRSRAN_HIP_VITERBI_MAX_FRAMEBITS is refused
 * with one line on stderr.  gain_quant starts at 1000 (DEFAULT_GAIN_16).  Needs no device. */
SRSRAN_API int  srsran_viterbi_init(srsran_viterbi_t* q, srsran_viterbi_type_t type, int poly[3], uint32_t max_frame_length, bool tail_bitting);
SRSRAN_API void srsran_viterbi_set_gain_quant(srsran_viterbi_t* q, float gain_quant);
SRSRAN_API void srsran_viterbi_set_gain_quant_s(srsran_viterbi_t* q, int16_t gain_quant);
SRSRAN_API void srsran_viterbi_free(srsran_viterbi_t* q);
/* symbols: 3 frame_length values with tail biting, 3 (frame_length + 6) without, HOST memory; data: frame_length bits, one per byte.  Return
 * q->framebits on success (as the reference does), -1 when frame_length > q->framebits, SRSRAN_ERROR on a device-side failure.
 * _f: max = 1e-9 raised by every fabs, (int32)(32767.5f + gain_quant / max * x) as one fused multiply-add, clamped to 0 .. 65535 -- on the device;
 * _s: (int32)(32767.f + (float)x) clamped; _us: straight in; _uc: SRSRAN_ERROR (the reference's 16-bit object has no 8-bit function). */
SRSRAN_API int srsran_viterbi_decode_f(srsran_viterbi_t* q, float* symbols, uint8_t* data, uint32_t frame_length);
SRSRAN_API int srsran_viterbi_decode_s(srsran_viterbi_t* q, int16_t* symbols, uint8_t* data, uint32_t frame_length);
SRSRAN_API int srsran_viterbi_decode_us(srsran_viterbi_t* q, uint16_t* symbols, uint8_t* data, uint32_t frame_length);
SRSRAN_API int srsran_viterbi_decode_uc(srsran_viterbi_t* q, uint8_t* symbols, uint8_t* data, uint32_t frame_length);

/* n frames of uint16 symbols in one launch and one host wait (one wave per frame); q says tail biting and the longest frame.  n == 0 is a no-op;
 * n > 256, NULL pointers and a frame_length of 0 or above q->framebits are refused (SRSRAN_ERROR_INVALID_INPUTS, one line on stderr) before the device
 * is looked for.  Returns q->framebits on success. */
SRSRAN_API int srsran_hip_viterbi_decode_us_multi(srsran_viterbi_t* q, uint32_t n, const uint16_t* const* symbols, uint8_t* const* data,
                                                  const uint32_t* frame_length);

/* ---- the PDCCH blind search's decodes */
#define SRSRAN_HIP_DCI_MAX_BITS 128       /* SRSRAN_DCI_MAX_BITS */
#define SRSRAN_HIP_PDCCH_MAX_CANDIDATES 256

typedef struct SRSRAN_API {
  uint32_t ncce;     /* first CCE of the location */
  uint32_t L;        /* aggregation level 0 .. 3: 72 << L soft bits */
  uint32_t nof_bits; /* size of the DCI format tried, 1 .. 128 */
} srsran_hip_pdcch_cand_t;

typedef struct SRSRAN_API {
  uint8_t  payload[SRSRAN_HIP_DCI_MAX_BITS + 16]; /* nof_bits + 16 decoded bits, one per byte, the CRC bits included; the rest 0 */
  uint16_t crc_rem;                               /* the 16 bits after the payload, packed MSB first, xor the CRC of the payload: the RNTI of a hit */
  uint16_t decoded;                               /* 0: mean <= 0.3, the candidate was not decoded: payload and crc_rem are 0 */
  float    mean;                                  /* mean |soft bit| over the candidate (a double sum in index order, as pdcch.c:388-392) */
} srsran_hip_pdcch_res_t;

/* llr: the control region's descrambled soft bits (q->llr after srsran_pdcch_extract_llr), nof_llr = 72 NOF_CCE floats, HOST memory.  Per candidate
 * what srsran_pdcch_decode_msg does between the location check and the format differentiation: the mean rule on the host, then on the device, one wave per
 * candidate and all candidates in one launch, srsran_rm_conv_rx, srsran_viterbi_decode_f's quantiser, the decoder over nof_bits + 16 bits and the CRC.
 * One upload, one launch, one download, one host wait.  n == 0 is a no-op (0).  Refused with SRSRAN_ERROR_INVALID_INPUTS before the device is looked for, one
 * line on stderr, n results zeroed (when res and n allow): NULL pointers, n > 256, L > 3, ncce 72 + (72 << L) > nof_llr, nof_bits 0 or above 128.
 * A device-side failure returns SRSRAN_ERROR (there is no CPU fallback). */
SRSRAN_API int srsran_hip_pdcch_dci_decode_multi(const float* llr, uint32_t nof_llr, uint32_t n, const srsran_hip_pdcch_cand_t* cand,
                                                 srsran_hip_pdcch_res_t* res);
/* the same; rm_f and symbols (either may be NULL) receive per candidate 432-value rows: the 3 (nof_bits + 16) de-matched floats and quantised symbols
 * in front, the rest (and the rows of candidates that were not decoded) 0 */
SRSRAN_API int srsran_hip_pdcch_dci_decode_multi_dbg(const float* llr, uint32_t nof_llr, uint32_t n, const srsran_hip_pdcch_cand_t* cand,
                                                     srsran_hip_pdcch_res_t* res, float* rm_f, uint16_t* symbols);

/* ---- the PDCCH search of a subframe from the received grids: REG de-mapping, equaliser, demodulator, descrambler, the mean rule and the decodes on the
 * device (pdcch_map.h, pdcch_kernels.hip, pdcch_host.cpp) */

/* the control region of one subframe: what srsran_regs_init_opts, srsran_pdcch_set_cell and srsran_pdcch_extract_llr read of the cell and of
 * srsran_dl_sf_cfg_t.  44 bytes, no padding.  A description outside these ranges is refused. */
typedef struct SRSRAN_API {
  uint32_t cell_nof_prb;       /* 6 .. 110 */
  uint32_t cell_nof_ports;     /* 1, 2 or 4 */
  uint32_t cell_id;            /* 0 .. 503 */
  uint32_t cp_nsymb;           /* 7 (normal cyclic prefix) or 6 (extended) */
  uint32_t phich_length;       /* 0 normal, 1 extended */
  uint32_t phich_resources;    /* 0 .. 3: Ng = 1/6, 1/2, 1, 2 */
  uint32_t phich_mi;           /* 0 .. 3; 0: the subframe has no PHICH */
  uint32_t mbsfn_or_sf1_6_tdd; /* 0 or 1 (regs.c:331-341) */
  uint32_t cfi;                /* 1 .. 3; the region spans cfi symbols, cfi + 1 when cell_nof_prb <= 10 */
  uint32_t sf_idx;             /* 0 .. 9: the scrambling sequence's c_init = sf_idx 512 + cell_id */
  uint32_t nof_rx;             /* 1 or 2 receive antennas */
} srsran_hip_pdcch_sf_t;

/* Host only (no device is looked for).  What srsran_regs_pdcch_nregs returns for the description -- a multiple of 9 -- or -1 for a NULL or out-of-range one. */
SRSRAN_API int srsran_hip_regs_pdcch_nregs(const srsran_hip_pdcch_sf_t* sf);
/* Host only.  re_idx: the 4 nregs grid indices k + l 12 cell_nof_prb of the region's REs, in the order srsran_regs_pdcch_get reads them.  Returns nregs
 * or -1. */
SRSRAN_API int srsran_hip_regs_pdcch_table(const srsran_hip_pdcch_sf_t* sf, uint32_t* re_idx);
/* srsran_regs_pdcch_get on n_planes (1 .. 10) grids at once, HOST memory, one launch: d[p][i] = grids[p][re_idx[i]].  Each grid holds at least the
 * region's symbols (rows of 12 cell_nof_prb points), each d 4 nregs points.  Returns 4 nregs, -1 for what is refused (one line on stderr) or failed. */
SRSRAN_API int srsran_hip_regs_pdcch_get(const srsran_hip_pdcch_sf_t* sf, uint32_t n_planes, const cf_t* const* grids, cf_t* const* d);
/* srsran_pdcch_extract_llr.  sf_symbols[rx]: the received grids, ce[port][rx]: the estimate grids (HOST memory; only the region's symbols are read),
 * noise_estimate: channel->noise_estimate (halved here, as pdcch.c:471 does; one port only); llr: 72 NOF_CCE floats.  One fused kernel: the REs are read
 * through the REG table, equalised (one port: sum y conj(h) / (sum |h|^2 + noise), noise added when above 0; two ports: the SFBC combiner with the
 * hh == 0 -> 1e-4 rule; four ports: the reference's body WITHOUT CSI, precoding.c:465-498), layer de-mapped by where they are stored, demodulated
 * (x -sqrt 2) and descrambled.  Returns 72 NOF_CCE, SRSRAN_ERROR_INVALID_INPUTS for what is refused, SRSRAN_ERROR on a device-side failure. */
SRSRAN_API int srsran_hip_pdcch_extract_llr(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                            float* llr);
/* The whole search of a subframe: srsran_hip_pdcch_extract_llr chained into the decodes of srsran_hip_pdcch_dci_decode_multi without a host wait between
 * them; the mean rule runs on the device (a double sum in index order: mean and decoded come out as the host's).  One upload (the region's rows of the
 * planes and the candidates; the REG table is resident), two launches, one download, one host wait.  n == 0 returns 0 and touches nothing.  Refused with
 * SRSRAN_ERROR_INVALID_INPUTS before the device is looked for, one line on stderr, n results zeroed (when res and n allow): NULL pointers (a needed plane
 * included), a description out of range, n > 256, L > 3, nof_bits 0 or above 128, ncce 72 + (72 << L) > 72 NOF_CCE of this cfi.  A device-side failure
 * returns SRSRAN_ERROR (there is no CPU fallback). */
SRSRAN_API int srsran_hip_pdcch_search_sf(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                          uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res);
/* the same; each output may be NULL.  llr_out: the 72 NOF_CCE soft bits; d_out: the 36 NOF_CCE equalised symbols; sym_out[rx] / ce_out[port][rx] (the arrays
 * or any entry may be NULL): the extracted planes, 36 NOF_CCE points each; rm_f / symbols: as srsran_hip_pdcch_dci_decode_multi_dbg */
SRSRAN_API int srsran_hip_pdcch_search_sf_dbg(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                              float noise_estimate, uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, float* llr_out,
                                              cf_t* d_out, cf_t* const* sym_out, cf_t* const (*ce_out)[SRSRAN_MAX_PORTS], float* rm_f, uint16_t* symbols);

/* ---- PCFICH and PHICH on the device (pdcch_map.h, ctrl_kernels.hip, ctrl_host.cpp): the CFI of a subframe and its HARQ indications from the received
 * grids and the estimates.  sf->cfi is not read by any of these calls, but the description goes through the same validation as everywhere: it must hold
 * 1 .. 3. */

/* Host only (no device is looked for).  re_idx: the 16 grid indices srsran_regs_pcfich_get reads (all on symbol 0), in its order: four REGs at
 * k = (6 (cell_id % (2 nof_prb)) + 6 (i nof_prb / 2)) % (12 nof_prb), found by their first sub-carrier.  Returns 16, or -1 for what the PDCCH table refuses. */
SRSRAN_API int srsran_hip_regs_pcfich_table(const srsran_hip_pdcch_sf_t* sf, uint32_t re_idx[16]);
/* Host only.  srsran_regs_phich_ngroups: phich_mi ceilf(Ng (nof_prb / 8)), twice that with the extended cyclic prefix, 0 when phich_mi == 0; -1 as above. */
SRSRAN_API int srsran_hip_regs_phich_ngroups(const srsran_hip_pdcch_sf_t* sf);
/* Host only.  re_idx: the 12 grid indices k + l 12 nof_prb srsran_regs_phich_get reads for the group (mapping unit ngroup / 2 with the extended prefix), on
 * symbols 0 .. 2.  Returns 12, or -1 (ngroup >= ngroups included). */
SRSRAN_API int srsran_hip_regs_phich_table(const srsran_hip_pdcch_sf_t* sf, uint32_t ngroup, uint32_t re_idx[12]);

/* srsran_pcfich_decode (pcfich.c:118-137, 156-222).  sf_symbols[rx], ce[port][rx]: HOST memory, only symbol 0 is read; noise_estimate:
 * channel->noise_estimate, NOT halved (unlike the PDCCH), one port only, added to the gain when above 0 (the body the reference runs on 16 symbols,
 * srsran_predecoding_single_gen, adds it as it is: the same for every estimate that is not negative).  One launch of one wave: the 16 REs through the table,
 * the PDCCH's three equalisers (four ports WITHOUT CSI), layer de-mapping by where the result is stored, the QPSK float demodulator, the descrambler with
 * c_init = (sf_idx + 1)(2 cell_id + 1) 512 + cell_id, and three correlations against 2 b - 1 of Table 5.3.4-1, each summed in index order from 0
 * (srsran_vec_dot_prod_fff is a plain loop, and the reference's flags do not let the compiler reorder it).  The decision is the reference's: max_corr starts at
 * 0 and the comparison is strict, so when no correlation is positive *cfi = 1 and *corr = 0.  corr may be NULL.  One upload, one launch, one download, one host
 * wait.  Returns 1 as the reference does; SRSRAN_ERROR_INVALID_INPUTS with one line on stderr and *cfi, *corr zeroed, before the device is looked for, for NULL
 * pointers (a needed plane included) and a description the map refuses; SRSRAN_ERROR on a device-side failure (there is no CPU fallback). */
SRSRAN_API int srsran_hip_pcfich_decode(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                        uint32_t* cfi, float* corr);
/* the same; each output may be NULL.  data_f: the 32 descrambled soft bits (q->data_f); d: the 16 equalised symbols (q->d); corr3: the three correlations */
SRSRAN_API int srsran_hip_pcfich_decode_dbg(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                            uint32_t* cfi, float* corr, float data_f[32], cf_t d[16], float corr3[3]);

#define SRSRAN_HIP_PHICH_MAX_RESOURCES 16

typedef struct SRSRAN_API {
  uint32_t ngroup; /* below srsran_hip_regs_phich_ngroups */
  uint32_t nseq;   /* below 8 (normal cyclic prefix) or 4 (extended) */
} srsran_hip_phich_resource_t;

typedef struct SRSRAN_API {
  uint32_t ack_value; /* srsran_phich_ack_decode: 1 when the mean of the three soft bits is above that of their negatives */
  float    distance;  /* that mean: max_corr starts at -9999 and the comparison is strict */
  float    bits[3];   /* q->data_rx: -(re + im) of z in float, times M_SQRT1_2 in double, rounded once */
  cf_t     z[3];      /* q->z: the de-spread symbols */
} srsran_hip_phich_res_t; /* 44 bytes */

/* srsran_phich_decode (phich.c:147-171, 181-312) of n resources of one subframe in one launch, one wave per resource: the group's 12 REs per plane, the
 * equalisers and the noise rule of srsran_hip_pcfich_decode, with the extended prefix d0[4 i + 2 (ngroup % 2) + {0, 1}], the descrambler of the PCFICH's c_init
 * (12 chips), the de-spreading sum of conj(w[nseq][j]) d[NSF i + j] / NSF in j order from 0 (NSF 4, or 2 with the extended prefix), the BPSK float demodulator and
 * the decision.  Only the symbols the PHICH reaches (at most 0 .. 2) are read.  n == 0 is a no-op (0).  One upload, one launch, one download, one host wait.
 * Returns SRSRAN_SUCCESS; SRSRAN_ERROR_INVALID_INPUTS with one line on stderr and the n results zeroed (when res and n allow), before the device is looked
 * for, for NULL pointers (a needed plane included), a description the map refuses, n > 16, ngroup >= ngroups, nseq >= 8 (4 with the extended prefix);
 * SRSRAN_ERROR on a device-side failure. */
SRSRAN_API int srsran_hip_phich_decode_multi(const srsran_hip_pdcch_sf_t* sf, cf_t* const sf_symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS], float noise_estimate,
                                             uint32_t n, const srsran_hip_phich_resource_t* r, srsran_hip_phich_res_t* res);

/* ---- the control side of a subframe from the received grids alone: what estimate_pdcch_pcfich (ue_dl.c:315-343) chains -- srsran_chest_dl_estimate_cfg,
 * srsran_pcfich_decode, srsran_pdcch_extract_llr -- with the candidate decodes and srsran_phich_decode behind it, in one device call */
typedef struct SRSRAN_API {
  uint32_t n_cand[3]; /* the lengths of the three candidate lists: n_cand[c - 1] candidates for CFI c, each 0 .. 256 */
  uint32_t cfi3_to_2; /* 1: the TDD subframe 1 / 6 rule of ue_dl.c:331, a decoded CFI of 3 becomes 2 before the PDCCH; 0 or 1 */
  uint32_t n_phich;   /* PHICH resources, 0 .. 16 */
} srsran_hip_pdcch_est_t;

/* sf: the description (cfi is not read, but must hold 1 .. 3); est, state_in: the estimator's, as srsran_hip_chest_dl_estimate takes them (phy_chan_abi.h);
 * sf_symbols[rx]: the whole received grids, HOST memory; cand: the three lists one behind the other -- the list of CFI c holds the candidates valid for that
 * CFI's NOF_CCE, since the caller cannot know the CFI yet; res: max(n_cand) rows, of which the first n_cand[cfi - 1] are filled and the rest stay zero; phich /
 * phich_res: opt->n_phich resources and results (may be NULL when it is 0); *cfi: the decoded CFI after the cfi3_to_2 rule; *cfi_corr: its correlation (may be
 * NULL); est_out: what srsran_hip_chest_dl_estimate returns.
 * On the device, in stream order and without a host wait between them: chest_dl_kernel (the ce grids go to device scratch, the pairs' noise estimates to device
 * memory), ctrl_kernel (PCFICH and PHICH with the noise estimate fill_res reports, averaged on the device; it leaves the CFI as one word of device memory),
 * pdcch_front_kernel launched for the region of CFI 3 (it reads that word, takes the table and the size of that CFI's region -- all three tables are resident --
 * and one port takes half the noise estimate) and pdcch_dci_sf_kernel launched for max(n_cand) waves (it takes that CFI's list; waves past its length leave).
 * One upload (the whole grids -- the estimator reads every CRS symbol -- the pilot rows, the estimator's jobs, the three lists and the PHICH resources), four
 * launches, one download (the estimator's records, the CFI and its correlation, the PHICH results, the result rows), one host wait.
 * Refused with SRSRAN_ERROR_INVALID_INPUTS before the device is looked for, one line on stderr, the results, *cfi, *cfi_corr and *est_out zeroed (when the
 * pointers and counts allow): everything srsran_hip_pdcch_search_sf, srsran_hip_chest_dl_estimate and srsran_hip_phich_decode_multi refuse, an estimator
 * description whose cell, subframe or antenna count is not sf's, nof_rx above 2, n_cand[c] > 256, a candidate past the region of its list's CFI, cfi3_to_2
 * above 1, a description on which any of the three CFIs has no table.  A device-side failure returns SRSRAN_ERROR (there is no CPU fallback). */
SRSRAN_API int srsran_hip_pdcch_search_est(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
                                           cf_t* const sf_symbols[], const srsran_hip_pdcch_est_t* opt, const srsran_hip_pdcch_cand_t* cand,
                                           srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* phich, srsran_hip_phich_res_t* phich_res, uint32_t* cfi,
                                           float* cfi_corr, srsran_hip_chest_dl_res_t* est_out);
/* the same; each output may be NULL.  llr_out: the 72 NOF_CCE soft bits of the decoded CFI (the caller sizes it for CFI 3; what lies behind is not written);
 * pcfich_data_f: the PCFICH's 32 soft bits; ce_grid_out[port][rx] (the array or an entry may be NULL): the pair's whole ce grid; rm_f / symbols: max(n_cand)
 * rows as srsran_hip_pdcch_search_sf_dbg has them, the rows past the chosen list's length zero */
SRSRAN_API int srsran_hip_pdcch_search_est_dbg(const srsran_hip_pdcch_sf_t* sf, const srsran_hip_chest_dl_t* est, const srsran_hip_chest_dl_state_t* state_in,
                                               cf_t* const sf_symbols[], const srsran_hip_pdcch_est_t* opt, const srsran_hip_pdcch_cand_t* cand,
                                               srsran_hip_pdcch_res_t* res, const srsran_hip_phich_resource_t* phich, srsran_hip_phich_res_t* phich_res,
                                               uint32_t* cfi, float* cfi_corr, srsran_hip_chest_dl_res_t* est_out, float* llr_out, float pcfich_data_f[32],
                                               cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS], float* rm_f, uint16_t* symbols);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PHY_CONV_ABI_H */
