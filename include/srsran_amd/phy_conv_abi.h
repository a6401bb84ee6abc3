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
 * NOT taken: srsran_viterbi_init_sse / _avx2 / _neon (the 8-bit decoders); PCFICH and PHICH (the CFI of a PDCCH search is the caller's, which is why there
 * is no _est form of it yet -- the REG map restated for the search already knows their REGs); the transmit side (srsran_pdcch_encode,
 * srsran_regs_pdcch_put); more than 2 receive antennas; the 0 / 1A format differentiation and the RNTI match (they need dci_cfg: the caller's); the NR
 * polar PDCCH.
 */
#ifndef SRSRAN_AMD_PHY_CONV_ABI_H
#define SRSRAN_AMD_PHY_CONV_ABI_H

#include "srsran_amd/phy_abi.h"
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

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PHY_CONV_ABI_H */
