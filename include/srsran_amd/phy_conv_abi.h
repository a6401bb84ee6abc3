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
 * NOT taken: srsran_viterbi_init_sse / _avx2 / _neon (the 8-bit decoders), srsran_pdcch_extract_llr (REG de-mapping and the diversity front end), the
 * 0 / 1A format differentiation and the RNTI match (they need dci_cfg: the caller's), the NR polar PDCCH.
 */
#ifndef SRSRAN_AMD_PHY_CONV_ABI_H
#define SRSRAN_AMD_PHY_CONV_ABI_H

#include "srsran_amd/phy_abi.h"

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

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PHY_CONV_ABI_H */
