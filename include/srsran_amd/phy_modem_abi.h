/* phy_modem_abi.h -- soft demodulation and descrambling: the step between SC-FDMA de-precoding / equalisation and rate
 * de-matching.
 *
 * Reference interfaces replaced (same names, arguments, return values and arithmetic, bit for bit on an x86 build):
 *   lib/include/srsran/phy/modem/demod_soft.h:38-42    srsran_demod_soft_demodulate{,_s,_b}
 *   lib/include/srsran/phy/common/sequence.h:66-70     srsran_sequence_apply_{f,s,c}
 *   lib/include/srsran/phy/common/sequence.h:93-160    srsran_sequence_{pdsch,pusch}_apply_{f,s,c}
 * Callers in the reference: pusch.c:419-443, pdsch.c:693-744 (demodulate, then descramble in place).
 *
 * The host-pointer functions copy in, run one kernel, copy out and synchronise.  The throughput path is the batched
 * call at the end: any number of (modulation, length, seed) jobs over device-resident symbols in ONE fused pass that
 * writes the descrambled soft bits once.
 */
#ifndef SRSRAN_AMD_PHY_MODEM_ABI_H
#define SRSRAN_AMD_PHY_MODEM_ABI_H

#include "srsran_amd/phy_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* phy_common.h:285-292 */
typedef enum {
  SRSRAN_MOD_BPSK = 0,
  SRSRAN_MOD_QPSK,
  SRSRAN_MOD_16QAM,
  SRSRAN_MOD_64QAM,
  SRSRAN_MOD_256QAM,
  SRSRAN_MOD_NITEMS
} srsran_mod_t;

/* demod_soft.h:38-42.  Return 0, or -1 for an invalid modulation (demod_soft.c:846-919). */
SRSRAN_API int srsran_demod_soft_demodulate(srsran_mod_t modulation, const cf_t* symbols, float* llr, int nsymbols);
SRSRAN_API int srsran_demod_soft_demodulate_s(srsran_mod_t modulation, const cf_t* symbols, short* llr, int nsymbols);
SRSRAN_API int srsran_demod_soft_demodulate_b(srsran_mod_t modulation, const cf_t* symbols, int8_t* llr, int nsymbols);

/* sequence.h:66-70: out[i] = in[i] * (1 - 2 c(i)), c = Gold sequence of TS 36.211 7.2 with c_init = seed */
SRSRAN_API void srsran_sequence_apply_f(const float* in, float* out, uint32_t length, uint32_t seed);
SRSRAN_API void srsran_sequence_apply_s(const int16_t* in, int16_t* out, uint32_t length, uint32_t seed);
SRSRAN_API void srsran_sequence_apply_c(const int8_t* in, int8_t* out, uint32_t length, uint32_t seed);

/* sequence.h:93-160 (phch/sequences.c:63-152) */
SRSRAN_API void srsran_sequence_pdsch_apply_f(const float* in, float* out, uint16_t rnti, int q, uint32_t nslot, uint32_t cell_id, uint32_t len);
SRSRAN_API void srsran_sequence_pdsch_apply_s(const int16_t* in, int16_t* out, uint16_t rnti, int q, uint32_t nslot, uint32_t cell_id, uint32_t len);
SRSRAN_API void srsran_sequence_pdsch_apply_c(const int8_t* in, int8_t* out, uint16_t rnti, int q, uint32_t nslot, uint32_t cell_id, uint32_t len);
SRSRAN_API void srsran_sequence_pusch_apply_s(const int16_t* in, int16_t* out, uint16_t rnti, uint32_t nslot, uint32_t cell_id, uint32_t len);
SRSRAN_API void srsran_sequence_pusch_apply_c(const int8_t* in, int8_t* out, uint16_t rnti, uint32_t nslot, uint32_t cell_id, uint32_t len);

/* ---- batched, device resident ---- */
#define SRSRAN_HIP_LLR_SHORT 0
#define SRSRAN_HIP_LLR_BYTE 1
#define SRSRAN_HIP_LLR_FLOAT 2
#define SRSRAN_HIP_MOD_NONE 5 /* job.mod: the input already holds soft bits of the output type (descrambling only) */
#define SRSRAN_HIP_SEQUENCE_MAX_LEN (1u << 21)

typedef struct {
  uint32_t mod;           /* srsran_mod_t, or SRSRAN_HIP_MOD_NONE */
  uint32_t nof_symbols;   /* symbols (soft bits with SRSRAN_HIP_MOD_NONE) */
  uint32_t symbol_offset; /* first symbol in d_symbols (cf_t units; soft bits with SRSRAN_HIP_MOD_NONE) */
  uint32_t llr_offset;    /* first soft bit in d_llr; multiples of 16 bytes take the fast store path */
  uint32_t seed;          /* c_init of the scrambling sequence */
  uint32_t descramble;    /* bit 0: descramble with `seed`; bit 1: change the sign of every soft bit first (the NR chain,
                           * pdsch_nr.c:467 srsran_vec_neg_bb); 0: demodulate only */
} srsran_hip_demod_job_t;

typedef struct srsran_hip_demod srsran_hip_demod_t;

SRSRAN_API int  srsran_hip_demod_create(srsran_hip_demod_t** h);
SRSRAN_API void srsran_hip_demod_free(srsran_hip_demod_t* h);
/* d_in: cf_t symbols (soft bits of llr_type for SRSRAN_HIP_MOD_NONE jobs); d_llr: soft bits of llr_type.  Asynchronous on
 * `stream`; the job list is copied before the call returns. */
SRSRAN_API int srsran_hip_demod_run(srsran_hip_demod_t* h, const void* d_in, void* d_llr, int llr_type,
                                    const srsran_hip_demod_job_t* jobs, uint32_t n_jobs, void* stream);
/* sequences.c:63-66 / 116-119 */
SRSRAN_API uint32_t srsran_hip_sequence_pdsch_seed(uint16_t rnti, int q, uint32_t nslot, uint32_t cell_id);
SRSRAN_API uint32_t srsran_hip_sequence_pusch_seed(uint16_t rnti, uint32_t nslot, uint32_t cell_id);

/* ---- single-antenna ZF / MMSE equaliser: lib/include/srsran/phy/mimo/precoding.h:70-71 (precoding.c:357-392), the step before
 * transform de-precoding in pusch.c:413.  x = y conj(h) / ((|h|^2 + noise_estimate) scaling); csi (optional) = |h|^2 + noise.
 * Returns nof_symbols.  Float arithmetic: equals the reference to 1e-6 relative (3e-4 with csi, where the reference's SIMD body
 * uses an approximate reciprocal). */
SRSRAN_API int srsran_predecoding_single(cf_t* y, cf_t* h, cf_t* x, float* csi, int nof_symbols, float scaling, float noise_estimate);
/* device buffers, 16-byte aligned (d_csi 8-byte); asynchronous on `stream` */
SRSRAN_API int srsran_hip_predecoding_single(const cf_t* d_y, const cf_t* d_h, cf_t* d_x, float* d_csi, uint32_t nof_symbols, float scaling,
                                             float noise_estimate, void* stream);

/* ---- transmit diversity (SFBC, TS 36.211 6.3.3.3 / 6.3.4.3) on 2 and 4 ports: lib/include/srsran/phy/mimo/precoding.h, layermap.h
 * (precoding.c:673-802 receive, :1943-1992 transmit; layermap.c:38-47, 138-147).  HOST buffers; only planes [0, nof_rxant) / [0, nof_ports) / [0, nof_layers)
 * of the pointer arrays are read. */
#define SRSRAN_MAX_PORTS 4
#define SRSRAN_MAX_LAYERS 4
#define SRSRAN_MAX_CODEWORDS 2
/* Receive: y[rx][nof_symbols], h[port][rx][nof_symbols] -> x[layer][nof_symbols / nof_ports]; nof_rxant 1 or 2.  The formulas are those of the reference's
 * _csi variant (srsran_predecoding_diversity_csi, the one srsran_pdsch_decode runs: a UE object always has q->csi) whether or not csi is given; csi[0]
 * (nof_symbols floats) is written when csi and csi[0] are non-NULL.  On 2 ports the reference's variants without csi are the same formula; on 4 ports its
 * generic body without csi reads OTHER channel samples (precoding.c:473-476: ports 0 / 2 at 4i and ports 1 / 3 at 4i + 2 for all four layers, against
 * :723-743) and is not reproduced here (the PDCCH search runs it: srsran_hip_pdcch_extract_llr, phy_conv_abi.h).  2 ports: a pair whose channel gain is 0 divides by 1e-4 (:699-701).  Float arithmetic, every operation rounded once
 * in a fixed order: equals the reference to a few ulp of the sum of products.  nof_symbols must be even (2 ports) or a multiple of 4 (4 ports: the
 * reference leaves the last two symbols of any other grant unwritten, :715; here it is refused with -1).  Returns nof_symbols / nof_ports, or -1. */
SRSRAN_API int srsran_predecoding_diversity_multi(cf_t* y[SRSRAN_MAX_PORTS], cf_t* h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS], cf_t* x[SRSRAN_MAX_LAYERS],
                                                  float* csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_symbols, float scaling);
/* Transmit: x[layer][nof_symbols] -> y[port][nof_ports * nof_symbols], zeros on the idle ports of a 4-port pair; one float product per component by
 * the reference's own factor ((float)(scaling * M_SQRT1_2) on 2 ports, the float scaling / M_SQRT2 on 4).  Returns nof_ports * nof_symbols, or -1. */
SRSRAN_API int srsran_precoding_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* y[SRSRAN_MAX_PORTS], int nof_ports, int nof_symbols, float scaling);
/* x[j][i] = d[nof_layers i + j], i < nof_symbols / nof_layers; returns nof_symbols / nof_layers */
SRSRAN_API int srsran_layermap_diversity(cf_t* d, cf_t* x[SRSRAN_MAX_LAYERS], int nof_layers, int nof_symbols);
/* d[nof_layers i + j] = x[j][i], i < nof_layer_symbols; returns nof_layers * nof_layer_symbols */
SRSRAN_API int srsran_layerdemap_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* d, int nof_layers, int nof_layer_symbols);
/* the same four on device buffers (every plane 16-byte aligned, d_csi 8-byte), asynchronous on `stream`; they return SRSRAN_SUCCESS or an error code */
SRSRAN_API int srsran_hip_predecoding_diversity_multi(const cf_t* const d_y[SRSRAN_MAX_PORTS], const cf_t* const d_h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS],
                                                      cf_t* const d_x[SRSRAN_MAX_LAYERS], float* d_csi, uint32_t nof_rxant, uint32_t nof_ports,
                                                      uint32_t nof_symbols, float scaling, void* stream);
SRSRAN_API int srsran_hip_precoding_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* const d_y[SRSRAN_MAX_PORTS], uint32_t nof_ports,
                                              uint32_t nof_symbols, float scaling, void* stream);
SRSRAN_API int srsran_hip_layermap_diversity(const cf_t* d_d, cf_t* const d_x[SRSRAN_MAX_LAYERS], uint32_t nof_layers, uint32_t nof_symbols, void* stream);
SRSRAN_API int srsran_hip_layerdemap_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* d_d, uint32_t nof_layers, uint32_t nof_layer_symbols,
                                               void* stream);

/* ---- spatial multiplexing and large-delay CDD on 2 ports with 2 receive antennas (TM3 / TM4; TS 36.211 6.3.4.2): the bodies srsran_predecoding_type and
 * srsran_precoding_type dispatch to for SRSRAN_TXSCHEME_CDD and SRSRAN_TXSCHEME_SPATIALMUX (precoding.c:841-1858 receive, :2044-2211 transmit; utils/mat.c:63-109).
 * The reference exports no name per scheme for them, and its _type dispatchers also take the schemes the entry points above have, so no reference name is
 * claimed: the arguments are those of the _type functions plus the decoder, which the reference keeps in a process-wide variable
 * (srsran_predecoding_set_mimo_decoder).  tx_scheme and decoder carry the values of srsran_tx_scheme_t / srsran_mimo_decoder_t (phy_common.h:273-280).
 * Taken, all with nof_ports == 2 and nof_rxant == 2:
 *   SRSRAN_HIP_TXSCHEME_CDD          2 layers; the precoder alternates with the parity of the RE index; nof_symbols even (the reference's loop runs past the end
 *                                    of an odd count)
 *   SRSRAN_HIP_TXSCHEME_SPATIALMUX   2 layers, codebook_idx 0 .. 2 (pmi + 1, pdsch.c:867); 1 layer, codebook_idx 0 .. 3 (maximum-ratio combining over both
 *                                    receive antennas); any nof_symbols
 * Receive: y[rx][nof_symbols], h[port][rx][nof_symbols] -> x[layer][nof_symbols].  The formulas and their operation order are those of the reference's scalar loop
 * bodies of the _csi variants (what srsran_pdsch_decode runs), whether or not csi is given; every float operation is rounded once, nothing contracts; the
 * reference's vector bodies use a reciprocal estimate and differ from this by up to 1.5 x 2^-12 relative.  A singular channel gets no replacement value: what
 * the formula gives (inf / NaN) comes out.  SRSRAN_HIP_MIMO_DECODER_MMSE with noise_estimate 0 is the reference's default (pdsch.c:819 zeroes the noise for ZF
 * and leaves the process-wide decoder at MMSE).  csi (when csi and csi[0] are non-NULL), nof_symbols floats per row, as the reference's scalar bodies write it:
 * ZF 1.0 -- for CDD in csi[0] and csi[1], for spatial multiplexing in csi[0] ONLY, csi[1] is left untouched (:1330-1331); MMSE 1 / Re(B00) in csi[0] and
 * 1 / Re(B11) in csi[1] (when non-NULL), B = norm (H^H H + noise I)^-1; one layer |h|^2 / norm * (float)M_SQRT1_2 in csi[0].
 * Transmit: x[layer][nof_symbols] -> y[port][nof_symbols]; every output component is one float sum or difference times the reference's float factor
 * (scaling / 2, or (float)(scaling * M_SQRT1_2) for one layer and codebook 0); a multiplication by +-j is a swap and a sign.
 * HOST buffers of any alignment (the reference's vector bodies fault on planes that are not 32-byte aligned).  Return SRSRAN_SUCCESS, SRSRAN_ERROR_INVALID_INPUTS
 * (with one line on stderr, nothing written) for anything else than the above -- 4 ports, nof_rxant != 2, other layer counts, a codebook_idx out of range, an odd
 * nof_symbols with CDD, a decoder that is neither, scaling 0 or not finite, a negative or non-finite noise_estimate, a NULL plane -- or SRSRAN_ERROR. */
#define SRSRAN_HIP_TXSCHEME_SPATIALMUX 2
#define SRSRAN_HIP_TXSCHEME_CDD 3
#define SRSRAN_HIP_MIMO_DECODER_ZF 0
#define SRSRAN_HIP_MIMO_DECODER_MMSE 1
SRSRAN_API int srsran_hip_predecoding_mimo(cf_t* y[SRSRAN_MAX_PORTS], cf_t* h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS], cf_t* x[SRSRAN_MAX_LAYERS],
                                           float* csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_layers, int codebook_idx, int nof_symbols,
                                           int tx_scheme, float scaling, float noise_estimate, int decoder);
SRSRAN_API int srsran_hip_precoding_mimo(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* y[SRSRAN_MAX_PORTS], int nof_layers, int nof_ports, int codebook_idx, int nof_symbols,
                                         float scaling, int tx_scheme);
/* the same two on device buffers (planes 4-byte aligned), asynchronous on `stream` */
SRSRAN_API int srsran_hip_predecoding_mimo_dev(const cf_t* const d_y[SRSRAN_MAX_PORTS], const cf_t* const d_h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS],
                                               cf_t* const d_x[SRSRAN_MAX_LAYERS], float* const d_csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_layers,
                                               int codebook_idx, int nof_symbols, int tx_scheme, float scaling, float noise_estimate, int decoder, void* stream);
SRSRAN_API int srsran_hip_precoding_mimo_dev(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* const d_y[SRSRAN_MAX_PORTS], int nof_layers, int nof_ports,
                                             int codebook_idx, int nof_symbols, float scaling, int tx_scheme, void* stream);

#ifdef __cplusplus
}
#endif
#endif
