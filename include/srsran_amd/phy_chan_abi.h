/*
 * phy_chan_abi.h -- one device call per GRANT: the stages the reference runs between the resource grid and the transport block
 * stay on the device.
 *
 * Reference call sites these entry points are bound at (tests/ref_link/chan_bind.c shows the binding a maintainer adds):
 *   srsran_pusch_decode   lib/src/phy/phch/pusch.c:358-478   extract REs -> srsran_predecoding_single -> srsran_dft_precoding ->
 *                                                            srsran_demod_soft_demodulate_{s,b} -> srsran_sequence_pusch_apply_{s,c} ->
 *                                                            srsran_ulsch_decode (sch.c:1121: channel de-interleaver, decode_tb)
 *   srsran_pdsch_decode   lib/src/phy/phch/pdsch.c:788-946   (per codeword, :662-760) demodulate -> srsran_sequence_pdsch_apply_{s,c} ->
 *                                                            srsran_dlsch_decode2 (sch.c:579); single port: srsran_predecoding_single in front
 *   srsran_pdsch_encode   lib/src/phy/phch/pdsch.c:1017-1144 (per codeword, :949-1015) srsran_dlsch_encode2 -> srsran_sequence_pdsch_apply_pack ->
 *                                                            srsran_mod_modulate_bytes (-> power scaling, :1119)
 *   srsran_ulsch_encode   lib/src/phy/phch/sch.c:1194-1340   encode_tb -> [CQI / RI / ACK multiplexing] -> channel interleaver
 *   srsran_pusch_encode   lib/src/phy/phch/pusch.c:259-354   srsran_ulsch_encode -> srsran_sequence_pusch_apply_pack -> placeholder / repetition fix-up ->
 *                                                            srsran_mod_modulate_bytes -> srsran_dft_precoding -> pusch_put
 * Through the per-stage handle API a grant costs four host <-> device round trips; here it costs one: symbols and channel estimates go up
 * (the kernels read them from the pinned staging image), the payload and the verdict come down.  Soft-buffer handling (HARQ combining
 * across calls, stored code blocks) is srsran_hip_decode_tb_cb's (phy_sch_abi.h).
 *
 * A PUSCH grant that carries control information (HARQ-ACK, RI, CQI multiplexed into it by TS 36.212 5.2.2.8) is taken by srsran_hip_pusch_decode_uci:
 * the de-multiplexer is part of the demodulator's store, the few soft bits of the control fields come down with the payload, and the caller runs the
 * reference's own small decoders (uci.c) on them.  The UE's transmit side is srsran_hip_pusch_encode: the caller runs the reference's small encoders and
 * hands over the types of the ACK / RI bits and the coded CQI bits; multiplexer, scrambler, fix-up and modulator are one kernel, the transform follows.
 *
 * A PDSCH codeword of a 2- or 4-port cell sent with transmit diversity (SRSRAN_TXSCHEME_DIVERSITY: TM2, the common channels and the TM3 / TM4 fallback of such a
 * cell) is taken by srsran_hip_pdsch_decode_txdiv / srsran_hip_pdsch_encode_txdiv: SFBC combining over 1 or 2 receive antennas and layer de-mapping sit in
 * front of the demodulator in one kernel, the layer map and the SFBC precoder are the modulator's store.
 *
 * A PDSCH grant of a 2-port cell sent with large-delay CDD (TM3: two codewords) or closed-loop spatial multiplexing (TM4: a PMI, one or two codewords),
 * received on 2 antennas, is taken by srsran_hip_pdsch_decode_mimo / srsran_hip_pdsch_encode_mimo: the precoder applied to the estimates, the 2x2 ZF / MMSE solve
 * (or maximum-ratio combining), the demodulator and the descrambler of BOTH codewords are one kernel, and both transport blocks decode behind it in one pass.
 *
 * The PDSCH's resource DE-mapping (srsran_pdsch_get: the gather around reference signals, PSS / SSS and PBCH) is taken by the _sf form of each PDSCH receive
 * call, which starts at srsran_pdsch_decode's own signature: subframe grids and the channel estimator's grids in, one more launch, still one host wait.
 *
 * The PUSCH's channel estimator (srsran_chest_ul_estimate_pusch, the first of the two calls of srsran_enb_ul_get_pusch, enb_ul.c:272-281) is taken by
 * srsran_hip_chest_ul_estimate_pusch and, in front of the equaliser of the same call, by srsran_hip_pusch_decode_est{,_multi}: the grid and the grant's DMRS
 * row in, the payload and the estimator's six measurements out, one more launch, still one host wait.
 *
 * What is NOT taken here and stays with the caller: the PUCCH and SRS channel estimators, generating the DMRS rows (refsignal_ul.c), the PDSCH's resource mapping on transmit (srsran_pdsch_put: the caller's grid holds other channels' REs),
 * spatial multiplexing and CDD on 4 ports (the
 * reference refuses them too) or with other than 2 receive antennas, PMI and condition-number selection (srsran_precoding_pmi_select, srsran_precoding_cn:
 * reductions over a whole subframe's estimates), the PUSCH's CSI weighting (pusch_cfg.h: csi_enable), PMCH, a PUSCH without a transport block (tbs == 0: CQI
 * only; in both directions), 8-bit soft bits on a grant with control information, the block codes of the control information themselves (srsran_uci_encode_ack_ri,
 * srsran_uci_encode_cqi_pusch, srsran_cqi_value_pack and their decoders), EVM measurement.
 *
 * CSI weighting of the PDSCH's soft bits (cfg->csi_enable, which srsue turns on by default; csi_correction, pdsch.c:523-618, between the descrambler and
 * srsran_dlsch_decode2) is taken by the _csi form of each PDSCH receive call: the front end files the equaliser's channel-state values, one more kernel finds
 * their maximum and scales every soft bit in the reference's integer arithmetic, bit for bit (its pairwise weight swaps for QPSK and 64-QAM and the halving of
 * its 16-bit vector body included: csi_kernels.hip), still with one host wait.
 * The NR shared channels (pdsch_nr.c / pusch_nr.c, LDPC) have their own one-call-per-codeword entry points in phy_nr_chan_abi.h.
 */
#ifndef SRSRAN_AMD_PHY_CHAN_ABI_H
#define SRSRAN_AMD_PHY_CHAN_ABI_H

#include "srsran_amd/phy_modem_abi.h"
#include "srsran_amd/phy_sch_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the transport-block part every grant shares (srsran_ra_tb_t, ra.h:60-70, + what pusch.c / pdsch.c take from their cfg) */
typedef struct SRSRAN_API {
  uint32_t mod;                /* srsran_mod_t */
  uint32_t tbs;                /* transport block size in bits */
  uint32_t rv;                 /* redundancy version */
  uint32_t nof_re;             /* modulation symbols of the grant; nof_bits = nof_re * Qm */
  uint32_t seed;               /* c_init of the scrambling sequence: srsran_hip_sequence_pusch_seed / _pdsch_seed */
  uint32_t max_nof_iterations; /* turbo half iterations (srsran_sch_set_max_noi) */
  uint32_t llr_is_8bit;        /* q->llr_is_8bit: 8-bit soft bits, de-matcher and decoders */
  uint32_t nl;                 /* layers per codeword for the rate matcher's granularity Qm * Nl (sch.c:590,632: 2 when nof_layers != nof_tb); 0 = 1 */
} srsran_hip_grant_tb_t;

typedef struct SRSRAN_API {
  int32_t crc_ok;               /* 1 when every code block and the transport block passed (out->crc) */
  float   avg_iterations_block; /* q->ul_sch.avg_iterations / srsran_sch_last_noi */
  float   epre;                 /* PUSCH with meas_epre: average power of the extracted REs (linear; the caller converts to dB), else NAN */
} srsran_hip_grant_res_t;

/* ---- PUSCH receive (srsran_pusch_decode without UCI): sf_symbols / ce are the subframe's resource grids as srsran_ofdm_rx_sf and the channel
 * estimator leave them (14 or 12 symbols x 12 nof_prb), HOST memory; the grant's REs are taken from both as pusch.c:48-104 does. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb;
  uint32_t cell_nof_prb;   /* width of the grid */
  uint32_t cp_nsymb;       /* 7 (normal) or 6 (extended) symbols per slot */
  uint32_t n_prb_tilde[2]; /* first PRB of the allocation in each slot */
  uint32_t L_prb;          /* PRBs: transform precoding over 12 L_prb sub-carriers (srsran_dft_precoding_valid_prb) */
  uint32_t shortened;      /* last symbol taken by SRS */
  float    noise_estimate; /* channel->noise_estimate */
  uint32_t meas_epre;
} srsran_hip_pusch_rx_t;
SRSRAN_API int srsran_hip_pusch_decode(const srsran_hip_pusch_rx_t* g, const cf_t* sf_symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* data, srsran_hip_grant_res_t* res);
/* the grants of one TTI (the loop of srsenb/src/phy/lte/cc_worker.cc:359-371 over the UEs with a grant) in ONE call: one launch per stage and
 * block size over the code blocks of all grants.  Arrays of n entries; grants whose tb.llr_is_8bit / tb.max_nof_iterations differ are
 * decoded in separate passes.  Returns SRSRAN_SUCCESS when every grant was processed (res[i].crc_ok tells its outcome). */
SRSRAN_API int srsran_hip_pusch_decode_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const cf_t* const* sf_symbols, const cf_t* const* ce,
                                             srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data, srsran_hip_grant_res_t* res);

/* ---- PUSCH receive with control information (srsran_pusch_decode -> srsran_ulsch_decode, sch.c:1121-1192, with HARQ-ACK / RI / CQI configured).
 * With H' = tb.nof_re, cols = SC-FDMA symbols of the grant, rows = H' / cols: ACK symbol n sits in row rows - 1 - n / 4, column {2,3,8,9}[(3 n) % 4]
 * (cols > 10) or {1,2,6,7}; RI symbol n in the same row, column {1,4,7,10} or {0,3,5,8} (uci.c:364-416); soft bit k of the symbol at (row, col) has
 * position row Qm + rows col Qm + k in the reference's q_bits.  The data stream g is every symbol that is not an RI symbol, row by row, with zeros at
 * ACK symbols; its first Q_prime_cqi Qm soft bits are the CQI code word, the transport block is decoded from the G Qm behind it, G = H' - Q_prime_ri -
 * Q_prime_cqi.  (As in the reference, with Q_prime_ri > 0 g[0] holds the soft bit of the highest RI position: vector.c:141-146 on the table of
 * sch.c:660-681.)  Taken: 16-bit soft bits, Q_prime_ack and Q_prime_ri <= 4 * 12 * L_prb, Q_prime_ri + Q_prime_cqi < H'. */
typedef struct SRSRAN_API {
  uint32_t Q_prime_ack; /* modulation symbols punctured by HARQ-ACK (uci.c:418 Q_prime_ri_ack), 0 = none */
  uint32_t Q_prime_ri;  /* modulation symbols taken by RI, 0 = none */
  uint32_t Q_prime_cqi; /* modulation symbols of the CQI code word in front of the data (uci.c:173), 0 = none */
} srsran_hip_pusch_uci_t;
/* caller's memory; a pointer may be NULL when its count is 0.  *_llr: the demodulated and descrambled soft bit of bit k of symbol n at [n Qm + k]
 * (q_bits[position]); *_c: the scrambling chip c_seq[position] (the 1-bit decoder undoes the scrambling of the repeated bit with it, uci.c:678-682);
 * *_pos: the position; cqi_llr: g[0 .. Q_prime_cqi Qm) */
typedef struct SRSRAN_API {
  int16_t*  ack_llr;
  uint8_t*  ack_c;
  uint32_t* ack_pos; /* Q_prime_ack * Qm entries each */
  int16_t*  ri_llr;
  uint8_t*  ri_c;
  uint32_t* ri_pos;  /* Q_prime_ri * Qm entries each */
  int16_t*  cqi_llr; /* Q_prime_cqi * Qm entries */
} srsran_hip_pusch_uci_out_t;
/* uci: the three counts; out: where the control soft bits go.  All three counts 0: exactly srsran_hip_pusch_decode.  Still ONE host wait. */
SRSRAN_API int srsran_hip_pusch_decode_uci(const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* sf_symbols, const cf_t* ce,
                                           srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_pusch_uci_out_t* out);
/* the grants of one TTI, with and without control information, in ONE call: arrays of n entries (uci[i] all zero: a grant without; out[i] is then not
 * looked at).  One equaliser launch, one transform launch per allocation size, one demodulator launch per soft-bit width.  Every res[i] is initialised
 * before anything is checked; an invalid grant refuses the whole call (SRSRAN_ERROR_INVALID_INPUTS) before anything is enqueued. */
SRSRAN_API int srsran_hip_pusch_decode_uci_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_pusch_uci_t* uci, const cf_t* const* sf_symbols,
                                                 const cf_t* const* ce, srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data,
                                                 srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* out);

/* ---- PUSCH channel estimation on the device (srsran_chest_ul_estimate_pusch, chest_ul.c:370-404): with it the PUSCH grant calls start at the level of
 * srsran_enb_ul_get_pusch (enb_ul.c:272-281) -- subframe grid in, payload and the estimator's measurements out, no ce grid and no noise estimate from the
 * caller.  Per slot, with n = 12 L_prb and L(slot) = (slot + 1) cp_nsymb - 4: the received references are symbol L(slot) of the grid at sub-carriers
 * 12 n_prb_tilde[slot] + k; ls = rx conj(r); with filter_len 3 the estimate is srsran_conv_same_cf(ls, filter) (the virtual neighbour in front of element 0
 * is 3 ls[1] - 2 ls[0], the one behind the last 3 ls[n-1] - 2 ls[n-2]) and noise_estimate the calibrated mean |estimate - ls|^2 (chest_ul.c:200-221, the
 * calibration from filter[0]); with filter_len 0 the estimate is ls, noise_estimate 0 and snr NAN.  The slot's row is the estimate of every symbol of the slot
 * (no time interpolation: the reference compiles none in).  cfo_hz, ta_us (0 unless meas_ta_en), snr and the dB values as chest_ul.c:300-326, :358-367.
 * Intra-subframe hopping (n_prb_tilde[0] != n_prb_tilde[1]) is taken: each slot is estimated where the UE sent it.  The reference's estimator logs an error
 * there and places its rows by n_prb (chest_ul.c:329-331), so the record the library is tested against (tests/golden/chest_ul_ref.npz) has no such case.
 * Not taken: generating the DMRS rows (the caller's pregen table is handed over), the PUCCH and SRS estimators, filters longer than 3 taps, rsrp / epre of
 * srsran_chest_ul_res_t (the PUSCH estimator does not set them). */
typedef struct SRSRAN_API {
  uint32_t    filter_len;  /* 3: {w, 1-2w, w} in filter[] (the reference's default: w = 0.3333f); 0: no smoothing */
  float       filter[3];
  uint32_t    meas_ta_en;
  const cf_t* r;           /* the grant's DMRS row, dmrs_pregen.r[n_dmrs][tti % 10][L_prb]: 2 x 12 L_prb points, HOST memory */
} srsran_hip_chest_ul_t;

typedef struct SRSRAN_API {   /* what srsran_chest_ul_estimate_pusch leaves in srsran_chest_ul_res_t */
  float noise_estimate, noise_estimate_dbm, snr, snr_db, cfo_hz, ta_us;
} srsran_hip_chest_ul_res_t;
/* the stage by itself.  Of g only the geometry is read: cell_nof_prb, cp_nsymb, n_prb_tilde[], L_prb.  sf_symbols: the subframe grid, HOST memory.  ce: a
 * full grid of HOST memory -- only the grant's columns of all 2 cp_nsymb symbols are written -- or NULL for the measurements only.  One launch (one
 * workgroup per grant), one host wait.  Refused before the device is looked for, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS, *out zeroed and
 * nothing else written: a NULL g, est, est->r, sf_symbols or out, a geometry that is not a PUSCH allocation (as srsran_hip_pusch_decode), filter_len other
 * than 0 or 3, a filter tap that is not finite. */
SRSRAN_API int srsran_hip_chest_ul_estimate_pusch(const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const cf_t* sf_symbols, cf_t* ce,
                                                  srsran_hip_chest_ul_res_t* out);
/* arrays of n entries (ce, or any ce[i], may be NULL) */
SRSRAN_API int srsran_hip_chest_ul_estimate_pusch_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est,
                                                        const cf_t* const* sf_symbols, cf_t* const* ce, srsran_hip_chest_ul_res_t* out);
/* the grant calls: srsran_hip_pusch_decode_uci{,_multi} without the ce argument.  g->noise_estimate is not read: the estimator's kernel runs ahead of the
 * equaliser on the same stream and hands it the rows and the noise estimate on the device; est_out[i] is filled after the call's ONE host wait.  uci may
 * be NULL, or uci[i] all zero for a grant without control information (uci_out[i] is then not looked at); the rules are those of srsran_hip_pusch_decode_uci.
 * The single call is the multi call with n = 1.  Refused before the device is looked for, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS, every res[i]
 * = {0, 0, NAN}, every est_out[i] zeroed and nothing else written: everything srsran_hip_pusch_decode_uci refuses, a NULL est, est[i].r or est_out,
 * filter_len other than 0 or 3, a filter tap that is not finite. */
SRSRAN_API int srsran_hip_pusch_decode_est(const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const srsran_hip_pusch_uci_t* uci,
                                           const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res,
                                           srsran_hip_pusch_uci_out_t* uci_out, srsran_hip_chest_ul_res_t* est_out);
SRSRAN_API int srsran_hip_pusch_decode_est_multi(uint32_t n, const srsran_hip_pusch_rx_t* g, const srsran_hip_chest_ul_t* est, const srsran_hip_pusch_uci_t* uci,
                                                 const cf_t* const* sf_symbols, srsran_softbuffer_rx_t* const* softbuffers, uint8_t* const* data,
                                                 srsran_hip_grant_res_t* res, const srsran_hip_pusch_uci_out_t* uci_out, srsran_hip_chest_ul_res_t* est_out);

/* ---- PDSCH receive, one codeword: `symbols` are the grant's nof_re extracted REs (srsran_pdsch_get) of HOST memory.  ce != NULL: single
 * port, single receive antenna -- the zero-forcing / MMSE equaliser srsran_predecoding_single(symbols, ce, ., NULL, nof_re, scaling,
 * noise_estimate) runs on the device; ce == NULL: `symbols` are already equalised and layer-demapped (q->d[codeword], pdsch.c:880-899). */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb;
  float scaling;        /* pdsch_scaling (rho_a), 1.0f without power allocation */
  float noise_estimate; /* 0 for SRSRAN_MIMO_DECODER_ZF */
} srsran_hip_pdsch_rx_t;
SRSRAN_API int srsran_hip_pdsch_decode(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                       uint8_t* data, srsran_hip_grant_res_t* res);
/* the same, and the intermediate results the reference leaves in the PDSCH object where its callers can see them (lib/test/phy/phy_dl_test.c:253-298 compares
 * both with the transmitter's): d_out (or NULL) <- the nof_re equalised symbols (q->d[cw]; only written when ce != NULL -- otherwise they are `symbols`),
 * e_out (or NULL) <- the nof_re * Qm descrambled soft bits (q->e[cw]: int16, int8 with llr_is_8bit).  Each costs a device -> host copy.
 * SRSRAN_ERROR when an output that was asked for was not produced: the front end does not run for a codeword whose soft buffer has fewer rows than it has code
 * blocks, or whose code blocks were all decoded in an earlier round.  That output is left untouched; *res is filled as usual.  (d_out with ce == NULL is
 * never written and is not such an output.)  A device-side failure returns SRSRAN_ERROR, in this and in the plain call. */
SRSRAN_API int srsran_hip_pdsch_decode_dbg(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, srsran_softbuffer_rx_t* softbuffer,
                                           uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out);

/* the same with cfg->csi_enable: the soft bits are weighted with the codeword's channel-state values (csi_correction, pdsch.c:523-618) in front of the transport
 * block.  ce != NULL: the values are the equaliser's (what srsran_predecoding_single files in q->csi[0]) and `csi` must be NULL; ce == NULL: `csi` is the
 * caller's q->csi[cw], nof_re floats of HOST memory, required -- this form keeps the weighting, the rate de-matching and the decoding on the device for the
 * port / antenna counts the library does not equalise.  Refused like the plain call, and with one line on stderr and SRSRAN_ERROR_INVALID_INPUTS before
 * anything is enqueued: both or neither of ce and csi, a caller's csi entry that is negative or not finite.
 * _dbg: e_out <- the WEIGHTED soft bits (what q->e[cw] holds when srsran_pdsch_decode returns), csi_out (or NULL) <- the nof_re values that were used;
 * SRSRAN_ERROR, as in srsran_hip_pdsch_decode_dbg, when one of them was asked for and not produced. */
SRSRAN_API int srsran_hip_pdsch_decode_csi(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, const float* csi,
                                           srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res);
SRSRAN_API int srsran_hip_pdsch_decode_csi_dbg(const srsran_hip_pdsch_rx_t* g, const cf_t* symbols, const cf_t* ce, const float* csi,
                                               srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                               float* csi_out);

/* ---- PDSCH transmit, one codeword (srsran_pdsch_codeword_encode, pdsch.c:949-1015, + the scaling of :1116-1120): payload bytes ->
 * CRC24A, segmentation, CRC24B, turbo coding, rate matching (encode_tb, sch.c:238-368) -> scrambling -> constellation points x scaling.
 * data == NULL: a retransmission of what the soft buffer holds.  symbols: nof_re points, HOST memory. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb; /* max_nof_iterations, llr_is_8bit unused */
  float scaling;            /* 1.0f: none */
} srsran_hip_pdsch_tx_t;
SRSRAN_API int srsran_hip_pdsch_encode(const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* symbols);
/* the same, and e_out (or NULL) <- the scrambled, byte-packed coded bits the reference leaves in q->e[cw] (pdsch.c:1005-1012), nof_re * Qm bits rounded
 * up to whole bytes */
/* the codewords of one TTI in ONE call (the loop over the scheduled UEs of srsenb/src/phy/lte/cc_worker.cc encode_pdsch, each of which ends in
 * srsran_pdsch_encode, pdsch.c:1017): arrays of n entries, one coding launch over the code blocks of all of them and one scrambling + modulation launch. */
SRSRAN_API int srsran_hip_pdsch_encode_multi(uint32_t n, const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* const* softbuffers, uint8_t* const* data,
                                             cf_t* const* symbols);
SRSRAN_API int srsran_hip_pdsch_encode_dbg(const srsran_hip_pdsch_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* symbols, uint8_t* e_out);

/* ---- PDSCH with transmit diversity, one codeword on a 2- or 4-port cell (pdsch.c:788 / :1017 with tx_scheme == SRSRAN_TXSCHEME_DIVERSITY, nof_tb == 1,
 * nof_layers == cell.nof_ports).  Receive: symbols[rx] are the grant's nof_re extracted REs of each receive antenna, ce[port][rx] the channel estimates at the
 * same REs (q->symbols, q->ce after srsran_pdsch_get), HOST memory.  srsran_predecoding_diversity_multi (phy_modem_abi.h: the arithmetic and its limits) ->
 * srsran_layerdemap_diversity -> demodulator -> descrambler are ONE kernel; the combined symbols never reach memory.  One host wait.
 * Refused before anything is enqueued, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS, *res zeroed and nothing else written: NULL pointers or a NULL
 * plane inside the used range, nof_ports not 2 or 4, nof_rx not 1 or 2, nof_re odd (2 ports) or not a multiple of 4 (4 ports), scaling 0 or not finite,
 * and what every grant call refuses (modulation, tbs, rv, length); *res = {0, 0, NAN} then.  A device-side failure returns SRSRAN_ERROR. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb; /* tb.nl is taken as 2 (sch.c:590,632: nof_layers != nof_tb); tb.nof_re = REs of the grant */
  uint32_t nof_ports;       /* 2 or 4 */
  uint32_t nof_rx;          /* 1 or 2 */
  float    scaling;         /* pdsch_scaling: rho_a as pdsch.c:486-520 returns it (with the sqrt 2 of a multi-port cell) */
  uint32_t reserved;
} srsran_hip_pdsch_txdiv_rx_t;
/* symbols, ce: what a caller passes q->symbols and q->ce as (cf_t* symbols[SRSRAN_MAX_PORTS], cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = [port][rx]:
 * plain C converts both without a cast); the planes are only read */
SRSRAN_API int srsran_hip_pdsch_decode_txdiv(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                             srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res);
/* the same, and d_out (or NULL) <- the nof_re combined, layer-demapped symbols (q->d[0]; made by the per-stage kernels in this case only: same arithmetic),
 * e_out (or NULL) <- the nof_re * Qm descrambled soft bits (q->e[0]: int16, int8 with llr_is_8bit).  SRSRAN_ERROR, as in srsran_hip_pdsch_decode_dbg, when an
 * output that was asked for was not produced (here and in _csi_dbg). */
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                 srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out);
/* the same with cfg->csi_enable: the soft bits are weighted with the combiner's channel-state values (what srsran_predecoding_diversity_multi files in
 * q->csi[0]); arguments and refusals of the plain calls.  _dbg: e_out <- the WEIGHTED soft bits, csi_out (or NULL) <- the nof_re values that were used. */
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_csi(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                 srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res);
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_csi_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                     srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                                     float* csi_out);
/* Transmit: srsran_hip_pdsch_encode's coding pass, then scrambling + modulation + srsran_layermap_diversity + srsran_precoding_diversity in one kernel:
 * symbols[port] <- nof_re points each (HOST memory), ready for srsran_pdsch_put per port; no intermediate d reaches memory.  scaling: what pdsch.c:486-492
 * returns on an eNB object (rho_a sqrt 2 on a multi-port cell); the precoder's 1 / sqrt 2 is applied inside.  data == NULL: a
 * retransmission of what the soft buffer holds.  Refusals as on the receive side. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb; /* tb.nl taken as 2; max_nof_iterations, llr_is_8bit unused */
  uint32_t nof_ports;       /* 2 or 4 */
  float    scaling;
} srsran_hip_pdsch_txdiv_tx_t;
SRSRAN_API int srsran_hip_pdsch_encode_txdiv(const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* const symbols[]);
/* the codewords of one TTI in ONE call: one coding launch, one modulation + precoding launch, one host wait; symbols[i][port] */
SRSRAN_API int srsran_hip_pdsch_encode_txdiv_multi(uint32_t n, const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* const* softbuffers,
                                                   uint8_t* const* data, cf_t* const* const* symbols);

/* ---- PDSCH with spatial multiplexing or large-delay CDD on a 2-port cell, 2 receive antennas: one or two codewords in ONE call (pdsch.c:788 / :1017 with
 * tx_scheme == SRSRAN_TXSCHEME_CDD or SRSRAN_TXSCHEME_SPATIALMUX).  Taken: CDD with 2 layers and 2 codewords; spatial multiplexing with 2 layers and 2
 * codewords (codebook_idx 0 .. 2 = pmi + 1, pdsch.c:867) or 1 layer and 1 codeword (codebook_idx 0 .. 3).  Layer mapping is the identity in all three
 * (nof_layers == nof_tb, pdsch.c:858): codeword k is layer k.  The arithmetic, its limits and the decoder values: srsran_hip_predecoding_mimo (phy_modem_abi.h).
 * Receive: symbols[rx], ce[port][rx] as for transmit diversity (nof_re REs each, HOST memory, only read).  One staging image (2 + 4 planes), one front-end
 * kernel for both codewords (srsran_hip_predecoding_mimo's arithmetic -> demodulator -> descrambler per codeword; the equalised symbols never reach memory),
 * one decoding pass over the code blocks of both transport blocks, one host wait.  softbuffers[k] == NULL skips codeword k (the reference skips a transport
 * block whose crc is already set, pdsch.c:893): its layer is still part of the solve, res[k] = {0, 0, NAN}, data[k] is not touched.  Both res entries are
 * initialised before anything is checked.
 * Refused before anything is enqueued, with one line on stderr and SRSRAN_ERROR_INVALID_INPUTS: NULL arguments or a NULL plane, nof_rx != 2, a (tx_scheme,
 * nof_layers, nof_tb) other than the three above (4 ports have no field: the reference refuses them, precoding.c:1035, :1852, :2078), a codebook_idx out of
 * range, an odd nof_re with CDD, a decoder that is neither ZF nor MMSE, scaling 0 or not finite, a negative or non-finite noise_estimate, two codewords
 * whose nof_re, llr_is_8bit or max_nof_iterations differ, every codeword skipped, and what every grant call refuses per codeword (modulation, tbs, rv,
 * length).  A device-side failure returns SRSRAN_ERROR.
 * Not taken: PMI and condition-number selection, EVM, resource mapping on transmit (de-mapping: the _sf form below), 4 ports. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb[2]; /* tb[k]: codeword k; seed with q = k; tb[k].nl is taken as 1; nof_re = REs of the grant, the same in both */
  uint32_t nof_tb;             /* 1 or 2 */
  uint32_t nof_layers;         /* = nof_tb */
  uint32_t tx_scheme;          /* SRSRAN_HIP_TXSCHEME_CDD or SRSRAN_HIP_TXSCHEME_SPATIALMUX */
  uint32_t codebook_idx;       /* spatial multiplexing only */
  uint32_t decoder;            /* SRSRAN_HIP_MIMO_DECODER_ZF or _MMSE (two layers) */
  uint32_t nof_rx;             /* 2 */
  float    scaling;            /* pdsch_scaling */
  float    noise_estimate;     /* MMSE: added to the diagonal; 0 is what srsran_pdsch_decode passes for SRSRAN_MIMO_DECODER_ZF */
} srsran_hip_pdsch_mimo_rx_t;
SRSRAN_API int srsran_hip_pdsch_decode_mimo(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                            srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                            srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS]);
/* the same, and per codeword (the array or an entry may be NULL) d_out[k] <- the nof_re equalised symbols of layer k (q->d[k]; made by the per-stage kernel
 * in this case only: same arithmetic), e_out[k] <- the nof_re * Qm descrambled soft bits (q->e[k]: int16, int8 with llr_is_8bit; not for a skipped codeword).
 * SRSRAN_ERROR when an output that was asked for was not produced: the front end does not run for a codeword whose soft buffer has fewer rows than it has code
 * blocks, or whose code blocks were all decoded in an earlier round.  That output is left untouched; res[] is filled as usual. */
SRSRAN_API int srsran_hip_pdsch_decode_mimo_dbg(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], cf_t* const d_out[SRSRAN_MAX_CODEWORDS],
                                                void* const e_out[SRSRAN_MAX_CODEWORDS]);
/* the same with cfg->csi_enable: codeword k's soft bits are weighted with layer k's channel-state values (what srsran_hip_predecoding_mimo files in
 * q->csi[k]), both codewords in one launch; arguments and refusals of the plain calls.  Two-layer zero-forcing spatial multiplexing is undefined in the
 * reference: its equaliser writes q->csi[0] only, all 1.0 (precoding.c:1330-1331), and codeword 1 is weighted with whatever an earlier call left in q->csi[1];
 * the library uses 1.0 for that row as well.  _dbg: e_out[k] <- the WEIGHTED soft bits, csi_out[k] (the array or an entry may be NULL; not for a skipped
 * codeword) <- the nof_re values that were used. */
SRSRAN_API int srsran_hip_pdsch_decode_mimo_csi(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS]);
SRSRAN_API int srsran_hip_pdsch_decode_mimo_csi_dbg(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                    srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                    srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], cf_t* const d_out[SRSRAN_MAX_CODEWORDS],
                                                    void* const e_out[SRSRAN_MAX_CODEWORDS], float* const csi_out[SRSRAN_MAX_CODEWORDS]);
/* Transmit: one coding launch over the code blocks of the grant's codewords, then scrambling + modulation of each codeword + srsran_hip_precoding_mimo's
 * arithmetic in one kernel: symbols[port] <- nof_re points each (HOST memory), ready for srsran_pdsch_put per port.  data[k] == NULL: a retransmission of what
 * softbuffers[k] holds.  Refusals as on the receive side (both soft buffers of a two-codeword grant are needed). */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb[2]; /* as above; max_nof_iterations, llr_is_8bit unused */
  uint32_t nof_tb;
  uint32_t nof_layers;
  uint32_t tx_scheme;
  uint32_t codebook_idx;
  float    scaling;
} srsran_hip_pdsch_mimo_tx_t;
SRSRAN_API int srsran_hip_pdsch_encode_mimo(const srsran_hip_pdsch_mimo_tx_t* g, srsran_softbuffer_tx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                            uint8_t* const data[SRSRAN_MAX_CODEWORDS], cf_t* const symbols[]);
/* the grants of one TTI in ONE call: one coding launch, one modulation + precoding launch, one host wait; softbuffers[i][k], data[i][k], symbols[i][port] */
SRSRAN_API int srsran_hip_pdsch_encode_mimo_multi(uint32_t n, const srsran_hip_pdsch_mimo_tx_t* g, srsran_softbuffer_tx_t* const (*softbuffers)[SRSRAN_MAX_CODEWORDS],
                                                  uint8_t* const (*data)[SRSRAN_MAX_CODEWORDS], cf_t* const* const* symbols);

/* ---- PDSCH receive from the subframe grids: RE de-mapping on the device.  The _sf form of each receive call starts where srsran_pdsch_decode does
 * (pdsch.c:788): it takes the subframe grids (sf_symbols[rx]) and the channel estimator's grids (channel->ce[port][rx]), HOST memory, (nof_symb_slot[0] +
 * nof_symb_slot[1]) * 12 * cell_nof_prb points each, where its twin takes the nof_re REs srsran_pdsch_get (pdsch.c:246; srsran_pdsch_cp :136-220) extracts
 * from them.  The host copies the used rows of every grid into the staging image (symbol lstart to the grant's last symbol; whole rows, or the span from the
 * lowest to the highest allocated PRB), ONE more launch de-maps all nof_rx * (1 + nof_ports) planes into device scratch around the reference signals, PSS / SSS
 * and PBCH (half PRBs on a cell with an odd PRB count), and the twin's kernels run on those planes unchanged: one launch more than the twin, still one host
 * wait.  apply_power_allocation (pdsch.c:809) stays with the caller, as for the twins.  The transmit direction (srsran_pdsch_put) is not taken. */
typedef struct SRSRAN_API {
  uint32_t cell_nof_prb;     /* 6 .. 110: width of the grids */
  uint32_t cell_nof_ports;   /* 1, 2 or 4: decides the CRS pattern */
  uint32_t cell_id;          /* 0 .. 503 */
  uint32_t cp_nsymb;         /* 7 or 6 */
  uint32_t frame_type;       /* 0 FDD, 1 TDD */
  uint32_t sf_idx;           /* sf->tti % 10 */
  uint32_t lstart;           /* SRSRAN_NOF_CTRL_SYMBOLS(cell, cfi) */
  uint32_t nof_symb_slot[2]; /* grant->nof_symb_slot */
  uint32_t csi_enable;       /* cfg->csi_enable */
  uint8_t  prb_idx[2][110];  /* grant->prb_idx (bool [2][SRSRAN_MAX_PRB]) */
} srsran_hip_pdsch_sf_t;
/* host only: the count srsran_pdsch_get would return for this description, or -1 for an invalid one (a field outside the ranges above, nof_symb_slot[s] >
 * cp_nsymb, lstart >= nof_symb_slot[0], csi_enable above 1, a prb_idx byte above 1, an empty allocation) */
SRSRAN_API int srsran_hip_pdsch_nof_re(const srsran_hip_pdsch_sf_t* sf);
/* the stage by itself on HOST buffers: symbols[p] <- the nof_re REs of grids[p], p < n_planes, all planes in ONE launch.  Returns nof_re, or -1 (an invalid
 * description, a NULL pointer, no device) */
SRSRAN_API int srsran_hip_pdsch_get(const srsran_hip_pdsch_sf_t* sf, uint32_t n_planes, const cf_t* const* grids, cf_t* const* symbols);
/* the grant calls.  Arguments of the twin with `sf` behind `g` and grids where the planes went; sf->csi_enable selects what the _csi twin does.  (The one-port
 * call needs ce: the "already equalised" form has no grid.)  Refused before the device is looked for, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS,
 * *res = {0, 0, NAN} and nothing else written: everything the twin refuses, a NULL sf, what srsran_hip_pdsch_nof_re refuses, csi_enable above 1, a
 * cell_nof_ports that is not the call's (1; nof_ports; 2), and srsran_hip_pdsch_nof_re(sf) != tb.nof_re (the reference's "expecting %d symbols but got %d",
 * pdsch.c:834).
 * _sf_dbg: the outputs of the _csi_dbg twin (csi_out is only written with csi_enable) and the extracted planes, sym_out[rx] <- q->symbols[rx], ce_out[port][rx]
 * <- q->ce[port][rx], nof_re points each; either array, or any entry of it, may be NULL.  They cost one device -> host copy. */
SRSRAN_API int srsran_hip_pdsch_decode_sf(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const cf_t* sf_symbols, const cf_t* ce,
                                          srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res);
SRSRAN_API int srsran_hip_pdsch_decode_sf_dbg(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const cf_t* sf_symbols, const cf_t* ce,
                                              srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                              float* csi_out, cf_t* sym_out, cf_t* ce_out);
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_sf(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                                srsran_hip_grant_res_t* res);
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_sf_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                    cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                                    srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out, float* csi_out, cf_t* const sym_out[],
                                                    cf_t* const (*ce_out)[SRSRAN_MAX_PORTS]);
SRSRAN_API int srsran_hip_pdsch_decode_mimo_sf(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                               cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                               uint8_t* const data[SRSRAN_MAX_CODEWORDS], srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS]);
SRSRAN_API int srsran_hip_pdsch_decode_mimo_sf_dbg(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                   cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                                   uint8_t* const data[SRSRAN_MAX_CODEWORDS], srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS],
                                                   cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS],
                                                   float* const csi_out[SRSRAN_MAX_CODEWORDS], cf_t* const sym_out[],
                                                   cf_t* const (*ce_out)[SRSRAN_MAX_PORTS]);

/* ---- Downlink channel estimation on the device (srsran_chest_dl_estimate_cfg, chest_dl.c:1004, with estimate_port, average_pilots, interpolate_pilots, the
 * three noise estimators, chest_dl_rssi, chest_estimate_cfo and fill_res, srsran_conv_same_cf, srsran_interp_linear_offset and srsran_interp_linear_vector{,2}),
 * restated AS WRITTEN: with it the PDSCH receive calls start at the level of srsran_ue_dl_decode_fft_estimate / srsran_pdsch_decode.  One launch, one
 * workgroup per (rx antenna, port) pair, one host wait; a call gives the same bits every time.  Kept as the reference has them: estimate_noise_pilots
 * returns the last CRS symbol's power only; get_rsrp walks ports with an antenna counter; srsran_conv_same_cf's uneven end extrapolation; the AVERAGE path
 * interpolates every port with offset id % 3 and, without a filter, reads the first 4 nof_prb raw estimates as one row; ports 2 and 3 extrapolate the symbols
 * behind their second CRS symbol from the first; time interpolation is a chain of additions; automatic Gauss taps from a noise estimate of 0 give a filter of
 * length 0 and a ce of zeros.  One difference: ce is computed whether or not the caller takes it, so the PSS / EMPTY noise estimates do not depend on a NULL
 * ce (the reference skips them then).
 * Taken: SRSRAN_SF_NORM subframes with the full CRS pattern; 1, 2 and 4 ports; 1 .. 4 receive antennas; both cyclic prefixes; 6 .. 110 PRB; AVERAGE and
 * INTERPOLATE; filters NONE, TRIANGLE and GAUSS (fixed taps: order filter_coef[0] <= 8, i.e. at most 9 taps; automatic taps with filter_coef[0] <= 0: order 4,
 * std 200 x the pair's noise estimate -- this call's with REFS, the state's otherwise); noise algorithms REFS, PSS and EMPTY; rsrp_neighbour; the CFO estimate
 * on cells of 1 or 2 ports.
 * State is the caller's: the reference's object keeps noise_estimate[rx][port] and cfo between subframes (PSS / EMPTY estimates change in subframes 0 and 5
 * only, cfo in the subframes of the mask only); the caller hands them in (all zero at start) and takes them from res->state.  rsrp_corr without
 * rsrp_neighbour and sync_err are 0 (a fresh object's).
 * Refused before the device is looked for, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS, *res zeroed and nothing else written: NULL cfg, state, grids
 * or res, a NULL grid or pilot row that the call reads, a field out of range, estimator_alg WIENER, sf_type MBSFN, a TDD special subframe, sync_error_enable
 * (it rewrites the caller's grid), more than 9 taps or a non-finite coefficient that is read, cfo_estimate_enable on a 4-port cell (the reference reads the
 * previous port's stale estimates there), noise_alg PSS without pss_signal, a negative or non-finite state. */
#define SRSRAN_HIP_ESTIMATOR_ALG_AVERAGE 0 /* srsran_chest_dl_estimator_alg_t */
#define SRSRAN_HIP_ESTIMATOR_ALG_INTERPOLATE 1
#define SRSRAN_HIP_ESTIMATOR_ALG_WIENER 2 /* refused */
#define SRSRAN_HIP_NOISE_ALG_REFS 0 /* srsran_chest_dl_noise_alg_t */
#define SRSRAN_HIP_NOISE_ALG_PSS 1
#define SRSRAN_HIP_NOISE_ALG_EMPTY 2
#define SRSRAN_HIP_CHEST_FILTER_GAUSS 0 /* srsran_chest_filter_t */
#define SRSRAN_HIP_CHEST_FILTER_TRIANGLE 1
#define SRSRAN_HIP_CHEST_FILTER_NONE 2
#define SRSRAN_HIP_CHEST_DL_MAX_TAPS 9
typedef struct SRSRAN_API {
  uint32_t nof_prb;              /* cell: 6 .. 110 */
  uint32_t nof_ports;            /* 1, 2 or 4 */
  uint32_t id;                   /* 0 .. 503 */
  uint32_t cp_nsymb;             /* 7 or 6 */
  uint32_t nof_rx;               /* q->nof_rx_antennas: 1 .. 4 */
  uint32_t sf_idx;               /* sf->tti % 10 */
  uint32_t sf_type;              /* sf->sf_type: 0 (SRSRAN_SF_NORM); 1 (MBSFN) is refused */
  uint32_t tdd_special;          /* 1: a TDD special subframe (srsran_sfidx_tdd_type(...) == SRSRAN_TDD_SF_S) -- refused */
  uint32_t estimator_alg;        /* cfg->estimator_alg */
  uint32_t noise_alg;            /* cfg->noise_alg */
  uint32_t filter_type;          /* cfg->filter_type */
  float    filter_coef[2];       /* cfg->filter_coef */
  uint32_t rsrp_neighbour;       /* cfg->rsrp_neighbour */
  uint32_t cfo_estimate_enable;  /* cfg->cfo_estimate_enable */
  uint32_t cfo_estimate_sf_mask; /* cfg->cfo_estimate_sf_mask */
  uint32_t sync_error_enable;    /* cfg->sync_error_enable: 1 is refused */
  uint32_t decoder_zf;           /* read by srsran_hip_pdsch_decode_est only: 1 = cfg->decoder_type is SRSRAN_MIMO_DECODER_ZF, the equaliser gets 0 in place of
                                    get_noise() (pdsch.c:819); 0 or 1 */
  const cf_t* pilots[2];         /* q->csr_refs.pilots[p][sf_idx]: 8 nof_prb points (ports 0, 1) and 4 nof_prb points (ports 2, 3; read on a 4-port cell), HOST
                                    memory.  The library does not generate the CRS rows */
  const cf_t* pss_signal;        /* q->pss_signal, 62 points: read with noise_alg PSS, may be NULL otherwise */
} srsran_hip_chest_dl_t;
typedef struct SRSRAN_API { /* what the reference's object carries from subframe to subframe */
  float noise_estimate[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; /* [rx][port] */
  float cfo;
} srsran_hip_chest_dl_state_t;
typedef struct SRSRAN_API { /* srsran_chest_dl_res_t behind fill_res (entries it does not set are 0), the object's per-pair values, the state out */
  float noise_estimate;
  float noise_estimate_dbm;
  float snr_db;
  float snr_ant_port_db[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];
  float rsrp;
  float rsrp_dbm;
  float rsrp_neigh;
  float rsrp_port_dbm[SRSRAN_MAX_PORTS];
  float rsrp_ant_port_dbm[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];
  float rsrq;
  float rsrq_db;
  float rsrq_ant_port_db[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];
  float rssi_dbm;
  float cfo;
  float sync_error;                                    /* 0 */
  float rsrp_pair[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];      /* q->rsrp[rx][port] */
  float rssi_pair[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];      /* q->rssi[rx][port] */
  float rsrp_corr_pair[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; /* q->rsrp_corr[rx][port] */
  srsran_hip_chest_dl_state_t state;                   /* hand it to the next subframe's call */
} srsran_hip_chest_dl_res_t;
/* the stage by itself.  A UE binding no longer needs it ahead of PCFICH / PHICH and the PDCCH search: they run on the device, and
 * srsran_hip_pdcch_search_est (phy_conv_abi.h) chains this estimator, both channels and the search in one call from the received grids; the calls that take
 * these estimates (srsran_hip_pcfich_decode, srsran_hip_phich_decode_multi, srsran_hip_pdcch_search_sf) remain for callers that hold them.  sf_symbols[rx]: the
 * received grids, 2 cp_nsymb x 12 nof_prb points each, HOST memory, only read.  ce: NULL (the measurements only), or what a caller passes res->ce as
 * (cf_t* ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = [port][rx]); a NULL entry is not written.  The measurements do not depend on which entries are there. */
SRSRAN_API int srsran_hip_chest_dl_estimate(const srsran_hip_chest_dl_t* cfg, const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                            cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_hip_chest_dl_res_t* res);

/* the grant calls from the grids alone: the arguments of the _sf twin without ce, and the estimator's description, the state and est_out (what the stage
 * returns) in their place.  The caller's noise_estimate is not read: the equaliser takes get_noise() of this subframe's estimates (chest_dl.c:868-878), averaged
 * on the device, or 0 when the grant asks for zero forcing (pdsch.c:819: est->decoder_zf on one port, g->decoder with MIMO; diversity combining takes none).
 * Inside the one receive frame the host stages the received grids only (whole: the estimator reads every CRS symbol), the estimator's kernel writes the ce
 * grids into device scratch, the de-mapping kernel reads them there, and the twin's front-end kernels run unchanged: one launch more than the _sf twin, still
 * one host wait.  The call re-estimates rather than taking a handle from the stage call: between the two the UE finds the CFI on the host and searches the PDCCH
 * (srsran_hip_pdcch_search_sf, phy_conv_abi.h: a call of its own, since the grant is its result).
 * Refused before the device is looked for, with one line on stderr, SRSRAN_ERROR_INVALID_INPUTS, *res = {0, 0, NAN}, *est_out zeroed and nothing else written:
 * everything the _sf twin refuses, everything srsran_hip_chest_dl_estimate refuses, an estimator description whose cell, subframe or antenna count is not
 * the call's, a grant that does not span both whole slots (nof_symb_slot[s] != cp_nsymb: the estimator's grids), decoder_zf above 1.
 * SRSRAN_ERROR with est_out left zeroed when the front end did not run (every code block decoded in an earlier round, or a soft buffer with too few rows).
 * _est_dbg: the outputs of the _sf_dbg twin and ce_grid_out[port][rx] (the array or an entry may be NULL) <- the pair's whole ce grid. */
SRSRAN_API int srsran_hip_pdsch_decode_est(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                           const srsran_hip_chest_dl_state_t* state_in, const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                           srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out);
SRSRAN_API int srsran_hip_pdsch_decode_est_dbg(const srsran_hip_pdsch_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                               const srsran_hip_chest_dl_state_t* state_in, const cf_t* sf_symbols, srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                               srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out, cf_t* d_out, void* e_out, float* csi_out, cf_t* sym_out,
                                               cf_t* ce_out, cf_t* ce_grid_out);
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_est(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                 const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* softbuffer,
                                                 uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out);
SRSRAN_API int srsran_hip_pdsch_decode_txdiv_est_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                     const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* softbuffer,
                                                     uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out, cf_t* d_out, void* e_out,
                                                     float* csi_out, cf_t* const sym_out[], cf_t* const (*ce_out)[SRSRAN_MAX_PORTS],
                                                     cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS]);
SRSRAN_API int srsran_hip_pdsch_decode_mimo_est(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], srsran_hip_chest_dl_res_t* est_out);
SRSRAN_API int srsran_hip_pdsch_decode_mimo_est_dbg(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                    const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                                    srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                    srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], srsran_hip_chest_dl_res_t* est_out,
                                                    cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS],
                                                    float* const csi_out[SRSRAN_MAX_CODEWORDS], cf_t* const sym_out[], cf_t* const (*ce_out)[SRSRAN_MAX_PORTS],
                                                    cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS]);

/* ---- UL-SCH transmit without UCI (srsran_ulsch_encode, sch.c:1194-1340, with no ACK / RI / CQI configured): encode_tb -> channel
 * interleaver of 36.212 5.2.2.8 over nof_symb columns.  q_bits: nof_bits = nof_re * Qm bits, byte packed (what pusch.c:322 scrambles next). */
SRSRAN_API int srsran_hip_ulsch_encode(const srsran_hip_grant_tb_t* tb, uint32_t nof_symb, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, uint8_t* q_bits);

/* ---- PUSCH transmit, with or without control information: all of srsran_pusch_encode (pusch.c:259-354) in one call.  The transport block is coded for
 * G Qm bits, G = H' - Q_prime_ri - Q_prime_cqi (H' = tb.nof_re); ONE kernel then does srsran_ulsch_encode's multiplexing (sch.c:1194-1337: the CQI code word in
 * front of the data stream, the channel interleaver around the RI positions, RI and ACK bits at the positions of uci.c:364-416, computed in closed form as on
 * the receive side), srsran_sequence_pusch_apply_pack, the placeholder / repetition fix-up of pusch.c:315-331 and the modulator; one transform launch over
 * 12 L_prb points per SC-FDMA symbol follows, and after the call's ONE host wait the precoded rows are copied to their places in sf_symbols (pusch_put,
 * pusch.c:48-100: every symbol but each slot's reference symbol and, when shortened, the last).  The block codes are NOT built here: the caller runs the
 * reference's srsran_uci_encode_ack_ri / srsran_uci_encode_cqi_pusch and hands over what they leave -- the .type of every ACK / RI bit (a bit of type 1 is sent
 * as 1, every other type as 0; after scrambling a placeholder becomes 1 and a repetition at position p > 1 the bit at p - 1, in the order of the reference's
 * list: RI first) and the coded CQI bits.
 * Refused before anything is enqueued, with one line on stderr and SRSRAN_ERROR_INVALID_INPUTS: a NULL argument (uci may be NULL: no control information; in
 * may be NULL when all counts are 0; data may be NULL: a retransmission of what the soft buffer holds), an allocation that is not a PUSCH allocation (as on the
 * receive side), a modulation outside QPSK .. 64-QAM, Q_prime_ack or Q_prime_ri above 4 * 12 * L_prb, Q_prime_ri + Q_prime_cqi >= H', a NULL array for a
 * non-zero count, a type byte above 3, a cqi_bits byte above 1, tbs == 0 (CQI only: stays with the caller, as on the receive side).  A device-side failure
 * returns SRSRAN_ERROR. */
typedef struct SRSRAN_API {
  srsran_hip_grant_tb_t tb;  /* nof_re = nof_symb * 12 * L_prb; max_nof_iterations, llr_is_8bit unused */
  uint32_t cell_nof_prb;     /* width of the grid */
  uint32_t cp_nsymb;         /* 7 or 6 */
  uint32_t n_prb_tilde[2];   /* first PRB of the allocation in each slot */
  uint32_t L_prb;            /* srsran_dft_precoding_valid_prb */
  uint32_t shortened;        /* last symbol left to SRS */
} srsran_hip_pusch_tx_t;

/* what the reference's encoders leave, caller's HOST memory; a pointer may be NULL when its count is 0 */
typedef struct SRSRAN_API {
  const uint8_t* ack_type; /* Q_prime_ack * Qm entries: ack_ri_bits[Q_prime_ri*Qm + i].type (0, 1, 2 = repetition, 3 = placeholder) */
  const uint8_t* ri_type;  /* Q_prime_ri  * Qm entries: ack_ri_bits[i].type */
  const uint8_t* cqi_bits; /* Q_prime_cqi * Qm coded CQI bits, one bit per byte (q->temp_g_bits as srsran_uci_encode_cqi_pusch fills it) */
} srsran_hip_pusch_uci_in_t;

/* sf_symbols: the caller's subframe grid, 2 cp_nsymb x 12 cell_nof_prb points of HOST memory; only the allocation's REs are written */
SRSRAN_API int srsran_hip_pusch_encode(const srsran_hip_pusch_tx_t* g, const srsran_hip_pusch_uci_t* uci, const srsran_hip_pusch_uci_in_t* in,
                                       srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* sf_symbols);
/* the same, and what the reference leaves in the PUSCH object (each may be NULL; each costs a device -> host copy): q_out <- the byte-packed bits after
 * scrambling and the fix-up (q->q, nof_re * Qm / 8 bytes), d_out <- the nof_re constellation points (q->d), z_out <- the nof_re precoded points (q->z) */
SRSRAN_API int srsran_hip_pusch_encode_dbg(const srsran_hip_pusch_tx_t* g, const srsran_hip_pusch_uci_t* uci, const srsran_hip_pusch_uci_in_t* in,
                                           srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* sf_symbols, uint8_t* q_out, cf_t* d_out, cf_t* z_out);
/* srsran_ulsch_encode alone with control information: q_bits <- the unscrambled interleaved bits, nof_re * Qm bits byte packed, placeholder and repetition
 * bits written as 0 as the reference leaves them.  nof_symb columns, rows = nof_re / nof_symb (4 rows' worth of ACK / RI symbols at most; ACK or RI needs
 * nof_symb >= 9).  All counts 0 (or uci == NULL): byte for byte what srsran_hip_ulsch_encode gives.  Refusals as above. */
SRSRAN_API int srsran_hip_ulsch_encode_uci(const srsran_hip_grant_tb_t* tb, uint32_t nof_symb, const srsran_hip_pusch_uci_t* uci,
                                           const srsran_hip_pusch_uci_in_t* in, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, uint8_t* q_bits);

/* ---- warm start.  The first grant of a process / of a worker thread otherwise pays for loading the kernels' device code, creating the thread's staging
 * context (stream, pinned and device images, decoder / encoder objects, transform plans) and building rate-matching tables: 20-28 ms where a warm
 * call takes 0.1-0.4 ms.  srsran_hip_warmup(n) builds every rate-matching table and prepares n staging contexts by running real grants (the
 * largest of a 100-PRB cell, a one-block and a scalar-decoder one; receive and transmit side; 16- and 8-bit soft bits, one CSI-weighted grant of each width;
 * one 2-port transmit-diversity grant and one two-codeword spatial-multiplexing grant each way, one PDSCH grant from the subframe grids, one PUSCH transmit
 * grant with control information) on
 * short-lived threads; a worker
 * thread adopts a prepared context at its first call.  srsran_rm_turbo_gentables() -- which srsran_sch_init calls (sch.c:166) -- does the same
 * for one worker, so an application that does nothing gets a warm first subframe on one thread; srsenb's pool of nof_phy_threads workers
 * wants srsran_hip_warmup(nof_phy_threads) once after its objects are created.  Idempotent; returns SRSRAN_ERROR without a device. */
SRSRAN_API int srsran_hip_warmup(uint32_t nof_workers);

/* modulator alone: srsran_mod_modulate_bytes (mod.c:135-166) of byte-packed bits with the tables of lte_tables.c, optional scrambling in front
 * (srsran_sequence_apply_pack) and scaling behind; HOST buffers.  Returns the number of symbols or -1. */
SRSRAN_API int srsran_hip_modulate_bytes(uint32_t mod, const uint8_t* bits, cf_t* symbols, uint32_t nbits, uint32_t seed, uint32_t scramble, float scaling);

#ifdef __cplusplus
}
#endif
#endif
