/* tests/ref_link/uci_bind.c -- chan_bind.c plus PUSCH grants that carry control information.
 *
 * Compiled against the REFERENCE's headers like chan_bind.c, and in its place: the four bindings of chan_bind.c are taken over unchanged (the file is
 * included, its srsran_pusch_decode under another name) and srsran_pusch_decode below sends a grant with HARQ-ACK / RI / CQI bits through
 * srsran_hip_pusch_decode_uci: ONE device call that returns the payload and the few soft bits of the control fields, on which the REFERENCE's own
 * decoders run (srsran_uci_decode_ack_ri, srsran_uci_decode_cqi_pusch, srsran_cqi_value_unpack: uci.c, unmodified, in the link).  Everything else goes
 * where chan_bind.c sends it. */
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "srsran/phy/ch_estimation/chest_ul.h"
#include "srsran/phy/mimo/layermap.h"
#include "srsran/phy/mimo/precoding.h"
#include "srsran/phy/phch/cqi.h"
#include "srsran/phy/phch/pdsch.h"
#include "srsran/phy/phch/pusch.h"
#include "srsran/phy/phch/sch.h"
#include "srsran/phy/phch/uci.h"
#include "srsran/phy/utils/debug.h"
#include "srsran/phy/utils/vector.h"

#define srsran_pusch_decode srsran_pusch_decode_chan /* (the reference's headers are in: only chan_bind.c's definition takes the other name) */
#include "chan_bind.c"
#undef srsran_pusch_decode

/* include/srsran_amd/phy_chan_abi.h, by hand as in chan_bind.c */
typedef struct {
  uint32_t Q_prime_ack, Q_prime_ri, Q_prime_cqi;
} srsran_hip_pusch_uci_t;
typedef struct {
  int16_t*  ack_llr;
  uint8_t*  ack_c;
  uint32_t* ack_pos;
  int16_t*  ri_llr;
  uint8_t*  ri_c;
  uint32_t* ri_pos;
  int16_t*  cqi_llr;
} srsran_hip_pusch_uci_out_t;
extern int srsran_hip_pusch_decode_uci(const srsran_hip_pusch_rx_t*, const srsran_hip_pusch_uci_t*, const cf_t*, const cf_t*, srsran_softbuffer_rx_t*, uint8_t*,
                                       srsran_hip_grant_res_t*, srsran_hip_pusch_uci_out_t*);

/* TS 36.213 tables 8.6.3-1 / -2 / -3: the offset values beta an index signalled by higher layers stands for (negative: reserved), and what sch.c:42-87
 * does with an index outside the table (the first valid entry) */
static float beta_ack_of(uint32_t idx)
{
  static const float t[16] = {2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.25f, 8.0f, 10.0f, 12.625f, 15.875f, 20.0f, 31.0f, 50.0f, 80.0f, 126.0f, -1.0f};
  return idx < 15 ? t[idx] : t[0];
}
static float beta_ri_of(uint32_t idx)
{
  static const float t[16] = {1.25f, 1.625f, 2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.25f, 8.0f, 10.0f, 12.625f, 15.875f, 20.0f, -1.0f, -1.0f, -1.0f};
  return idx < 13 ? t[idx] : t[0];
}
static float beta_cqi_of(uint32_t idx)
{
  static const float t[16] = {-1.0f, -1.0f, 1.125f, 1.25f, 1.375f, 1.625f, 1.75f, 2.0f, 2.25f, 2.5f, 2.875f, 3.125f, 3.5f, 4.0f, 5.0f, 6.25f};
  return (idx > 1 && idx < 16) ? t[idx] : t[2];
}

/* TS 36.212 5.2.2.6: coded modulation symbols of the CQI code word of O bits (uci.c:173-188 computes the same; with a transport block, K = K_segm > 0) */
static uint32_t q_prime_cqi_of(const srsran_pusch_cfg_t* cfg, uint32_t O, float beta, uint32_t Q_prime_ri)
{
  const uint32_t L = O < 11 ? 0 : 8, all = cfg->grant.L_prb * SRSRAN_NRE * cfg->grant.nof_symb;
  const uint32_t x = (uint32_t)ceilf((float)(O + L) * cfg->grant.L_prb * SRSRAN_NRE * cfg->grant.nof_symb * beta / cfg->K_segm);
  return SRSRAN_MIN(x, all - Q_prime_ri);
}

/* ---- pusch.c:358 */
int srsran_pusch_decode(srsran_pusch_t* q, srsran_ul_sf_cfg_t* sf, srsran_pusch_cfg_t* cfg, srsran_chest_ul_res_t* channel, cf_t* sf_symbols, srsran_pusch_res_t* out)
{
  if (!q || !sf_symbols || !out || !cfg || !sf || !channel) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const bool     evm     = cfg->meas_evm_en && q->evm_buffer;
  const uint32_t nof_ack = srsran_uci_cfg_total_ack(&cfg->uci_cfg), ri_len = cfg->uci_cfg.cqi.ri_len;
  const bool     cqi_en  = cfg->uci_cfg.cqi.data_enable;
  /* the length of a higher-layer sub-band report depends on the RI that is decoded from this very grant (sch.c:1111-1116): its Q' is not known up front */
  const bool  cqi_after_ri = cqi_en && cfg->uci_cfg.cqi.type == SRSRAN_CQI_TYPE_SUBBAND_HL && ri_len;
  const float b_ack = beta_ack_of(cfg->uci_offset.I_offset_ack), b_ri = beta_ri_of(cfg->uci_offset.I_offset_ri), b_cqi = beta_cqi_of(cfg->uci_offset.I_offset_cqi);
  srsran_cbsegm_t seg;
  if (!has_uci(cfg) || cfg->grant.tb.tbs <= 0 || evm || !cfg->softbuffers.rx || !out->data || q->llr_is_8bit || cqi_after_ri || (nof_ack && b_ack < 0) ||
      (ri_len && b_ri < 0) || (cqi_en && b_cqi < 0) || srsran_cbsegm(&seg, (uint32_t)cfg->grant.tb.tbs) != SRSRAN_SUCCESS) {
    return srsran_pusch_decode_chan(q, sf, cfg, channel, sf_symbols, out);
  }
  count(0, true);
  struct timeval t0;
  if (cfg->meas_time_en) {
    gettimeofday(&t0, NULL);
  }
  if (!cfg->enable_64qam && cfg->grant.tb.mod >= SRSRAN_MOD_64QAM) { /* pusch.c:374-380 */
    cfg->grant.tb.mod      = SRSRAN_MOD_16QAM;
    cfg->grant.tb.nof_bits = cfg->grant.nof_re * srsran_mod_bits_x_symbol(SRSRAN_MOD_16QAM);
  }
  const uint32_t Qm = srsran_mod_bits_x_symbol(cfg->grant.tb.mod), nof_re = cfg->grant.nof_re;
  cfg->K_segm       = seg.C1 * seg.K1 + seg.C2 * seg.K2; /* sch.c:1141 */
  /* the three counts (uci.c:418-446 through its public face; uci.c:173-188) */
  const uint32_t         cqi_len = srsran_cqi_size(&cfg->uci_cfg.cqi);
  srsran_hip_pusch_uci_t u       = {0, 0, 0};
  if (nof_ack) {
    u.Q_prime_ack = srsran_qprime_ack_ext(cfg->grant.L_prb, cfg->grant.nof_symb, cfg->K_segm, nof_ack, b_ack);
  }
  if (ri_len) {
    u.Q_prime_ri = srsran_qprime_ack_ext(cfg->grant.L_prb, cfg->grant.nof_symb, cfg->K_segm, ri_len, b_ri);
  }
  if (cqi_en) {
    u.Q_prime_cqi = q_prime_cqi_of(cfg, cqi_len, b_cqi, u.Q_prime_ri);
  }
  const uint32_t        nslot = 2 * (sf->tti % SRSRAN_NOF_SF_X_FRAME);
  srsran_hip_pusch_rx_t g     = {.tb             = {.mod                = (uint32_t)cfg->grant.tb.mod,
                                                    .tbs                = (uint32_t)cfg->grant.tb.tbs,
                                                    .rv                 = (uint32_t)cfg->grant.tb.rv,
                                                    .nof_re             = nof_re,
                                                    .seed               = srsran_hip_sequence_pusch_seed(cfg->rnti, nslot, q->cell.id),
                                                    .max_nof_iterations = 0, /* below */
                                                    .llr_is_8bit        = 0,
                                                    .nl                 = 1},
                                 .cell_nof_prb   = q->cell.nof_prb,
                                 .cp_nsymb       = SRSRAN_CP_NSYMB(q->cell.cp),
                                 .n_prb_tilde    = {cfg->grant.n_prb_tilde[0], cfg->grant.n_prb_tilde[1]},
                                 .L_prb          = cfg->grant.L_prb,
                                 .shortened      = sf->shortened,
                                 .noise_estimate = channel->noise_estimate,
                                 .meas_epre      = cfg->meas_epre_en};
  srsran_sch_set_max_noi(&q->ul_sch, cfg->max_nof_iterations); /* :450 */
  g.tb.max_nof_iterations = q->ul_sch.max_iterations;
  /* where the control soft bits come down: one allocation, [ack | ri] x (soft bit, position, chip) and the CQI soft bits */
  const size_t n_ar = (size_t)(u.Q_prime_ack + u.Q_prime_ri) * Qm, n_a = (size_t)u.Q_prime_ack * Qm, n_c = (size_t)u.Q_prime_cqi * Qm;
  uint32_t*    pos  = malloc((n_ar + 1) * (sizeof(uint32_t) + sizeof(int16_t) + 1) + (n_c + 1) * sizeof(int16_t));
  if (!pos) {
    return SRSRAN_ERROR;
  }
  int16_t*                   llr   = (int16_t*)(pos + n_ar + 1);
  int16_t*                   cqi   = llr + n_ar + 1;
  uint8_t*                   chips = (uint8_t*)(cqi + n_c + 1);
  srsran_hip_pusch_uci_out_t o     = {llr, chips, pos, llr + n_a, chips + n_a, pos + n_a, cqi};
  srsran_hip_grant_res_t     r;
  int                        ret = SRSRAN_ERROR;
  if (srsran_hip_pusch_decode_uci(&g, &u, sf_symbols, channel->ce, cfg->softbuffers.rx, out->data, &r, &o) != SRSRAN_SUCCESS) {
    goto done;
  }
  /* the soft bits and chips back at their positions in the object's own (otherwise unused) buffers: what the reference's decoders index */
  int16_t* q_bits = (int16_t*)q->q;
  uint8_t* c_seq  = (uint8_t*)q->z; /* pusch.c:445 */
  for (size_t i = 0; i < n_ar; i++) {
    q_bits[pos[i]] = llr[i];
    c_seq[pos[i]] = chips[i];
  }
  /* sch.c:1041-1046,1050-1116 (uci_decode_ri_ack) on them; each decoder returns the Q' it computed */
  if (cqi_en && cfg->uci_cfg.cqi.type == SRSRAN_CQI_TYPE_SUBBAND_HL && ri_len) {
    cfg->uci_cfg.cqi.rank_is_not_one = false;
  }
  if (nof_ack) {
    const int k = srsran_uci_decode_ack_ri(cfg, q_bits, c_seq, b_ack, nof_re, cqi_len, q->ul_sch.ack_ri_bits, out->uci.ack.ack_value, &out->uci.ack.valid, nof_ack, false);
    if (k < 0 || (uint32_t)k != u.Q_prime_ack) {
      ERROR("uci_bind: Q'ack %u passed to the device, the decoder computed %d", u.Q_prime_ack, k);
      goto done;
    }
  }
  if (ri_len) {
    const int k = srsran_uci_decode_ack_ri(cfg, q_bits, c_seq, b_ri, nof_re, cqi_len, q->ul_sch.ack_ri_bits, &out->uci.ri, NULL, ri_len, true);
    if (k < 0 || (uint32_t)k != u.Q_prime_ri) {
      ERROR("uci_bind: Q'ri %u passed to the device, the decoder computed %d", u.Q_prime_ri, k);
      goto done;
    }
  }
  if (cqi_en && cfg->uci_cfg.cqi.type == SRSRAN_CQI_TYPE_SUBBAND_HL && ri_len) {
    cfg->uci_cfg.cqi.rank_is_not_one = out->uci.ri > 0;
  }
  if (cqi_en) { /* sch.c:1165-1182 */
    uint8_t cqi_buff[SRSRAN_CQI_MAX_BITS];
    memset(cqi_buff, 0, sizeof(cqi_buff));
    const int k = srsran_uci_decode_cqi_pusch(&q->ul_sch.uci_cqi, cfg, cqi, b_cqi, u.Q_prime_ri, cqi_len, cqi_buff, &out->uci.cqi.data_crc);
    if (k < 0 || (uint32_t)k != u.Q_prime_cqi) {
      ERROR("uci_bind: Q'cqi %u passed to the device, the decoder computed %d", u.Q_prime_cqi, k);
      goto done;
    }
    srsran_cqi_value_unpack(&cfg->uci_cfg.cqi, cqi_buff, &out->uci.cqi);
  }
  out->crc                  = r.crc_ok != 0;
  out->avg_iterations_block = r.avg_iterations_block;
  q->ul_sch.avg_iterations  = r.avg_iterations_block;
  out->epre_dbfs            = cfg->meas_epre_en ? srsran_convert_power_to_dB(r.epre) : NAN;
  out->evm                  = NAN;
  cfg->last_O_cqi           = cqi_len; /* :460 */
  if (cfg->meas_time_en) {
    cfg->meas_time_value = elapsed_us(&t0);
  }
  ret = SRSRAN_SUCCESS;
done:
  free(pos);
  return ret;
}
