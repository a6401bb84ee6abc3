/* pusch_tx_ref_wrap.c -- the one exported wrapper tools/gen_golden_pusch_tx.py calls: the reference's srsran_ulsch_encode on one grant.  The reference's sch.c is
 * included where it lies (REF_SCH_C: its path, given on the compiler's command line; nothing of it is copied or committed) so that the wrapper reaches its
 * static offset tables; uci.c, cqi.c, the block and convolutional coders and softbuffer.c are compiled beside it from the reference tree.  Built into a temporary
 * directory with the reference flags of oracle/Makefile and loaded lazily behind oracle/_ref/libsrsran_ref.so. */
#include REF_SCH_C

/* cqi_kind: 0 none, 1 wideband (4 bits: block code), 2 higher-layer subband with N = 5 (14 bits: CRC + convolutional code).
 * Outputs: q_bits = srsran_ulsch_encode's packed bits; scr_bits = srsran_sequence_pusch_apply_pack of them; pos / type = the ack_ri_bits list (RI first);
 * counts = {Q'ack, Q'ri, Q'cqi}; cqi_coded = the Q'cqi Qm coded CQI bits, one per byte.  Returns the number of list entries or < 0. */
int pusch_tx_ref(int mod, int tbs, int rv, unsigned L_prb, unsigned nof_symb, unsigned nof_ack, const uint8_t* ack, unsigned N_bundle, unsigned ri_len, unsigned ri,
                 int cqi_kind, unsigned cqi_value, unsigned I_ack, unsigned I_ri, unsigned I_cqi, unsigned rnti, unsigned tti, unsigned cell_id, uint8_t* payload,
                 uint8_t* q_bits, uint8_t* scr_bits, uint32_t* pos, uint8_t* type, uint32_t* counts, uint8_t* cqi_coded)
{
  static srsran_sch_t    q;
  static uint8_t         g_bits[200000];
  static srsran_uci_bit_t tmp_bits[57600];
  srsran_pusch_cfg_t     cfg;
  srsran_uci_value_t     uv;
  srsran_softbuffer_tx_t sb;
  int                    ret = -1;
  memset(&cfg, 0, sizeof(cfg));
  memset(&uv, 0, sizeof(uv));
  if (srsran_sch_init(&q)) {
    return -10;
  }
  if (srsran_softbuffer_tx_init_guru(&sb, 16, 18600)) {
    return -11;
  }
  const uint32_t Qm     = srsran_mod_bits_x_symbol((srsran_mod_t)mod);
  cfg.grant.L_prb       = L_prb;
  cfg.grant.nof_symb    = nof_symb;
  cfg.grant.nof_re      = nof_symb * 12 * L_prb;
  cfg.grant.tb.mod      = (srsran_mod_t)mod;
  cfg.grant.tb.tbs      = tbs;
  cfg.grant.tb.nof_bits = cfg.grant.nof_re * Qm;
  cfg.softbuffers.tx    = &sb;
  cfg.uci_offset.I_offset_ack = I_ack;
  cfg.uci_offset.I_offset_ri  = I_ri;
  cfg.uci_offset.I_offset_cqi = I_cqi;
  cfg.uci_cfg.ack[0].nof_acks = nof_ack;
  cfg.uci_cfg.ack[0].N_bundle = N_bundle;
  cfg.uci_cfg.cqi.ri_len      = ri_len;
  uv.ri                       = (uint8_t)ri;
  for (unsigned i = 0; i < nof_ack; i++) {
    uv.ack.ack_value[i] = ack[i];
  }
  if (cqi_kind == 1) {
    cfg.uci_cfg.cqi.data_enable = true;
    cfg.uci_cfg.cqi.type        = SRSRAN_CQI_TYPE_WIDEBAND;
    uv.cqi.wideband.wideband_cqi = (uint8_t)(cqi_value & 15u);
  } else if (cqi_kind == 2) {
    cfg.uci_cfg.cqi.data_enable = true;
    cfg.uci_cfg.cqi.type        = SRSRAN_CQI_TYPE_SUBBAND_HL;
    cfg.uci_cfg.cqi.N           = 5;
    uv.cqi.subband_hl.wideband_cqi_cw0     = (uint8_t)(cqi_value & 15u);
    uv.cqi.subband_hl.subband_diff_cqi_cw0 = (cqi_value >> 4) & 1023u;
  }
  const uint32_t nbytes = cfg.grant.tb.nof_bits / 8;
  /* rm_turbo.c fills the circular buffer at rv 0 only: a later redundancy version follows a first transmission on the same soft buffer */
  for (int pass = (rv == 0) ? 1 : 0; pass < 2; pass++) {
    cfg.grant.tb.rv = pass ? rv : 0;
    memset(q_bits, 0, nbytes); /* pusch.c:299 */
    memset(g_bits, 0, sizeof(g_bits));
    ret = srsran_ulsch_encode(&q, &cfg, payload, &uv, g_bits, q_bits);
    if (ret < 0) {
      return ret;
    }
  }
  for (int i = 0; i < ret; i++) {
    pos[i]  = q.ack_ri_bits[i].position;
    type[i] = (uint8_t)q.ack_ri_bits[i].type;
  }
  /* the counts srsran_ulsch_encode keeps to itself: the same two encoders again, on scratch (cfg.K_segm was set by the call above) */
  uint8_t cqi_buff[SRSRAN_CQI_MAX_BITS];
  memset(cqi_buff, 0, sizeof(cqi_buff));
  int cqi_len = cfg.uci_cfg.cqi.data_enable ? srsran_cqi_value_pack(&cfg.uci_cfg.cqi, &uv.cqi, cqi_buff) : 0;
  int Qri = 0, Qcqi = 0;
  if (ri_len > 0) {
    uint8_t r[2] = {uv.ri, 0};
    Qri = srsran_uci_encode_ack_ri(&cfg, r, ri_len, (uint32_t)cqi_len, get_beta_ri_offset(I_ri), cfg.grant.nof_re, true, N_bundle, tmp_bits);
  }
  if (cqi_len > 0) {
    Qcqi = srsran_uci_encode_cqi_pusch(&q.uci_cqi, &cfg, cqi_buff, (uint32_t)cqi_len, get_beta_cqi_offset(I_cqi), (uint32_t)Qri, cqi_coded);
  }
  if (Qri < 0 || Qcqi < 0) {
    return -12;
  }
  counts[0] = (uint32_t)ret / Qm - (uint32_t)Qri;
  counts[1] = (uint32_t)Qri;
  counts[2] = (uint32_t)Qcqi;
  srsran_sequence_pusch_apply_pack(q_bits, scr_bits, (uint16_t)rnti, 2 * (tti % 10), cell_id, cfg.grant.tb.nof_bits);
  srsran_softbuffer_tx_free(&sb);
  srsran_sch_free(&q);
  return ret;
}
