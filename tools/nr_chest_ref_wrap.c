/* nr_chest_ref_wrap.c -- the one exported wrapper tools/gen_golden_nr_chest.py calls.  The reference's dmrs_sch.c is included where it lies (REF_DMRS_SCH_C:
 * its path, given on the compiler's command line; nothing of it is copied or committed).  The wrapper fills the carrier, the configuration and the grant
 * from plain arguments, runs srsran_dmrs_sch_init / _set_carrier / srsran_dmrs_sch_get_symbols_idx / srsran_dmrs_sch_estimate and hands back what they
 * leave.  Built into a temporary directory with the reference flags of oracle/Makefile, together with the reference files the calls bind into, and loaded
 * lazily. */
#include REF_DMRS_SCH_C

/* cfg: nof_prb, scs, slot_idx, S, L, dmrs_type, typeA_pos, additional_pos, length, n_id, n_scid, cdm groups, nof_rvd
 * rvd: nof_rvd x (rb_begin, rb_end, rb_stride, sc mask, symbol mask); prb: nof_prb flags; grid: 14 x 12 nof_prb points
 * ce: room for 14 x 12 nof_prb points; out8: noise_estimate, noise_estimate_dbm, rsrp, rsrp_dbm, snr_db, cfo, sync_error, nof_re;
 * sym5: the count srsran_dmrs_sch_get_symbols_idx returns and its (at most 4) symbols */
int nr_chest_ref(const uint32_t* cfg, float beta_dmrs, const uint32_t* rvd, const uint8_t* prb, cf_t* grid, cf_t* ce, float* out8, int32_t* sym5)
{
  srsran_dmrs_sch_t     q;
  srsran_carrier_nr_t   carrier;
  srsran_slot_cfg_t     slot;
  srsran_sch_cfg_nr_t   sch;
  srsran_chest_dl_res_t res;
  memset(&carrier, 0, sizeof(carrier));
  memset(&slot, 0, sizeof(slot));
  memset(&sch, 0, sizeof(sch));
  memset(&res, 0, sizeof(res));
  carrier.nof_prb = cfg[0];
  carrier.scs     = (srsran_subcarrier_spacing_t)cfg[1];
  carrier.pci     = cfg[9];
  carrier.max_mimo_layers = 1;
  slot.idx        = cfg[2];
  srsran_sch_grant_nr_t* grant = &sch.grant;
  grant->mapping = srsran_sch_mapping_type_A;
  grant->S       = cfg[3];
  grant->L       = cfg[4];
  grant->n_scid  = cfg[10];
  grant->beta_dmrs = beta_dmrs;
  grant->nof_layers = 1;
  grant->nof_dmrs_cdm_groups_without_data = cfg[11];
  for (uint32_t i = 0; i < cfg[0]; i++) {
    grant->prb_idx[i] = prb[i] != 0;
  }
  sch.dmrs.type           = cfg[5] ? srsran_dmrs_sch_type_2 : srsran_dmrs_sch_type_1;
  sch.dmrs.typeA_pos      = cfg[6] == 3 ? srsran_dmrs_sch_typeA_pos_3 : srsran_dmrs_sch_typeA_pos_2;
  sch.dmrs.additional_pos = cfg[7] == 0 ? srsran_dmrs_sch_add_pos_0 : cfg[7] == 1 ? srsran_dmrs_sch_add_pos_1 : cfg[7] == 2 ? srsran_dmrs_sch_add_pos_2 : srsran_dmrs_sch_add_pos_3;
  sch.dmrs.length         = cfg[8] == 2 ? srsran_dmrs_sch_len_2 : srsran_dmrs_sch_len_1;
  sch.rvd_re.count        = cfg[12];
  for (uint32_t i = 0; i < cfg[12]; i++) {
    srsran_re_pattern_t* p = &sch.rvd_re.data[i];
    p->rb_begin = rvd[5 * i], p->rb_end = rvd[5 * i + 1], p->rb_stride = rvd[5 * i + 2];
    for (uint32_t k = 0; k < SRSRAN_NRE; k++) {
      p->sc[k] = (rvd[5 * i + 3] >> k) & 1u;
    }
    for (uint32_t l = 0; l < SRSRAN_NSYMB_PER_SLOT_NR; l++) {
      p->symbol[l] = (rvd[5 * i + 4] >> l) & 1u;
    }
  }
  uint32_t symbols[SRSRAN_DMRS_SCH_MAX_SYMBOLS] = {0, 0, 0, 0};
  sym5[0] = srsran_dmrs_sch_get_symbols_idx(&sch.dmrs, grant, symbols);
  for (int i = 0; i < SRSRAN_DMRS_SCH_MAX_SYMBOLS; i++) {
    sym5[1 + i] = (int32_t)symbols[i];
  }
  if (srsran_dmrs_sch_init(&q, true) < SRSRAN_SUCCESS || srsran_dmrs_sch_set_carrier(&q, &carrier) < SRSRAN_SUCCESS) {
    return -100;
  }
  res.ce[0][0] = ce;
  int rc  = srsran_dmrs_sch_estimate(&q, &slot, &sch, grant, grid, &res);
  out8[0] = res.noise_estimate;
  out8[1] = res.noise_estimate_dbm;
  out8[2] = res.rsrp;
  out8[3] = res.rsrp_dbm;
  out8[4] = res.snr_db;
  out8[5] = res.cfo;
  out8[6] = res.sync_error;
  out8[7] = (float)res.nof_re;
  srsran_dmrs_sch_free(&q);
  return rc;
}
