/* chest_ul_ref_wrap.c -- the one exported wrapper tools/gen_golden_chest_ul.py calls.  The reference's chest_ul.c is included where it lies (REF_CHEST_UL_C:
 * its path, given on the compiler's command line; nothing of it is copied or committed) and the wrapper fills the fields srsran_chest_ul_estimate_pusch
 * reads: cell, dmrs_signal.cell, dmrs_signal_configured, the three work buffers, the smoothing filter and ONE entry of the pregenerated DMRS table,
 * dmrs_pregen.r[0][0], pointing to a table whose [L_prb] is the case's r.  No init and no pregen is needed.  Built into a temporary directory with the
 * reference flags of oracle/Makefile, together with the reference files the call binds into, and loaded lazily. */
#include REF_CHEST_UL_C

/* out6: noise_estimate, noise_estimate_dbm, snr, snr_db, cfo_hz, ta_us.  input, ce: grids of 2 cp_nsymb x 12 nof_prb points */
int chest_ul_ref(uint32_t nof_prb, int cp_ext, uint32_t n_prb, uint32_t L_prb, uint32_t filter_len, const float* filter, int meas_ta_en, cf_t* r, cf_t* input,
                 cf_t* ce, float* out6)
{
  srsran_chest_ul_t     q;
  srsran_ul_sf_cfg_t    sf;
  srsran_pusch_cfg_t    cfg;
  srsran_chest_ul_res_t res;
  const uint32_t        n = 2 * 12 * L_prb;
  memset(&q, 0, sizeof(q));
  memset(&sf, 0, sizeof(sf));
  memset(&cfg, 0, sizeof(cfg));
  memset(&res, 0, sizeof(res));
  q.cell.nof_prb           = nof_prb;
  q.cell.cp                = cp_ext ? SRSRAN_CP_EXT : SRSRAN_CP_NORM;
  q.dmrs_signal.cell       = q.cell;
  q.dmrs_signal_configured = true;
  q.pilot_estimates        = srsran_vec_cf_malloc(n);
  q.pilot_recv_signal      = srsran_vec_cf_malloc(n);
  q.tmp_noise              = srsran_vec_cf_malloc(n);
  cf_t** table             = calloc(L_prb + 1, sizeof(cf_t*));
  if (!q.pilot_estimates || !q.pilot_recv_signal || !q.tmp_noise || !table || filter_len > SRSRAN_CHEST_MAX_SMOOTH_FIL_LEN) {
    return -100;
  }
  table[L_prb]         = r;
  q.dmrs_pregen.r[0][0] = table;
  q.smooth_filter_len  = filter_len;
  for (uint32_t i = 0; i < filter_len; i++) {
    q.smooth_filter[i] = filter[i];
  }
  cfg.grant.L_prb          = L_prb;
  cfg.grant.n_prb[0]       = n_prb;
  cfg.grant.n_prb[1]       = n_prb;
  cfg.grant.n_prb_tilde[0] = n_prb;
  cfg.grant.n_prb_tilde[1] = n_prb;
  cfg.grant.n_dmrs         = 0;
  cfg.meas_ta_en           = meas_ta_en != 0;
  sf.tti                   = 0;
  res.ce                   = ce;
  int rc  = srsran_chest_ul_estimate_pusch(&q, &sf, &cfg, input, &res);
  out6[0] = res.noise_estimate;
  out6[1] = res.noise_estimate_dbm;
  out6[2] = res.snr;
  out6[3] = res.snr_db;
  out6[4] = res.cfo_hz;
  out6[5] = res.ta_us;
  free(q.pilot_estimates);
  free(q.pilot_recv_signal);
  free(q.tmp_noise);
  free(table);
  return rc;
}
