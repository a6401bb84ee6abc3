/* chest_dl_ref_wrap.c -- the one exported wrapper tools/gen_golden_chest_dl.py calls.  The reference's chest_dl.c is included where it lies (REF_CHEST_DL_C:
 * its path, given on the compiler's command line; nothing of it is copied or committed) and the wrapper fills the fields srsran_chest_dl_estimate_cfg
 * reads: cell, nof_rx_antennas, csr_refs.cell and ONE row per pilot table, csr_refs.pilots[p][sf_idx] (the case's rows: no sequence is generated), the five
 * work buffers, the three interpolators, pss_signal and the state that the object carries between subframes (noise_estimate, cfo).  No Wiener object: the
 * estimator looks at it only when it is there.  Built into a temporary directory with the reference flags of oracle/Makefile, together with the reference
 * files the call binds into, and loaded lazily. */
#include REF_CHEST_DL_C

/* cfg_u: nof_prb, nof_ports, id, cp_ext, nof_rx, sf_idx, estimator_alg, noise_alg, filter_type, rsrp_neighbour, cfo_estimate_enable, cfo_estimate_sf_mask
 * state: noise_estimate[4][4] ([rx][port]) then cfo: 17 floats in, 17 out
 * ce: 16 pointers, [port][rx] (NULL: the reference estimates nothing for that pair)
 * out: the 11 scalars of fill_res in the order of srsran_chest_dl_res_t, rsrp_port_dbm[4], snr_ant_port_db, rsrp_ant_port_dbm, rsrq_ant_port_db [4][4]
 *      each, then the object's rsrp, rssi, rsrp_corr [4][4] each: 111 floats */
int chest_dl_ref(const uint32_t* cfg_u, const float* filter_coef, const cf_t* pilots0, const cf_t* pilots1, const cf_t* pss, const float* state_in,
                 cf_t** input, cf_t** ce, float* state_out, float* out)
{
  srsran_chest_dl_t     q;
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_cfg_t cfg;
  srsran_chest_dl_res_t res;
  memset(&q, 0, sizeof(q));
  memset(&sf, 0, sizeof(sf));
  memset(&cfg, 0, sizeof(cfg));
  memset(&res, 0, sizeof(res));
  const uint32_t prb = cfg_u[0], sf_idx = cfg_u[5];
  q.cell.nof_prb     = prb;
  q.cell.nof_ports   = cfg_u[1];
  q.cell.id          = cfg_u[2];
  q.cell.cp          = cfg_u[3] ? SRSRAN_CP_EXT : SRSRAN_CP_NORM;
  q.cell.frame_type  = SRSRAN_FDD;
  q.nof_rx_antennas  = cfg_u[4];
  q.csr_refs.cell    = q.cell;
  q.csr_refs.pilots[0][sf_idx] = (cf_t*)pilots0;
  q.csr_refs.pilots[1][sf_idx] = (cf_t*)pilots1;
  q.tmp_noise               = srsran_vec_cf_malloc(20 * prb);
  q.tmp_cfo_estimate        = srsran_vec_cf_malloc(20 * prb);
  q.pilot_estimates         = srsran_vec_cf_malloc(20 * prb);
  q.pilot_estimates_average = srsran_vec_cf_malloc(20 * prb);
  q.pilot_recv_signal       = srsran_vec_cf_malloc(20 * prb);
  if (!q.tmp_noise || !q.tmp_cfo_estimate || !q.pilot_estimates || !q.pilot_estimates_average || !q.pilot_recv_signal ||
      srsran_interp_linear_vector_init(&q.srsran_interp_linvec, SRSRAN_NRE * prb) || srsran_interp_linear_init(&q.srsran_interp_lin, 2 * prb, SRSRAN_NRE / 2) ||
      srsran_interp_linear_init(&q.srsran_interp_lin_3, 4 * prb, SRSRAN_NRE / 4)) {
    return -100;
  }
  if (pss) {
    memcpy(q.pss_signal, pss, sizeof(q.pss_signal));
  }
  memcpy(q.noise_estimate, state_in, sizeof(q.noise_estimate));
  q.cfo  = state_in[16];
  sf.tti = sf_idx;
  sf.sf_type = SRSRAN_SF_NORM;
  cfg.estimator_alg        = (srsran_chest_dl_estimator_alg_t)cfg_u[6];
  cfg.noise_alg            = (srsran_chest_dl_noise_alg_t)cfg_u[7];
  cfg.filter_type          = (srsran_chest_filter_t)cfg_u[8];
  cfg.filter_coef[0]       = filter_coef[0];
  cfg.filter_coef[1]       = filter_coef[1];
  cfg.rsrp_neighbour       = cfg_u[9] != 0;
  cfg.cfo_estimate_enable  = cfg_u[10] != 0;
  cfg.cfo_estimate_sf_mask = cfg_u[11];
  for (int p = 0; p < SRSRAN_MAX_PORTS; p++) {
    for (int a = 0; a < SRSRAN_MAX_PORTS; a++) {
      res.ce[p][a] = ce[p * SRSRAN_MAX_PORTS + a];
    }
  }
  int rc = srsran_chest_dl_estimate_cfg(&q, &sf, &cfg, input, &res);
  memcpy(state_out, q.noise_estimate, sizeof(q.noise_estimate));
  state_out[16] = q.cfo;
  float* o = out;
  *o++ = res.noise_estimate;
  *o++ = res.noise_estimate_dbm;
  *o++ = res.snr_db;
  *o++ = res.rsrp;
  *o++ = res.rsrp_dbm;
  *o++ = res.rsrp_neigh;
  *o++ = res.rsrq;
  *o++ = res.rsrq_db;
  *o++ = res.rssi_dbm;
  *o++ = res.cfo;
  *o++ = res.sync_error;
  memcpy(o, res.rsrp_port_dbm, sizeof(res.rsrp_port_dbm));
  o += 4;
  memcpy(o, res.snr_ant_port_db, 16 * sizeof(float));
  o += 16;
  memcpy(o, res.rsrp_ant_port_dbm, 16 * sizeof(float));
  o += 16;
  memcpy(o, res.rsrq_ant_port_db, 16 * sizeof(float));
  o += 16;
  memcpy(o, q.rsrp, 16 * sizeof(float));
  o += 16;
  memcpy(o, q.rssi, 16 * sizeof(float));
  o += 16;
  memcpy(o, q.rsrp_corr, 16 * sizeof(float));
  srsran_interp_linear_vector_free(&q.srsran_interp_linvec);
  srsran_interp_linear_free(&q.srsran_interp_lin);
  srsran_interp_linear_free(&q.srsran_interp_lin_3);
  free(q.tmp_noise);
  free(q.tmp_cfo_estimate);
  free(q.pilot_estimates);
  free(q.pilot_estimates_average);
  free(q.pilot_recv_signal);
  return rc;
}
