/* pucch_ref_wrap.c -- the exported wrappers tools/gen_golden_pucch.py calls.  The reference's pucch.c is included where it lies (REF_PUCCH_C: its path, given
 * on the compiler's command line), so that its static stages (encode_signal, pucch_put, get_N_sf, get_pucch_symbol) can be called; chest_ul.c and the other
 * reference files the calls bind into are compiled beside it, where they lie, with the reference flags of oracle/Makefile, into a temporary directory:
 * nothing of the reference is copied or committed.  The estimator object is filled field by field as tools/chest_ul_ref_wrap.c does (no init: the PUSCH
 * tables and the interpolator are not needed); its DMRS object and the PUCCH object go through the reference's own set_cell. */
#include REF_PUCCH_C

#include "srsran/phy/ch_estimation/chest_ul.h"
#include "srsran/phy/common/zc_sequence.h"

#include <stdlib.h>
#include <string.h>

static srsran_pucch_t    pucch;
static srsran_chest_ul_t est;
static srsran_cell_t     cell;
static int               is_open;

void pucch_ref_close(void)
{
  if (is_open) {
    srsran_pucch_free(&pucch);
    free(est.pilot_estimates);
    free(est.pilot_recv_signal);
    free(est.pilot_known_signal);
    free(est.tmp_noise);
    for (int i = 0; i < 4; i++) {
      free(est.pilot_estimates_tmp[i]);
    }
    is_open = 0;
  }
}

int pucch_ref_open(uint32_t nof_prb, uint32_t cp_ext, uint32_t id)
{
  const uint32_t n = 2 * 3 * 12 + 16;
  pucch_ref_close();
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb   = nof_prb;
  cell.nof_ports = 1;
  cell.id        = id;
  cell.cp        = cp_ext ? SRSRAN_CP_EXT : SRSRAN_CP_NORM;
  if (srsran_pucch_init_enb(&pucch)) {
    return -100;
  }
  memset(&est, 0, sizeof(est));
  est.cell               = cell;
  est.pilot_estimates    = srsran_vec_cf_malloc(n);
  est.pilot_recv_signal  = srsran_vec_cf_malloc(n);
  est.pilot_known_signal = srsran_vec_cf_malloc(n);
  est.tmp_noise          = srsran_vec_cf_malloc(n);
  for (int i = 0; i < 4; i++) {
    est.pilot_estimates_tmp[i] = srsran_vec_cf_malloc(n);
  }
  is_open = 1;
  if (srsran_pucch_set_cell(&pucch, cell) || srsran_refsignal_ul_set_cell(&est.dmrs_signal, cell)) {
    return -101;
  }
  est.dmrs_signal_configured = true;
  return 0;
}

/* the two tables the library takes from its caller, and the two cell sequences, as data of the run */
void pucch_ref_tables(cf_t* base, uint8_t* basis, uint32_t* n_cs_cell, uint32_t* f_gh)
{
  for (uint32_t u = 0; u < 30; u++) {
    srsran_zc_sequence_generate_lte(u, 0, 0, 1, base + 12 * u);
  }
  for (uint32_t n = 0; n < 13; n++) {
    uint8_t unit[13] = {0};
    unit[n]          = 1;
    srsran_uci_encode_cqi_pucch(unit, 13, basis + 20 * n);
  }
  memcpy(n_cs_cell, pucch.n_cs_cell, sizeof(pucch.n_cs_cell));
  memcpy(f_gh, pucch.f_gh, sizeof(pucch.f_gh));
}

/* d: format, n_pucch, N_cs, delta_pucch_shift, n_rb_2, group_hopping_en, rnti, nof_uci_bits, meas_ta_en, tti, shortened */
static void make_cfg(const uint32_t* d, srsran_pucch_cfg_t* cfg, srsran_ul_sf_cfg_t* sf)
{
  memset(cfg, 0, sizeof(*cfg));
  memset(sf, 0, sizeof(*sf));
  cfg->format             = (srsran_pucch_format_t)d[0];
  cfg->n_pucch            = (uint16_t)d[1];
  cfg->N_cs               = d[2];
  cfg->delta_pucch_shift  = d[3];
  cfg->n_rb_2             = d[4];
  cfg->group_hopping_en   = d[5] != 0;
  cfg->rnti               = (uint16_t)d[6];
  cfg->uci_cfg.cqi.ri_len = d[7]; /* nof_uci_bits = ri_len when set (pucch.c:811) */
  cfg->meas_ta_en         = d[8] != 0;
  sf->tti                 = d[9];
  sf->shortened           = d[10] != 0;
}

/* the fields of srsran_hip_pucch_plan_t, in its order (65 words), from the reference's own functions; n_prime of formats 2x is not exposed there (left 0).
 * Returns 0, or 1 for what srsran_pucch_cfg_isvalid or pucch_cp refuse. */
int pucch_ref_plan(const uint32_t* d, uint32_t* out)
{
  srsran_pucch_cfg_t cfg;
  srsran_ul_sf_cfg_t sf;
  make_cfg(d, &cfg, &sf);
  memset(out, 0, 65 * sizeof(uint32_t));
  if (!srsran_pucch_cfg_isvalid(&cfg, cell.nof_prb)) {
    return 1;
  }
  const bool f1 = cfg.format < SRSRAN_PUCCH_FORMAT_2;
  uint32_t*  n_prb = out + 1, *u = out + 3, *N_sf = out + 5, *sym = out + 7, *n_cs = out + 17, *n_oc = out + 27, *n_pr = out + 37, *dsym = out + 47, *dcs = out + 53,
            *doc = out + 59;
  out[0] = srsran_refsignal_dmrs_N_rs(cfg.format, cell.cp);
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t ns = 2 * (sf.tti % 10) + s;
    n_prb[s]          = srsran_pucch_n_prb(&cell, &cfg, s);
    if (n_prb[s] >= cell.nof_prb) {
      memset(out, 0, 65 * sizeof(uint32_t));
      return 1;
    }
    u[s]    = ((cfg.group_hopping_en ? pucch.f_gh[ns] : 0) + (cell.id % 30)) % 30;
    N_sf[s] = get_N_sf(cfg.format, s, sf.shortened);
    for (uint32_t m = 0; m < N_sf[s]; m++) {
      const uint32_t l = get_pucch_symbol(m, cfg.format, cell.cp);
      const float    a = f1 ? srsran_pucch_alpha_format1(pucch.n_cs_cell, &cfg, cell.cp, true, ns, l, &n_oc[5 * s + m], &n_pr[5 * s + m]) /* as encode_signal_format12 calls it, :419 */
                            : srsran_pucch_alpha_format2(pucch.n_cs_cell, &cfg, ns, l);
      sym[5 * s + m]   = l;
      n_cs[5 * s + m]  = (uint32_t)lroundf(a * 12 / (2 * (float)M_PI));
    }
    for (uint32_t m = 0; m < out[0]; m++) {
      const uint32_t l = srsran_refsignal_dmrs_pucch_symbol(m, cfg.format, cell.cp);
      const float    a = f1 ? srsran_pucch_alpha_format1(pucch.n_cs_cell, &cfg, cell.cp, true, ns, l, &doc[3 * s + m], NULL)
                            : srsran_pucch_alpha_format2(pucch.n_cs_cell, &cfg, ns, l);
      dsym[3 * s + m]  = l;
      dcs[3 * s + m]   = (uint32_t)lroundf(a * 12 / (2 * (float)M_PI));
    }
  }
  return 0;
}

/* The UE's signal into `grid`: the data symbols (encode_signal and pucch_put, what srsran_pucch_encode runs behind encode_bits) and the DMRS.
 * bits: formats 1A / 1B: the ACK bits; formats 2x: nof_uci_bits information bits, coded here by srsran_uci_encode_cqi_pucch.  drs: pucch2_drs_bits. */
int pucch_ref_encode(const uint32_t* d, const uint8_t* bits, const uint8_t* drs, cf_t* grid)
{
  srsran_pucch_cfg_t cfg;
  srsran_ul_sf_cfg_t sf;
  uint8_t            pucch_bits[SRSRAN_PUCCH_MAX_BITS] = {0};
  make_cfg(d, &cfg, &sf);
  cfg.pucch2_drs_bits[0] = drs[0];
  cfg.pucch2_drs_bits[1] = drs[1];
  if (cfg.format >= SRSRAN_PUCCH_FORMAT_2) {
    srsran_uci_encode_cqi_pucch((uint8_t*)bits, d[7], pucch_bits);
  } else {
    pucch_bits[0] = bits[0];
    pucch_bits[1] = bits[1];
  }
  if (encode_signal(&pucch, &sf, &cfg, pucch_bits, pucch.z) || pucch_put(&pucch, &sf, &cfg, pucch.z, grid) < 0) {
    return -1;
  }
  if (srsran_refsignal_dmrs_pucch_gen(&est.dmrs_signal, &sf, &cfg, est.pilot_known_signal) ||
      srsran_refsignal_dmrs_pucch_put(&est.dmrs_signal, &cfg, est.pilot_known_signal, grid)) {
    return -2;
  }
  return 0;
}

/* srsran_chest_ul_estimate_pucch, then srsran_pucch_decode.  filter_len: 3, or 1 with the tap {1} for "no smoothing" (the reference's length 0 zeroes the
 * estimate).  th: threshold_format1, _data_valid_format1a, _data_valid_format2, _dmrs_detection.
 * outf: detected, correlation, dmrs_correlation, ack_valid, noise_estimate, noise_estimate_dbm, snr, snr_db, rsrp, rsrp_dBfs, epre, epre_dBfs, ta_us.
 * outb: 13 pucch_bits then 2 drs bits.  For formats 2x the soft bits, the word and max_corr are local to decode_signal: the three reference calls of
 * pucch.c:702-710 are run again HERE on the symbol averages decode_signal left in q->z[0 .. 9].  z: q->z after the decode (formats 2x: entries 0 .. 9 are
 * those averages, the rest the equalised symbols).  pe: 2 n_rs rows of pilot_estimates after the in-place average.  Returns 0, or the reference's error. */
int pucch_ref_decode(const uint32_t* d, uint32_t filter_len, const float* filter, const float* th, cf_t* grid, cf_t* ce, float* outf, uint8_t* outb, cf_t* z,
                     int16_t* llr, cf_t* pe, int32_t* max_corr)
{
  srsran_pucch_cfg_t    cfg;
  srsran_ul_sf_cfg_t    sf;
  srsran_chest_ul_res_t res;
  srsran_pucch_res_t    data;
  make_cfg(d, &cfg, &sf);
  memset(&res, 0, sizeof(res));
  memset(&data, 0, sizeof(data));
  cfg.threshold_format1             = th[0];
  cfg.threshold_data_valid_format1a = th[1];
  cfg.threshold_data_valid_format2  = th[2];
  cfg.threshold_dmrs_detection      = th[3];
  est.smooth_filter_len             = filter_len;
  for (uint32_t i = 0; i < filter_len; i++) {
    est.smooth_filter[i] = filter[i];
  }
  res.ce = ce;
  memset(pucch.z, 0, SRSRAN_PUCCH_MAX_SYMBOLS * sizeof(cf_t));
  int rc = srsran_chest_ul_estimate_pucch(&est, &sf, &cfg, grid, &res);
  if (rc) {
    return rc;
  }
  const uint32_t n_rs = srsran_refsignal_dmrs_N_rs(cfg.format, cell.cp);
  memcpy(pe, est.pilot_estimates, 2 * n_rs * 12 * sizeof(cf_t));
  rc = srsran_pucch_decode(&pucch, &sf, &cfg, &res, grid, &data);
  if (rc) {
    return rc;
  }
  memcpy(z, pucch.z, SRSRAN_PUCCH_MAX_SYMBOLS * sizeof(cf_t));
  memset(outb, 0, 15);
  memset(llr, 0, 20 * sizeof(int16_t));
  *max_corr            = 0;
  const bool early     = isnormal(cfg.threshold_dmrs_detection) && data.correlation == 0.0f && !data.detected &&
                     (!isnormal(data.dmrs_correlation) || data.dmrs_correlation < cfg.threshold_dmrs_detection);
  if (!early) {
    if (cfg.format >= SRSRAN_PUCCH_FORMAT_2) {
      srsran_demod_soft_demodulate_s(SRSRAN_MOD_QPSK, pucch.z, llr, SRSRAN_PUCCH2_NOF_BITS / 2);
      srsran_sequence_pucch(&pucch.seq_f2, cfg.rnti, 2 * (sf.tti % 10), cell.id);
      srsran_scrambling_s_offset(&pucch.seq_f2, llr, 0, SRSRAN_PUCCH2_NOF_BITS);
      *max_corr = srsran_uci_decode_cqi_pucch(&pucch.cqi, llr, outb, d[7]);
    } else {
      outb[0] = data.uci_data.ack.ack_value[0];
      outb[1] = cfg.format == SRSRAN_PUCCH_FORMAT_1B ? data.uci_data.ack.ack_value[1] : 0;
      if (cfg.format == SRSRAN_PUCCH_FORMAT_1) {
        outb[0] = 0;
      }
    }
  }
  outb[13] = cfg.pucch2_drs_bits[0];
  outb[14] = cfg.pucch2_drs_bits[1];
  outf[0]  = data.detected;
  outf[1]  = data.correlation;
  outf[2]  = data.dmrs_correlation;
  outf[3]  = data.uci_data.ack.valid;
  outf[4]  = res.noise_estimate;
  outf[5]  = res.noise_estimate_dbm;
  outf[6]  = res.snr;
  outf[7]  = res.snr_db;
  outf[8]  = res.rsrp;
  outf[9]  = res.rsrp_dBfs;
  outf[10] = res.epre;
  outf[11] = res.epre_dBfs;
  outf[12] = res.ta_us;
  return 0;
}
