/* prach_ref_wrap.c -- the exported wrappers tools/gen_golden_prach.py calls.  The reference's prach.c is included where it lies (REF_PRACH_C: its path,
 * given on the compiler's command line) and compiled with the reference flags of oracle/Makefile into a temporary directory (nothing of the reference is
 * copied or committed); its vector and common functions are bound in oracle/_ref/libsrsran_ref.so.
 * The reference's transform backend (FFTW) is not available, so the srsran_dft_* functions prach.c calls are supplied HERE: a plan is its fields, and a run
 * goes to orc_dft_c of oracle/liboracle.so, which works in double precision and holds the mirror / dc / norm rules of dft_fftw.c:297-354. */
#include REF_PRACH_C

#include <stdlib.h>
#include <string.h>

void orc_dft_c(const float* in, float* out, int n, int backward, int mirror, int dc, int norm);

int srsran_dft_plan(srsran_dft_plan_t* plan, int dft_points, srsran_dft_dir_t dir, srsran_dft_mode_t type)
{
  memset(plan, 0, sizeof(*plan));
  plan->init_size = dft_points;
  plan->size      = dft_points;
  plan->dir       = dir;
  plan->forward   = dir == SRSRAN_DFT_FORWARD;
  plan->mode      = type;
  return type == SRSRAN_DFT_COMPLEX ? 0 : -1;
}
int srsran_dft_replan(srsran_dft_plan_t* plan, const int new_dft_points)
{
  if (new_dft_points > plan->init_size) {
    return -1;
  }
  plan->size = new_dft_points;
  return 0;
}
void srsran_dft_plan_free(srsran_dft_plan_t* plan) { memset(plan, 0, sizeof(*plan)); }
void srsran_dft_plan_set_mirror(srsran_dft_plan_t* plan, bool val) { plan->mirror = val; }
void srsran_dft_plan_set_norm(srsran_dft_plan_t* plan, bool val) { plan->norm = val; }
void srsran_dft_run(srsran_dft_plan_t* plan, const void* in, void* out)
{
  orc_dft_c((const float*)in, (float*)out, plan->size, !plan->forward, plan->mirror, plan->dc, plan->norm);
}

static srsran_prach_t prach;
static int            is_open;

void prach_ref_close(void)
{
  if (is_open) {
    srsran_prach_free(&prach);
    is_open = 0;
  }
}

/* d: nof_prb, config_idx, root_seq_idx, zero_corr_zone, num_ra_preambles, hs_flag, freq_domain_offset_calc (srsran_hip_prach_cfg_t) */
int prach_ref_open(const uint32_t* d, float detect_factor)
{
  srsran_prach_cfg_t cfg;
  prach_ref_close();
  memset(&cfg, 0, sizeof(cfg));
  cfg.config_idx                     = d[1];
  cfg.root_seq_idx                   = d[2];
  cfg.zero_corr_zone                 = d[3];
  cfg.num_ra_preambles               = d[4];
  cfg.hs_flag                        = d[5] != 0;
  cfg.enable_freq_domain_offset_calc = d[6] != 0;
  if (srsran_prach_init(&prach, srsran_symbol_sz(d[0]))) {
    return -100;
  }
  is_open = 1;
  if (srsran_prach_set_cfg(&prach, &cfg, d[0])) {
    return -101;
  }
  if (detect_factor != 0.0f) {
    srsran_prach_set_detect_factor(&prach, detect_factor);
  }
  return 0;
}

/* N_zc, N_cs, N_ifft_ul, N_ifft_prach, N_seq, N_cp, N_roots, n_wins, num_ra_preambles, then root_seqs_idx[64] */
void prach_ref_info(uint32_t* out)
{
  out[0] = prach.N_zc;
  out[1] = prach.N_cs;
  out[2] = prach.N_ifft_ul;
  out[3] = prach.N_ifft_prach;
  out[4] = prach.N_seq;
  out[5] = prach.N_cp;
  out[6] = prach.N_roots;
  out[7] = prach.N_zc / (prach.N_cs ? prach.N_cs : prach.N_zc);
  out[8] = prach.num_ra_preambles;
  memcpy(out + 9, prach.root_seqs_idx, 64 * sizeof(uint32_t));
}

void prach_ref_root_order(uint32_t* out838) { memcpy(out838, prach_zc_roots, 838 * sizeof(uint32_t)); }

int prach_ref_gen(uint32_t seq_index, uint32_t freq_offset, cf_t* signal) { return srsran_prach_gen(&prach, seq_index, freq_offset, signal); }

void prach_ref_spectrum(uint32_t seq_index, cf_t* out) { memcpy(out, get_precoded_dft(&prach, seq_index), prach.N_zc * sizeof(cf_t)); }

int prach_ref_detect(uint32_t freq_offset, cf_t* signal, uint32_t sig_len, uint32_t* indices, float* t_offsets, float* peak_to_avg, uint32_t* n_indices)
{
  return srsran_prach_detect_offset(&prach, freq_offset, signal, sig_len, indices, t_offsets, peak_to_avg, n_indices);
}

void prach_ref_bins(cf_t* out) { memcpy(out, prach.prach_bins, prach.N_zc * sizeof(cf_t)); }

/* What srsran_prach_process leaves for root i of the last detection: it is run over roots 0 .. i, so that corr, cross and the peaks are root i's when it
 * returns.  corr_ave and the cross sum are the expressions of :800 and :753 on what it left.  peak_offsets is zeroed first (the reference leaves the
 * offset of a window whose peak stayed 0 as it was). */
void prach_ref_root(uint32_t i, float* corr, float* corr_ave, cf_t* cross_sum, float* peak_values, uint32_t* peak_offsets)
{
  uint32_t        keep = prach.num_ra_preambles, n_wins = prach.N_zc / (prach.N_cs ? prach.N_cs : prach.N_zc), n = 0;
  static uint32_t indices[65 * 64];
  memset(prach.peak_offsets, 0, sizeof(prach.peak_offsets));
  prach.num_ra_preambles = i + 1;
  srsran_prach_process(&prach, NULL, indices, NULL, NULL, &n, -2, 0, 0);
  prach.num_ra_preambles = keep;
  memcpy(corr, prach.corr, prach.N_zc * sizeof(float));
  *corr_ave  = srsran_vec_acc_ff(prach.corr, prach.N_zc) / prach.N_zc;
  *cross_sum = srsran_vec_acc_cc(prach.cross, prach.N_zc);
  memcpy(peak_values, prach.peak_values, n_wins * sizeof(float));
  memcpy(peak_offsets, prach.peak_offsets, n_wins * sizeof(uint32_t));
}
