/*
 * oracle_shim.c -- TEST INFRASTRUCTURE ONLY (our own code, not reference text).
 *
 * Puts the CPU oracle (oracle/liboracle.so) behind the handful of reference entry points that the reference's
 * own test programs call for this path, so that those UNMODIFIED programs -- ofdm_test, turbodecoder_test,
 * ldpc_dec_c_test and the file tests that decode recorded captures (pbch / pcfich / phich / pdcch / pdsch_pdcch /
 * pmch _file_test) -- judge the ORACLE by their own pass criteria, on the CPU.  This is how orc_ofdm.c / orc_dft_c
 * get pinned to known answers the reference holds (the MIB of signal.1.92M.dat, CFI 2 of signal.10M.dat, the DCI
 * and PDSCH CRC of signal.1.92M.amar.dat, the PMCH CRC of the 100-PRB MBSFN subframe): the reference's channel
 * estimator, PBCH / PCFICH / PDCCH / PDSCH decoders consume what the oracle's OFDM demodulator produces.
 *
 * The product never sees this file: it is linked only into oracle/_ref/ref_link/bin_oracle/.
 * Struct layouts come from include/srsran_amd/phy_abi.h (checked against the reference headers by
 * tests/test_host_cpu.py); handle state that the oracle does not need is left zero.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LSindex LSindex_declared_const_in_the_header
#include "srsran_amd/phy_abi.h"
#undef LSindex
#include "oracle.h"

int srsran_symbol_sz(uint32_t nof_prb); /* the reference's own (phy_common.c, part of the test program) */

/* ------------------------------------------------------------------ OFDM (ofdm.c) */

static int ofdm_init(srsran_ofdm_t* q, srsran_ofdm_cfg_t* cfg, int forward)
{
  if (cfg->symbol_sz == 0) { /* ofdm.c:41-48 */
    int n = srsran_symbol_sz(cfg->nof_prb);
    if (n <= 0) {
      return SRSRAN_ERROR;
    }
    cfg->symbol_sz = (uint32_t)n;
  }
  if (q->max_prb > 0) { /* ofdm.c:50-58: a re-initialisation only resizes */
    q->cfg.cp        = cfg->cp;
    q->cfg.nof_prb   = cfg->nof_prb;
    q->cfg.symbol_sz = cfg->symbol_sz;
  } else {
    q->cfg     = *cfg;
    q->max_prb = cfg->nof_prb;
  }
  const uint32_t N     = q->cfg.symbol_sz;
  q->nof_symbols       = q->cfg.cp == SRSRAN_CP_NORM ? 7 : 6;
  q->nof_symbols_mbsfn = 6;
  q->nof_re            = q->cfg.nof_prb * 12;
  q->nof_guards        = (N - q->nof_re) / 2;
  q->slot_sz           = 15 * N / 2;
  q->sf_sz             = 15 * N;
  q->fft_plan.size     = (int)N;
  q->fft_plan.forward  = forward != 0;
  q->fft_plan.norm     = q->cfg.normalize;
  q->mbsfn_subframe    = q->cfg.sf_type == SRSRAN_SF_MBSFN;
  q->non_mbsfn_region  = q->mbsfn_subframe ? 2 : 0; /* ofdm.c:198-203 */
  if (forward && q->cfg.in_buffer) {
    memset(q->cfg.in_buffer, 0, sizeof(cf_t) * q->sf_sz); /* ofdm.c:142-147 */
  }
  return SRSRAN_SUCCESS;
}

static void ofdm_cfg_of(const srsran_ofdm_t* q, orc_ofdm_cfg_t* c)
{
  memset(c, 0, sizeof(*c));
  c->nof_prb          = q->cfg.nof_prb;
  c->symbol_sz        = q->cfg.symbol_sz;
  c->cp_ext           = q->cfg.cp == SRSRAN_CP_EXT;
  c->normalize        = q->fft_plan.norm;
  c->freq_shift_f     = q->cfg.freq_shift_f;
  c->rx_window_offset = q->cfg.rx_window_offset;
  c->keep_dc          = q->cfg.keep_dc;
  c->mbsfn_region     = q->mbsfn_subframe ? q->non_mbsfn_region : 0;
}

#define OFDM_INIT(name, sf, fwd)                                                                                   \
  int name(srsran_ofdm_t* q, srsran_cp_t cp, cf_t* in, cf_t* out, uint32_t prb)                                      \
  {                                                                                                                \
    memset(q, 0, sizeof(*q));                                                                                      \
    srsran_ofdm_cfg_t cfg;                                                                                         \
    memset(&cfg, 0, sizeof(cfg));                                                                                  \
    cfg.cp = cp, cfg.in_buffer = in, cfg.out_buffer = out, cfg.nof_prb = prb, cfg.sf_type = sf;                    \
    return ofdm_init(q, &cfg, fwd);                                                                                \
  }
OFDM_INIT(srsran_ofdm_rx_init, SRSRAN_SF_NORM, 1)
OFDM_INIT(srsran_ofdm_rx_init_mbsfn, SRSRAN_SF_MBSFN, 1)
OFDM_INIT(srsran_ofdm_tx_init, SRSRAN_SF_NORM, 0)
OFDM_INIT(srsran_ofdm_tx_init_mbsfn, SRSRAN_SF_MBSFN, 0)

int srsran_ofdm_rx_init_cfg(srsran_ofdm_t* q, srsran_ofdm_cfg_t* cfg) { return ofdm_init(q, cfg, 1); }
int srsran_ofdm_tx_init_cfg(srsran_ofdm_t* q, srsran_ofdm_cfg_t* cfg) { return ofdm_init(q, cfg, 0); }

static int ofdm_set_prb(srsran_ofdm_t* q, srsran_cp_t cp, uint32_t nof_prb, int fwd)
{
  srsran_ofdm_cfg_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.cp = cp, cfg.nof_prb = nof_prb;
  return ofdm_init(q, &cfg, fwd);
}
int  srsran_ofdm_rx_set_prb(srsran_ofdm_t* q, srsran_cp_t cp, uint32_t nof_prb) { return ofdm_set_prb(q, cp, nof_prb, 1); }
int  srsran_ofdm_tx_set_prb(srsran_ofdm_t* q, srsran_cp_t cp, uint32_t nof_prb) { return ofdm_set_prb(q, cp, nof_prb, 0); }
void srsran_ofdm_rx_free(srsran_ofdm_t* q) { memset(q, 0, sizeof(*q)); }
void srsran_ofdm_tx_free(srsran_ofdm_t* q) { memset(q, 0, sizeof(*q)); }
void srsran_ofdm_set_normalize(srsran_ofdm_t* q, bool en) { q->fft_plan.norm = en; }
void srsran_ofdm_set_non_mbsfn_region(srsran_ofdm_t* q, uint8_t r) { q->non_mbsfn_region = r; }
int  srsran_ofdm_set_freq_shift(srsran_ofdm_t* q, float f)
{
  q->cfg.freq_shift_f = f;
  return SRSRAN_SUCCESS;
}

void srsran_ofdm_rx_sf(srsran_ofdm_t* q)
{
  orc_ofdm_cfg_t c;
  ofdm_cfg_of(q, &c);
  if (orc_ofdm_rx_sf(&c, (const float*)q->cfg.in_buffer, (float*)q->cfg.out_buffer)) {
    fprintf(stderr, "oracle_shim: orc_ofdm_rx_sf refused the configuration\n");
    abort();
  }
}

void srsran_ofdm_rx_sf_ng(srsran_ofdm_t* q, cf_t* input, cf_t* output)
{
  orc_ofdm_cfg_t c;
  ofdm_cfg_of(q, &c);
  if (q->mbsfn_subframe) { /* ofdm.c:477-480 uses the object's own buffers there */
    input = q->cfg.in_buffer, output = q->cfg.out_buffer;
  }
  if (orc_ofdm_rx_sf(&c, (const float*)input, (float*)output)) {
    abort();
  }
}

void srsran_ofdm_tx_sf(srsran_ofdm_t* q)
{
  orc_ofdm_cfg_t c;
  ofdm_cfg_of(q, &c);
  if (orc_ofdm_tx_sf(&c, (const float*)q->cfg.in_buffer, (float*)q->cfg.out_buffer)) {
    fprintf(stderr, "oracle_shim: orc_ofdm_tx_sf refused the configuration\n");
    abort();
  }
}

/* ------------------------------------------------------------------ DFT (dft_fftw.c): complex plans only */

int srsran_dft_plan_c(srsran_dft_plan_t* plan, int n, srsran_dft_dir_t dir)
{
  memset(plan, 0, sizeof(*plan));
  plan->init_size = plan->size = n;
  plan->in  = calloc((size_t)n, sizeof(cf_t));
  plan->out = calloc((size_t)n, sizeof(cf_t));
  plan->dir = dir, plan->forward = dir == SRSRAN_DFT_FORWARD, plan->mode = SRSRAN_DFT_COMPLEX;
  return plan->in && plan->out ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}
int srsran_dft_plan(srsran_dft_plan_t* plan, int n, srsran_dft_dir_t dir, srsran_dft_mode_t mode)
{
  return mode == SRSRAN_DFT_COMPLEX ? srsran_dft_plan_c(plan, n, dir) : SRSRAN_ERROR;
}
int srsran_dft_replan(srsran_dft_plan_t* plan, const int n)
{
  if (n > plan->init_size) {
    return SRSRAN_ERROR;
  }
  plan->size = n;
  return SRSRAN_SUCCESS;
}
int  srsran_dft_replan_c(srsran_dft_plan_t* plan, int n) { return srsran_dft_replan(plan, n); }
void srsran_dft_plan_free(srsran_dft_plan_t* plan)
{
  if (plan && !plan->is_guru) {
    free(plan->in);
    free(plan->out);
  }
  if (plan) {
    memset(plan, 0, sizeof(*plan));
  }
}
void srsran_dft_plan_set_mirror(srsran_dft_plan_t* plan, bool v) { plan->mirror = v; }
void srsran_dft_plan_set_db(srsran_dft_plan_t* plan, bool v) { plan->db = v; }
void srsran_dft_plan_set_norm(srsran_dft_plan_t* plan, bool v) { plan->norm = v; }
void srsran_dft_plan_set_dc(srsran_dft_plan_t* plan, bool v) { plan->dc = v; }
void srsran_dft_run_c(srsran_dft_plan_t* plan, const cf_t* in, cf_t* out)
{
  orc_dft_c((const float*)in, (float*)out, plan->size, !plan->forward, plan->mirror, plan->dc, plan->norm);
}
void srsran_dft_run_c_zerocopy(srsran_dft_plan_t* plan, const cf_t* in, cf_t* out)
{
  orc_dft_c((const float*)in, (float*)out, plan->size, !plan->forward, 0, 0, 0);
}
void srsran_dft_run(srsran_dft_plan_t* plan, const void* in, void* out) { srsran_dft_run_c(plan, (const cf_t*)in, (cf_t*)out); }

/* ------------------------------------------------------------------ the two PSS helpers the channel estimator links (pss.c:341-384) */

int srsran_pss_generate(cf_t* signal, uint32_t N_id_2) { return orc_pss_generate((float*)signal, N_id_2); }
void srsran_pss_get_slot(cf_t* slot, cf_t* pss_signal, uint32_t nof_prb, srsran_cp_t cp)
{
  int k = ((cp == SRSRAN_CP_NORM ? 7 : 6) - 1) * (int)nof_prb * 12 + (int)nof_prb * 12 / 2 - 31;
  memcpy(pss_signal, &slot[k], 62 * sizeof(cf_t));
}

/* ------------------------------------------------------------------ turbo decoder (turbodecoder.c): every call re-runs the oracle's
 * whole-run decoder for n_iter half iterations from the (unchanged) input -- same results as the reference's resumable loop */

uint32_t srsran_tdec_autoimp_get_subblocks(uint32_t long_cb) { return orc_tdec_autoimp_subblocks(long_cb); }
uint32_t srsran_tdec_autoimp_get_subblocks_8bit(uint32_t long_cb) { return orc_tdec_autoimp_subblocks_8bit(long_cb); }

int srsran_tdec_init_manual(srsran_tdec_t* h, uint32_t max_long_cb, srsran_tdec_impl_type_t dec_type)
{
  memset(h, 0, sizeof(*h));
  h->max_long_cb   = max_long_cb;
  h->dec_type      = dec_type;
  h->current_cbidx = -1;
  return SRSRAN_SUCCESS;
}
int  srsran_tdec_init(srsran_tdec_t* h, uint32_t max_long_cb) { return srsran_tdec_init_manual(h, max_long_cb, SRSRAN_TDEC_AUTO); }
void srsran_tdec_free(srsran_tdec_t* h) { memset(h, 0, sizeof(*h)); }
void srsran_tdec_force_not_sb(srsran_tdec_t* h) { h->force_not_sb = true; }
int  srsran_tdec_get_nof_iterations(srsran_tdec_t* h) { return h->n_iter; }
int  srsran_tdec_new_cb(srsran_tdec_t* h, uint32_t long_cb)
{
  if (long_cb > h->max_long_cb || orc_tc_cb_index(long_cb) < 0 || orc_tc_cb_size((uint32_t)orc_tc_cb_index(long_cb)) != (int)long_cb) {
    return SRSRAN_ERROR;
  }
  h->n_iter = 0, h->current_long_cb = long_cb, h->current_cbidx = orc_tc_cb_index(long_cb);
  return SRSRAN_SUCCESS;
}
static int sb_layout16(const srsran_tdec_t* h)
{
  /* turbodecoder_iter.h:88: the 16-bit decoders take the rm_turbo sub-block layout only in AUTO mode with a window decoder */
  return !h->force_not_sb && h->dec_type == SRSRAN_TDEC_AUTO && orc_tdec_autoimp_subblocks(h->current_long_cb) != 0;
}
static int sb_layout8(const srsran_tdec_t* h)
{
  return !h->force_not_sb && orc_tdec_autoimp_subblocks_8bit(h->current_long_cb) != 0;
}
void srsran_tdec_iteration(srsran_tdec_t* h, int16_t* input, uint8_t* output)
{
  if (h->current_cbidx >= 0) {
    h->n_iter++;
    if (orc_tdec_run_all(input, output, (uint32_t)h->n_iter, h->current_long_cb, (int)h->dec_type, sb_layout16(h), NULL, NULL)) {
      abort();
    }
  }
}
void srsran_tdec_iteration_8bit(srsran_tdec_t* h, int8_t* input, uint8_t* output)
{
  if (h->current_cbidx >= 0) {
    h->n_iter++;
    if (orc_tdec_run_all_8bit(input, output, (uint32_t)h->n_iter, h->current_long_cb, (int)h->dec_type, sb_layout8(h), NULL)) {
      abort();
    }
  }
}
int srsran_tdec_run_all(srsran_tdec_t* h, int16_t* input, uint8_t* output, uint32_t nof_iterations, uint32_t long_cb)
{
  if (srsran_tdec_new_cb(h, long_cb)) {
    return SRSRAN_ERROR;
  }
  h->n_iter = nof_iterations ? (int)nof_iterations : 1; /* do ... while: at least one (turbodecoder.c:542-544) */
  return orc_tdec_run_all(input, output, (uint32_t)h->n_iter, long_cb, (int)h->dec_type, sb_layout16(h), NULL, NULL) ? SRSRAN_ERROR : SRSRAN_SUCCESS;
}
int srsran_tdec_run_all_8bit(srsran_tdec_t* h, int8_t* input, uint8_t* output, uint32_t nof_iterations, uint32_t long_cb)
{
  if (srsran_tdec_new_cb(h, long_cb)) {
    return SRSRAN_ERROR;
  }
  h->n_iter = nof_iterations ? (int)nof_iterations : 1;
  return orc_tdec_run_all_8bit(input, output, (uint32_t)h->n_iter, long_cb, (int)h->dec_type, sb_layout8(h), NULL) ? SRSRAN_ERROR : SRSRAN_SUCCESS;
}

/* the reference's encoder (turbocoder.c, part of the test programs) builds its interleaver with this one (tc_interl_lte.c:61-94) */
int srsran_tc_interl_LTE_gen(srsran_tc_interl_t* h, uint32_t long_cb)
{
  if (long_cb > h->max_long_cb) {
    return SRSRAN_ERROR;
  }
  return orc_qpp_gen(long_cb, 1, h->forward, h->reverse) ? SRSRAN_ERROR : SRSRAN_SUCCESS;
}

/* ------------------------------------------------------------------ LDPC decoder (ldpc_decoder.c), int8 types */

/* base_graph.h:109-113: lifting size -> index of its set, 255 (VOID_LIFTSIZE) if invalid; the reference's cbsegm.c reads it */
uint8_t LSindex[385];
__attribute__((constructor)) static void fill_lsindex(void)
{
  for (int z = 0; z <= 384; z++) {
    int i     = orc_ldpc_ls_index((uint16_t)z);
    LSindex[z] = i < 0 ? VOID_LIFTSIZE : (uint8_t)i;
  }
}

typedef struct {
  orc_ldpc_graph_t g;
  int              flooded;
} shim_ldpc_t;

int srsran_ldpc_decoder_init(srsran_ldpc_decoder_t* q, const srsran_ldpc_decoder_args_t* args)
{
  memset(q, 0, sizeof(*q));
  shim_ldpc_t* s = (shim_ldpc_t*)calloc(1, sizeof(shim_ldpc_t));
  if (!s || orc_ldpc_graph(&s->g, (int)args->bg, args->ls)) {
    free(s);
    return SRSRAN_ERROR;
  }
  s->flooded = args->type == SRSRAN_LDPC_DECODER_C_FLOOD || args->type == SRSRAN_LDPC_DECODER_C_AVX2_FLOOD ||
               args->type == SRSRAN_LDPC_DECODER_C_AVX512_FLOOD;
  q->ptr = s, q->bg = args->bg, q->ls = args->ls;
  q->max_nof_iter = args->max_nof_iter ? args->max_nof_iter : 10; /* ldpc_decoder.c:42,579 */
  q->bgN = (uint8_t)s->g.bgN, q->bgM = (uint8_t)s->g.bgM, q->bgK = (uint8_t)s->g.bgK;
  q->liftN = (uint16_t)(q->bgN * q->ls), q->liftM = (uint16_t)(q->bgM * q->ls), q->liftK = (uint16_t)(q->bgK * q->ls);
  q->scaling_fctr = args->scaling_fctr;
  return SRSRAN_SUCCESS;
}
void srsran_ldpc_decoder_free(srsran_ldpc_decoder_t* q)
{
  free(q->ptr);
  memset(q, 0, sizeof(*q));
}
int srsran_ldpc_decoder_decode_c(srsran_ldpc_decoder_t* q, const int8_t* llrs, uint8_t* message, uint32_t cdwd_rm_length)
{
  shim_ldpc_t* s = (shim_ldpc_t*)q->ptr;
  return (s->flooded ? orc_ldpc_decode_c_flood : orc_ldpc_decode_c)(&s->g, q->scaling_fctr, (int)q->max_nof_iter, llrs, message,
                                                                    cdwd_rm_length, 0, 0, NULL);
}
