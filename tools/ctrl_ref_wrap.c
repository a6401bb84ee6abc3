/* ctrl_ref_wrap.c -- the exported wrappers tools/gen_golden_ctrl.py calls.  They hold one srsran_regs_t, srsran_pcfich_t, srsran_phich_t, srsran_pdcch_t and
 * srsran_refsignal_t of the reference and call srsran_regs_init_opts, the encoders and decoders of the three channels, srsran_refsignal_cs_put_sf and
 * srsran_chest_dl_estimate_cfg themselves.  The reference's files are compiled from where they lie, with the reference flags of oracle/Makefile, into a temporary
 * directory and loaded lazily (nothing of the reference is copied or committed).
 * chest_dl.c is included where it lies (REF_CHEST_DL_C: its path, given on the compiler's command line), as tools/chest_dl_ref_wrap.c does, so that the
 * estimator object can be filled without its Wiener and FFT parts; then the decoder's arithmetic (REF_V37_C), as tools/pdcch_sf_ref_wrap.c does: the reference
 * flags include debug.h in front of every file, whose DEBUG() macro would switch that file's own #ifdef DEBUG printing on. */
#include REF_CHEST_DL_C
#undef DEBUG
#include REF_V37_C

#include <string.h>

#include "srsran/phy/phch/pcfich.h"
#include "srsran/phy/phch/pdcch.h"
#include "srsran/phy/phch/phich.h"
#include "srsran/phy/phch/regs.h"

static srsran_regs_t      regs;
static srsran_pcfich_t    pcfich;
static srsran_phich_t     phich;
static srsran_pdcch_t     pdcch;
static srsran_refsignal_t refs;
static srsran_cell_t      cell;
static int                is_open;

/* d: nof_prb, nof_ports, id, cp_nsymb, phich_length, phich_resources, phich_mi, mbsfn_or_sf1_6_tdd, cfi, sf_idx, nof_rx (srsran_hip_pdcch_sf_t).
 * Returns srsran_regs_phich_ngroups, or a negative number. */
int ctrl_ref_open(const uint32_t* d)
{
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb         = d[0];
  cell.nof_ports       = d[1];
  cell.id              = d[2];
  cell.cp              = d[3] == 7 ? SRSRAN_CP_NORM : SRSRAN_CP_EXT;
  cell.phich_length    = d[4] ? SRSRAN_PHICH_EXT : SRSRAN_PHICH_NORM;
  cell.phich_resources = d[5] == 0 ? SRSRAN_PHICH_R_1_6 : d[5] == 1 ? SRSRAN_PHICH_R_1_2 : d[5] == 2 ? SRSRAN_PHICH_R_1 : SRSRAN_PHICH_R_2;
  cell.frame_type      = SRSRAN_FDD;
  if (srsran_regs_init_opts(&regs, cell, d[6], d[7] != 0)) {
    return -100;
  }
  memset(&pcfich, 0, sizeof(pcfich));
  memset(&phich, 0, sizeof(phich));
  memset(&pdcch, 0, sizeof(pdcch));
  memset(&refs, 0, sizeof(refs));
  if (srsran_pcfich_init(&pcfich, d[10]) || srsran_pcfich_set_cell(&pcfich, &regs, cell) || srsran_phich_init(&phich, d[10]) ||
      srsran_phich_set_cell(&phich, &regs, cell) || srsran_pdcch_init_ue(&pdcch, cell.nof_prb, d[10]) || srsran_pdcch_set_cell(&pdcch, &regs, cell) ||
      srsran_refsignal_cs_init(&refs, cell.nof_prb) || srsran_refsignal_cs_set_cell(&refs, cell)) {
    return -101;
  }
  is_open = 1;
  return (int)srsran_regs_phich_ngroups(&regs);
}

void ctrl_ref_close(void)
{
  if (is_open) {
    srsran_refsignal_free(&refs);
    srsran_pdcch_free(&pdcch);
    srsran_phich_free(&phich);
    srsran_pcfich_free(&pcfich);
    srsran_regs_free(&regs);
    is_open = 0;
  }
}

int ctrl_ref_pdcch_nregs(uint32_t cfi)
{
  return srsran_regs_pdcch_nregs(&regs, cfi);
}

int ctrl_ref_pcfich_get(cf_t* grid, cf_t* d)
{
  return srsran_regs_pcfich_get(&regs, grid, d);
}

int ctrl_ref_phich_get(cf_t* grid, cf_t* d, uint32_t ngroup)
{
  return srsran_regs_phich_get(&regs, grid, d, ngroup);
}

static void port_grids(cf_t** g, cf_t** grids)
{
  for (uint32_t i = 0; i < SRSRAN_MAX_PORTS; i++) {
    g[i] = i < cell.nof_ports ? grids[i] : NULL;
  }
}

/* the transmitters, into the port grids (which the caller zeroed before the first call) */
int ctrl_ref_pcfich_encode(uint32_t cfi, uint32_t sf_idx, cf_t** grids)
{
  srsran_dl_sf_cfg_t sf;
  cf_t*              g[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  sf.tti = sf_idx;
  sf.cfi = cfi;
  port_grids(g, grids);
  return srsran_pcfich_encode(&pcfich, &sf, g);
}

int ctrl_ref_phich_encode(uint32_t sf_idx, uint32_t ngroup, uint32_t nseq, uint32_t ack, cf_t** grids)
{
  srsran_dl_sf_cfg_t      sf;
  srsran_phich_resource_t r = {ngroup, nseq};
  cf_t*                   g[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  sf.tti = sf_idx;
  port_grids(g, grids);
  return srsran_phich_encode(&phich, &sf, r, (uint8_t)ack, g);
}

int ctrl_ref_pdcch_encode(uint32_t cfi, uint32_t sf_idx, uint32_t ncce, uint32_t L, uint32_t nof_bits, uint16_t rnti, const uint8_t* payload, cf_t** grids)
{
  srsran_dl_sf_cfg_t sf;
  srsran_dci_msg_t   msg;
  cf_t*              g[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  memset(&msg, 0, sizeof(msg));
  sf.tti = sf_idx;
  sf.cfi = cfi;
  memcpy(msg.payload, payload, nof_bits);
  msg.nof_bits      = nof_bits;
  msg.location.L    = L;
  msg.location.ncce = ncce;
  msg.rnti          = rnti;
  port_grids(g, grids);
  return srsran_pdcch_encode(&pdcch, &sf, &msg, g);
}

/* srsran_refsignal_cs_put_sf of one port into its grid */
int ctrl_ref_cs_put(uint32_t sf_idx, uint32_t port, cf_t* grid)
{
  srsran_dl_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = sf_idx;
  return srsran_refsignal_cs_put_sf(&refs, &sf, port, grid);
}

/* the subframe's pilot rows: 8 nof_prb points of ports 0 / 1, 4 nof_prb of ports 2 / 3 */
void ctrl_ref_cs_pilots(uint32_t sf_idx, cf_t* pilots0, cf_t* pilots1)
{
  memcpy(pilots0, refs.pilots[0][sf_idx], 8 * cell.nof_prb * sizeof(cf_t));
  memcpy(pilots1, refs.pilots[1][sf_idx], 4 * cell.nof_prb * sizeof(cf_t));
}

static void channel(srsran_chest_dl_res_t* ch, cf_t** y, uint32_t nof_rx, cf_t** rx, cf_t** ce, float noise_estimate)
{
  memset(ch, 0, sizeof(*ch));
  for (uint32_t j = 0; j < SRSRAN_MAX_PORTS; j++) {
    y[j] = j < nof_rx ? rx[j] : NULL;
  }
  for (uint32_t j = 0; j < nof_rx; j++) {
    for (uint32_t p = 0; p < cell.nof_ports; p++) {
      ch->ce[p][j] = ce[p * nof_rx + j];
    }
  }
  ch->noise_estimate = noise_estimate;
}

/* srsran_pcfich_decode: rx[nof_rx] received grids, ce[port * nof_rx + rx] estimate grids.  data_f: 32 floats (q->data_f), d: 16 points (q->d) */
int ctrl_ref_pcfich_decode(uint32_t sf_idx, uint32_t nof_rx, cf_t** rx, cf_t** ce, float noise_estimate, uint32_t* cfi, float* corr, float* data_f, cf_t* d)
{
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  sf.tti = sf_idx;
  channel(&ch, y, nof_rx, rx, ce, noise_estimate);
  int rc = srsran_pcfich_decode(&pcfich, &sf, &ch, y, corr);
  *cfi   = sf.cfi;
  memcpy(data_f, pcfich.data_f, 32 * sizeof(float));
  memcpy(d, pcfich.d, 16 * sizeof(cf_t));
  return rc;
}

/* srsran_phich_decode.  bits: 3 floats (q->data_rx), z: 3 points (q->z) */
int ctrl_ref_phich_decode(uint32_t sf_idx, uint32_t nof_rx, cf_t** rx, cf_t** ce, float noise_estimate, uint32_t ngroup, uint32_t nseq, uint32_t* ack,
                          float* distance, float* bits, cf_t* z)
{
  srsran_dl_sf_cfg_t      sf;
  srsran_chest_dl_res_t   ch;
  srsran_phich_resource_t r = {ngroup, nseq};
  srsran_phich_res_t      res;
  cf_t*                   y[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  memset(&res, 0, sizeof(res));
  sf.tti = sf_idx;
  channel(&ch, y, nof_rx, rx, ce, noise_estimate);
  int rc    = srsran_phich_decode(&phich, &sf, &ch, r, y, &res);
  *ack      = res.ack_value;
  *distance = res.distance;
  memcpy(bits, phich.data_rx, 3 * sizeof(float));
  memcpy(z, phich.z, 3 * sizeof(cf_t));
  return rc;
}

/* srsran_pdcch_extract_llr.  llr: 72 NOF_CCE floats (q->llr) */
int ctrl_ref_extract(uint32_t cfi, uint32_t sf_idx, uint32_t nof_rx, cf_t** rx, cf_t** ce, float noise_estimate, float* llr)
{
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS];
  memset(&sf, 0, sizeof(sf));
  sf.tti = sf_idx;
  sf.cfi = cfi;
  channel(&ch, y, nof_rx, rx, ce, noise_estimate);
  int rc = srsran_pdcch_extract_llr(&pdcch, &sf, &ch, y);
  memcpy(llr, pdcch.llr, 8 * srsran_regs_pdcch_nregs(&regs, cfi) * sizeof(float));
  return rc;
}

/* srsran_pdcch_dci_decode on the E soft bits at e: bits gets nof_bits + 16 */
int ctrl_ref_dci_decode(float* e, uint32_t E, uint32_t nof_bits, uint8_t* bits, uint16_t* crc_rem)
{
  return srsran_pdcch_dci_decode(&pdcch, e, bits, E, nof_bits, crc_rem);
}

/* srsran_chest_dl_estimate_cfg with the defaults of srsran_chest_dl_cfg_default but no filter state carried in (interpolating estimator, REFS noise, no
 * filter), on an estimator object filled as tools/chest_dl_ref_wrap.c fills it, with the cell's own pilot rows.  ce: [port * nof_rx + rx], whole-subframe
 * grids.  Returns the call's value; *noise_estimate is res.noise_estimate. */
int ctrl_ref_chest(uint32_t sf_idx, uint32_t nof_rx, cf_t** rx, cf_t** ce, float* noise_estimate)
{
  srsran_chest_dl_t     q;
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_cfg_t cfg;
  srsran_chest_dl_res_t res;
  cf_t*                 y[SRSRAN_MAX_PORTS];
  memset(&q, 0, sizeof(q));
  memset(&sf, 0, sizeof(sf));
  memset(&cfg, 0, sizeof(cfg));
  const uint32_t prb = cell.nof_prb;
  q.cell             = cell;
  q.nof_rx_antennas  = nof_rx;
  q.csr_refs.cell    = cell;
  q.csr_refs.pilots[0][sf_idx] = refs.pilots[0][sf_idx];
  q.csr_refs.pilots[1][sf_idx] = refs.pilots[1][sf_idx];
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
  sf.tti            = sf_idx;
  sf.sf_type        = SRSRAN_SF_NORM;
  cfg.estimator_alg = SRSRAN_ESTIMATOR_ALG_INTERPOLATE;
  cfg.noise_alg     = SRSRAN_NOISE_ALG_REFS;
  cfg.filter_type   = SRSRAN_CHEST_FILTER_NONE;
  channel(&res, y, nof_rx, rx, ce, 0.f);
  int rc          = srsran_chest_dl_estimate_cfg(&q, &sf, &cfg, y, &res);
  *noise_estimate = res.noise_estimate;
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
