/* pbch_ref_wrap.c -- the exported wrappers tools/gen_golden_pbch.py calls.  They hold one receiving and one transmitting srsran_pbch_t and one
 * srsran_refsignal_t of the reference and call srsran_pbch_set_cell, srsran_pbch_get, srsran_pbch_encode, srsran_pbch_decode, decode_frame (pbch.c:399, not
 * static), srsran_pbch_mib_unpack, srsran_refsignal_cs_put_sf and srsran_chest_dl_estimate_cfg themselves.  The reference's files are compiled from where they
 * lie, with the reference flags of oracle/Makefile, into a temporary directory and loaded lazily (nothing of the reference is copied or committed).
 * chest_dl.c is included where it lies (REF_CHEST_DL_C: its path, given on the compiler's command line), as tools/ctrl_ref_wrap.c does, so that the estimator
 * object can be filled without its Wiener and FFT parts; then the decoder's arithmetic (REF_V37_C): the reference flags include debug.h in front of every
 * file, whose DEBUG() macro would switch that file's own #ifdef DEBUG printing on. */
#include REF_CHEST_DL_C
#undef DEBUG
#include REF_V37_C

#include <string.h>
#include <time.h>

#include "srsran/phy/phch/pbch.h"

int decode_frame(srsran_pbch_t* q, uint32_t src, uint32_t dst, uint32_t n, uint32_t nof_bits, uint32_t nof_ports);

static srsran_pbch_t      rxq, txq;
static srsran_refsignal_t refs;
static srsran_cell_t      rx_cell, tx_cell;
static int                is_open;

static void cell_of(srsran_cell_t* c, const uint32_t* d, uint32_t ports)
{
  memset(c, 0, sizeof(*c));
  c->nof_prb         = d[0];
  c->nof_ports       = ports;
  c->id              = d[2];
  c->cp              = d[3] == 7 ? SRSRAN_CP_NORM : SRSRAN_CP_EXT;
  c->phich_length    = SRSRAN_PHICH_NORM;
  c->phich_resources = SRSRAN_PHICH_R_1;
  c->frame_type      = SRSRAN_FDD;
}

/* d: nof_prb, nof_ports (what the receiver is told: 0, 1, 2, 4), id, cp_nsymb (srsran_hip_pbch_cell_t); tx_ports: what the transmitter has */
int pbch_ref_open(const uint32_t* d, uint32_t tx_ports)
{
  cell_of(&rx_cell, d, d[1]);
  cell_of(&tx_cell, d, tx_ports);
  memset(&rxq, 0, sizeof(rxq));
  memset(&txq, 0, sizeof(txq));
  memset(&refs, 0, sizeof(refs));
  if (srsran_pbch_init(&rxq) || srsran_pbch_set_cell(&rxq, rx_cell) || srsran_pbch_init(&txq) || srsran_pbch_set_cell(&txq, tx_cell) ||
      srsran_refsignal_cs_init(&refs, tx_cell.nof_prb) || srsran_refsignal_cs_set_cell(&refs, tx_cell)) {
    return -100;
  }
  is_open = 1;
  return (int)rxq.nof_symbols;
}

void pbch_ref_close(void)
{
  if (is_open) {
    srsran_refsignal_free(&refs);
    srsran_pbch_free(&rxq);
    srsran_pbch_free(&txq);
    is_open = 0;
  }
}

int pbch_ref_get(cf_t* slot1, cf_t* out)
{
  return srsran_pbch_get(slot1, out, rx_cell);
}

/* srsran_pbch_encode of frame `frame_idx` (0 .. 3) of the 40 ms into the port grids (whole subframes) */
int pbch_ref_encode(uint8_t* payload, cf_t** grids, uint32_t frame_idx)
{
  cf_t* g[SRSRAN_MAX_PORTS];
  for (uint32_t i = 0; i < SRSRAN_MAX_PORTS; i++) {
    g[i] = i < tx_cell.nof_ports ? grids[i] : NULL;
  }
  return srsran_pbch_encode(&txq, payload, g, frame_idx);
}

int pbch_ref_cs_put(uint32_t port, cf_t* grid)
{
  srsran_dl_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  return srsran_refsignal_cs_put_sf(&refs, &sf, port, grid);
}

/* subframe 0's pilot rows of a cell with `ports` ports (the receiver's estimator: 4 when it searches) */
int pbch_ref_cs_pilots(const uint32_t* d, uint32_t ports, cf_t* pilots0, cf_t* pilots1)
{
  srsran_refsignal_t r;
  srsran_cell_t      c;
  cell_of(&c, d, ports);
  memset(&r, 0, sizeof(r));
  if (srsran_refsignal_cs_init(&r, c.nof_prb) || srsran_refsignal_cs_set_cell(&r, c)) {
    return -1;
  }
  memcpy(pilots0, r.pilots[0][0], 8 * c.nof_prb * sizeof(cf_t));
  memcpy(pilots1, r.pilots[1][0], 4 * c.nof_prb * sizeof(cf_t));
  srsran_refsignal_free(&r);
  return 0;
}

void pbch_ref_set_state(uint32_t frame_idx, const float* llr)
{
  rxq.frame_idx = frame_idx;
  memcpy(rxq.llr, llr, 4 * 2 * rxq.nof_symbols * sizeof(float));
}

uint32_t pbch_ref_get_state(float* llr, cf_t* d)
{
  memcpy(llr, rxq.llr, 4 * 2 * rxq.nof_symbols * sizeof(float));
  if (d) {
    memcpy(d, rxq.d, rxq.nof_symbols * sizeof(cf_t));
  }
  return rxq.frame_idx;
}

/* decode_frame on the object's q->llr: rm_f (120), data (40); returns its value (1: hit) */
int pbch_ref_frame(uint32_t src, uint32_t dst, uint32_t n, uint32_t nof_ports, float* rm_f, uint8_t* data)
{
  int rc = decode_frame(&rxq, src, dst, n, 2 * rxq.nof_symbols, nof_ports);
  if (rm_f) {
    memcpy(rm_f, rxq.rm_f, sizeof(rxq.rm_f));
  }
  if (data) {
    memcpy(data, rxq.data, sizeof(rxq.data));
  }
  return rc;
}

/* srsran_pbch_decode: rx: the first antenna's subframe grid, ce[port]: whole-subframe estimate grids */
int pbch_ref_decode(cf_t* rx, cf_t** ce, float noise_estimate, uint8_t* payload, uint32_t* nof_tx_ports, int* sfn_offset)
{
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS] = {rx, NULL, NULL, NULL};
  memset(&ch, 0, sizeof(ch));
  for (uint32_t p = 0; p < SRSRAN_MAX_PORTS; p++) {
    ch.ce[p][0] = ce[p];
  }
  ch.noise_estimate = noise_estimate;
  return srsran_pbch_decode(&rxq, &ch, y, payload, nof_tx_ports, sfn_offset);
}

void pbch_ref_mib_unpack(uint8_t* msg, uint32_t* out)
{
  srsran_cell_t c;
  uint32_t      sfn = 0;
  memset(&c, 0, sizeof(c));
  srsran_pbch_mib_unpack(msg, &c, &sfn);
  out[0] = c.nof_prb;
  out[1] = c.phich_length == SRSRAN_PHICH_EXT;
  out[2] = c.phich_resources == SRSRAN_PHICH_R_1_6 ? 0 : c.phich_resources == SRSRAN_PHICH_R_1_2 ? 1 : c.phich_resources == SRSRAN_PHICH_R_1 ? 2 : 3;
  out[3] = sfn;
}

/* srsran_chest_dl_estimate (a zeroed configuration: AVERAGE estimator, REFS noise, the Gauss filter made from the noise estimate) in subframe 0 on one
 * receive antenna, on an estimator object filled as tools/chest_dl_ref_wrap.c fills it, with the pilot rows given.  d, ports: the estimator's cell. */
static srsran_chest_dl_t est;
static int               est_open;

int pbch_ref_chest_open(const uint32_t* d, uint32_t ports, cf_t* pilots0, cf_t* pilots1)
{
  const uint32_t prb = d[0];
  memset(&est, 0, sizeof(est));
  cell_of(&est.cell, d, ports);
  est.nof_rx_antennas       = 1;
  est.csr_refs.cell         = est.cell;
  est.csr_refs.pilots[0][0] = pilots0;
  est.csr_refs.pilots[1][0] = pilots1;
  est.tmp_noise               = srsran_vec_cf_malloc(20 * prb);
  est.tmp_cfo_estimate        = srsran_vec_cf_malloc(20 * prb);
  est.pilot_estimates         = srsran_vec_cf_malloc(20 * prb);
  est.pilot_estimates_average = srsran_vec_cf_malloc(20 * prb);
  est.pilot_recv_signal       = srsran_vec_cf_malloc(20 * prb);
  if (!est.tmp_noise || !est.tmp_cfo_estimate || !est.pilot_estimates || !est.pilot_estimates_average || !est.pilot_recv_signal ||
      srsran_interp_linear_vector_init(&est.srsran_interp_linvec, SRSRAN_NRE * prb) || srsran_interp_linear_init(&est.srsran_interp_lin, 2 * prb, SRSRAN_NRE / 2) ||
      srsran_interp_linear_init(&est.srsran_interp_lin_3, 4 * prb, SRSRAN_NRE / 4)) {
    return -100;
  }
  est_open = 1;
  return 0;
}

void pbch_ref_chest_close(void)
{
  if (est_open) {
    srsran_interp_linear_vector_free(&est.srsran_interp_linvec);
    srsran_interp_linear_free(&est.srsran_interp_lin);
    srsran_interp_linear_free(&est.srsran_interp_lin_3);
    free(est.tmp_noise);
    free(est.tmp_cfo_estimate);
    free(est.pilot_estimates);
    free(est.pilot_estimates_average);
    free(est.pilot_recv_signal);
    est_open = 0;
  }
}

int pbch_ref_chest(cf_t* rx, cf_t** ce, float* noise_estimate)
{
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_res_t res;
  cf_t*                 y[SRSRAN_MAX_PORTS] = {rx, NULL, NULL, NULL};
  memset(&sf, 0, sizeof(sf));
  memset(&res, 0, sizeof(res));
  memset(est.noise_estimate, 0, sizeof(est.noise_estimate)); /* no state carried from call to call */
  est.cfo = 0;
  for (uint32_t p = 0; p < est.cell.nof_ports; p++) {
    res.ce[p][0] = ce[p];
  }
  int rc          = srsran_chest_dl_estimate(&est, &sf, y, &res);
  *noise_estimate = res.noise_estimate;
  return rc;
}

/* the time of srsran_chest_dl_estimate + srsran_pbch_decode from the state given, `iters` times over (the state is put back before every pass, which is
 * counted: a copy of 7.5 KB); seconds per pass */
double pbch_ref_time(uint32_t iters, uint32_t frame_idx, const float* llr, cf_t* rx, cf_t** ce)
{
  struct timespec t0, t1;
  uint8_t         payload[SRSRAN_BCH_PAYLOAD_LEN];
  uint32_t        ports;
  int             off;
  float           noise;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (uint32_t i = 0; i < iters; i++) {
    pbch_ref_set_state(frame_idx, llr);
    pbch_ref_chest(rx, ce, &noise);
    pbch_ref_decode(rx, ce, noise, payload, &ports, &off);
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec)) / iters;
}

/* what srsran_pbch_set_cell would set for a receiver told `ports` (0: search), without its id test: it keeps the cell of the first call when the id is the same */
void pbch_ref_told(uint32_t ports)
{
  rxq.search_all_ports = ports == 0;
  rxq.cell.nof_ports   = ports ? ports : SRSRAN_MAX_PORTS;
}
