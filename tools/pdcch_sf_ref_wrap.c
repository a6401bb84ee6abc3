/* pdcch_sf_ref_wrap.c -- the exported wrappers tools/gen_golden_pdcch_sf.py calls.  They hold one srsran_regs_t and one srsran_pdcch_t of the reference and
 * call srsran_regs_init_opts, srsran_pdcch_encode, srsran_pdcch_extract_llr and srsran_pdcch_dci_decode themselves; regs.c, pdcch.c and the reference files they
 * bind into are compiled from where they lie, with the reference flags of oracle/Makefile, into a temporary directory and loaded lazily (nothing of the
 * reference is copied or committed). */
/* the decoder's arithmetic is included where it lies (REF_V37_C: its path, given on the compiler's command line), as tools/conv_ref_wrap.c does: the reference
 * flags include debug.h in front of every file, whose DEBUG() macro would switch that file's own #ifdef DEBUG printing on */
#undef DEBUG
#include REF_V37_C

#include <string.h>

#include "srsran/phy/ch_estimation/chest_dl.h"
#include "srsran/phy/phch/pdcch.h"
#include "srsran/phy/phch/regs.h"

static srsran_regs_t  regs;
static srsran_pdcch_t pdcch;
static srsran_cell_t  cell;
static int            is_open;

/* d: nof_prb, nof_ports, id, cp_nsymb, phich_length, phich_resources, phich_mi, mbsfn_or_sf1_6_tdd, cfi, sf_idx, nof_rx (srsran_hip_pdcch_sf_t).
 * Returns srsran_regs_pdcch_nregs of d's cfi, or a negative number. */
int pdcch_sf_ref_open(const uint32_t* d)
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
  memset(&pdcch, 0, sizeof(pdcch));
  if (srsran_pdcch_init_ue(&pdcch, cell.nof_prb, d[10]) || srsran_pdcch_set_cell(&pdcch, &regs, cell)) {
    srsran_regs_free(&regs);
    return -101;
  }
  is_open = 1;
  return srsran_regs_pdcch_nregs(&regs, d[8]);
}

void pdcch_sf_ref_close(void)
{
  if (is_open) {
    srsran_pdcch_free(&pdcch);
    srsran_regs_free(&regs);
    is_open = 0;
  }
}

/* srsran_regs_pdcch_get on one grid: d gets 4 nregs points.  Returns what the call returns. */
int pdcch_sf_ref_get(uint32_t cfi, cf_t* grid, cf_t* d)
{
  return srsran_regs_pdcch_get(&regs, cfi, grid, d);
}

/* srsran_pdcch_encode of one message into the port grids (which the caller zeroed before the first message) */
int pdcch_sf_ref_encode(uint32_t cfi, uint32_t sf_idx, uint32_t ncce, uint32_t L, uint32_t nof_bits, uint16_t rnti, const uint8_t* payload, cf_t** grids)
{
  srsran_dl_sf_cfg_t sf;
  srsran_dci_msg_t   msg;
  cf_t*              g[SRSRAN_MAX_PORTS] = {NULL, NULL, NULL, NULL};
  memset(&sf, 0, sizeof(sf));
  memset(&msg, 0, sizeof(msg));
  sf.tti = sf_idx;
  sf.cfi = cfi;
  memcpy(msg.payload, payload, nof_bits);
  msg.nof_bits      = nof_bits;
  msg.location.L    = L;
  msg.location.ncce = ncce;
  msg.rnti          = rnti;
  for (uint32_t i = 0; i < cell.nof_ports; i++) {
    g[i] = grids[i];
  }
  return srsran_pdcch_encode(&pdcch, &sf, &msg, g);
}

/* srsran_pdcch_extract_llr: rx[nof_rx] received grids, ce[port * nof_rx + rx] estimate grids.  llr: 72 NOF_CCE floats (q->llr), d: 36 NOF_CCE points (q->d) */
int pdcch_sf_ref_extract(uint32_t cfi, uint32_t sf_idx, uint32_t nof_rx, cf_t** rx, cf_t** ce, float noise_estimate, float* llr, cf_t* d)
{
  srsran_dl_sf_cfg_t    sf;
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS] = {NULL, NULL, NULL, NULL};
  memset(&sf, 0, sizeof(sf));
  memset(&ch, 0, sizeof(ch));
  sf.tti = sf_idx;
  sf.cfi = cfi;
  for (uint32_t j = 0; j < nof_rx; j++) {
    y[j] = rx[j];
    for (uint32_t p = 0; p < cell.nof_ports; p++) {
      ch.ce[p][j] = ce[p * nof_rx + j];
    }
  }
  ch.noise_estimate = noise_estimate;
  int rc            = srsran_pdcch_extract_llr(&pdcch, &sf, &ch, y);
  int nbits         = 8 * srsran_regs_pdcch_nregs(&regs, cfi);
  memcpy(llr, pdcch.llr, nbits * sizeof(float));
  memcpy(d, pdcch.d, (nbits / 2) * sizeof(cf_t));
  return rc;
}

/* srsran_pdcch_dci_decode on the E soft bits at e: bits gets nof_bits + 16 */
int pdcch_sf_ref_decode(float* e, uint32_t E, uint32_t nof_bits, uint8_t* bits, uint16_t* crc_rem)
{
  return srsran_pdcch_dci_decode(&pdcch, e, bits, E, nof_bits, crc_rem);
}
