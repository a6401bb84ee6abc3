/* tests/ref_link/ctrl_bind.c -- the reference-side binding of the downlink control calls (INTEGRATION.md sections 2.13 to 2.15).
 *
 * Compiled against the REFERENCE's headers, like a file a maintainer adds to lib/src/phy/phch.  pcfich.c, phich.c and pdcch.c are compiled unmodified; in
 * their OBJECT files the definitions of srsran_pcfich_decode, srsran_phich_decode, srsran_pdcch_extract_llr and srsran_pdcch_decode_msg are renamed to
 * <name>_ref (objcopy --redefine-sym, tests/ref_link/Makefile target `ctrl`) and the functions below take the original names: every caller in the reference
 * (srsran_ue_dl_decode_fft_estimate, dci_blind_search, srsran_ue_dl_decode_phich, the test programs) reaches them.  In the same link every srsran_viterbi_*
 * definition of the unmodified viterbi.o is renamed away, so the handle inside srsran_pdcch_t / srsran_pbch_t / srsran_uci_cqi_pusch_t / ... is the library's.
 *
 * What the library refuses (SRSRAN_ERROR_INVALID_INPUTS) goes to the renamed original and is counted.  Environment:
 *   CTRL_BIND_CHECK=1    every call also runs the renamed original on the same inputs into scratch outputs; decisions are compared exactly, floats as the
 *                        records of tests/golden do (the tolerances come in CTRL_BIND_TOL_CORR / _DISTANCE / _LLR: this file holds none).  Once per distinct
 *                        description the library's REG tables are compared with the indices the object's srsran_regs_t holds.
 *   CTRL_BIND_SEARCH=1   srsran_pdcch_extract_llr keeps the region's rows of the grids; srsran_pdcch_decode_msg decodes its candidate a second time through
 *                        srsran_hip_pdcch_search_sf and requires the same result bytes.
 *   CTRL_BIND_REPORT=1   one [ctrl_bind] line at exit.
 *   CTRL_BIND_DUMP=file  the inputs of the first call whose correlation or soft bits exceed their tolerance are written there.
 * The counters and the kept rows are plain statics: the programs call these functions from one thread. */
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "srsran/phy/ch_estimation/chest_dl.h"
#include "srsran/phy/phch/dci.h"
#include "srsran/phy/phch/pcfich.h"
#include "srsran/phy/phch/pdcch.h"
#include "srsran/phy/phch/phich.h"
#include "srsran/phy/phch/regs.h"
#include "srsran/phy/utils/debug.h"

/* include/srsran_amd/phy_conv_abi.h (declared by hand: that header declares srsran_viterbi_t, which is the reference's own here) */
typedef struct {
  uint32_t cell_nof_prb, cell_nof_ports, cell_id, cp_nsymb, phich_length, phich_resources, phich_mi, mbsfn_or_sf1_6_tdd, cfi, sf_idx, nof_rx;
} srsran_hip_pdcch_sf_t;
typedef struct {
  uint32_t ncce, L, nof_bits;
} srsran_hip_pdcch_cand_t;
typedef struct {
  uint8_t  payload[128 + 16];
  uint16_t crc_rem, decoded;
  float    mean;
} srsran_hip_pdcch_res_t;
typedef struct {
  uint32_t ngroup, nseq;
} srsran_hip_phich_resource_t;
typedef struct {
  uint32_t ack_value;
  float    distance, bits[3];
  cf_t     z[3];
} srsran_hip_phich_res_t;
extern int srsran_hip_regs_pdcch_nregs(const srsran_hip_pdcch_sf_t*);
extern int srsran_hip_regs_pdcch_table(const srsran_hip_pdcch_sf_t*, uint32_t*);
extern int srsran_hip_regs_pcfich_table(const srsran_hip_pdcch_sf_t*, uint32_t[16]);
extern int srsran_hip_regs_phich_ngroups(const srsran_hip_pdcch_sf_t*);
extern int srsran_hip_regs_phich_table(const srsran_hip_pdcch_sf_t*, uint32_t, uint32_t[12]);
extern int srsran_hip_pcfich_decode(const srsran_hip_pdcch_sf_t*, cf_t* const[], cf_t* const (*)[SRSRAN_MAX_PORTS], float, uint32_t*, float*);
extern int srsran_hip_phich_decode_multi(const srsran_hip_pdcch_sf_t*, cf_t* const[], cf_t* const (*)[SRSRAN_MAX_PORTS], float, uint32_t,
                                         const srsran_hip_phich_resource_t*, srsran_hip_phich_res_t*);
extern int srsran_hip_pdcch_extract_llr(const srsran_hip_pdcch_sf_t*, cf_t* const[], cf_t* const (*)[SRSRAN_MAX_PORTS], float, float*);
extern int srsran_hip_pdcch_dci_decode_multi(const float*, uint32_t, uint32_t, const srsran_hip_pdcch_cand_t*, srsran_hip_pdcch_res_t*);
extern int srsran_hip_pdcch_search_sf(const srsran_hip_pdcch_sf_t*, cf_t* const[], cf_t* const (*)[SRSRAN_MAX_PORTS], float, uint32_t,
                                      const srsran_hip_pdcch_cand_t*, srsran_hip_pdcch_res_t*);

/* the originals, renamed in the object files */
extern int srsran_pcfich_decode_ref(srsran_pcfich_t*, srsran_dl_sf_cfg_t*, srsran_chest_dl_res_t*, cf_t* [SRSRAN_MAX_PORTS], float*);
extern int srsran_phich_decode_ref(srsran_phich_t*, srsran_dl_sf_cfg_t*, srsran_chest_dl_res_t*, srsran_phich_resource_t, cf_t* [SRSRAN_MAX_PORTS], srsran_phich_res_t*);
extern int srsran_pdcch_extract_llr_ref(srsran_pdcch_t*, srsran_dl_sf_cfg_t*, srsran_chest_dl_res_t*, cf_t* [SRSRAN_MAX_PORTS]);
extern int srsran_pdcch_decode_msg_ref(srsran_pdcch_t*, srsran_dl_sf_cfg_t*, srsran_dci_cfg_t*, srsran_dci_msg_t*);

/* ---- counters, switches, the report */
enum { PCFICH, PHICH, LLR, MSG, SEARCH, NFUN };
static const char* fun_name[NFUN] = {"pcfich_decode", "phich_decode", "extract_llr", "decode_msg", "search"};
static unsigned    n_dev[NFUN], n_ref[NFUN], n_bad[NFUN], n_tables, n_tables_bad;
static double      worst_corr, worst_distance, worst_llr;
static double      tol_corr = INFINITY, tol_distance = INFINITY, tol_llr = INFINITY; /* no tolerance handed over: floats are reported, not judged */
static bool        check, search_on;
static const char* dump_path;

static void distance_close(void);

static void report(void)
{
  distance_close();
  fprintf(stderr, "[ctrl_bind]");
  for (int f = 0; f < NFUN; f++) {
    fprintf(stderr, " %s dev %u ref %u bad %u |", fun_name[f], n_dev[f], n_ref[f], n_bad[f]);
  }
  fprintf(stderr, " tables %u bad %u | corr %.3g distance %.3g llr %.3g\n", n_tables, n_tables_bad, worst_corr, worst_distance, worst_llr);
}

/* runs when the program is loaded, so that a program that reaches none of the four functions (pbch_test: the decoder handle only) reports too */
__attribute__((constructor)) static void arm(void)
{
  static bool armed;
  if (armed) {
    return;
  }
  armed     = true;
  check     = getenv("CTRL_BIND_CHECK") != NULL;
  search_on = getenv("CTRL_BIND_SEARCH") != NULL;
  dump_path = getenv("CTRL_BIND_DUMP");
  if (getenv("CTRL_BIND_TOL_CORR")) {
    tol_corr = atof(getenv("CTRL_BIND_TOL_CORR"));
  }
  if (getenv("CTRL_BIND_TOL_DISTANCE")) {
    tol_distance = atof(getenv("CTRL_BIND_TOL_DISTANCE"));
  }
  if (getenv("CTRL_BIND_TOL_LLR")) {
    tol_llr = atof(getenv("CTRL_BIND_TOL_LLR"));
  }
  if (getenv("CTRL_BIND_REPORT")) {
    atexit(report);
  }
}

static void bad(int f, const srsran_hip_pdcch_sf_t* d, const char* what, double a, double b)
{
  if (n_bad[f]++ < 8) {
    fprintf(stderr, "[ctrl_bind] MISMATCH %s %s: device %.9g reference %.9g (prb %u ports %u id %u cp %u len %u ng %u mi %u mbsfn %u cfi %u sf %u rx %u)\n",
            fun_name[f], what, a, b, d->cell_nof_prb, d->cell_nof_ports, d->cell_id, d->cp_nsymb, d->phich_length, d->phich_resources, d->phich_mi,
            d->mbsfn_or_sf1_6_tdd, d->cfi, d->sf_idx, d->nof_rx);
  }
}

/* ---- the description of the control region, from what the objects hold */
static srsran_hip_pdcch_sf_t describe(const srsran_cell_t* cell, const srsran_regs_t* regs, uint32_t cfi, uint32_t tti, uint32_t nof_rx)
{
  srsran_hip_pdcch_sf_t d = {.cell_nof_prb    = cell->nof_prb,
                             .cell_nof_ports  = cell->nof_ports,
                             .cell_id         = cell->id,
                             .cp_nsymb        = SRSRAN_CP_NSYMB(cell->cp),
                             .phich_length    = regs->phich_len == SRSRAN_PHICH_EXT ? 1 : 0,
                             .phich_resources = (uint32_t)regs->phich_res,
                             .phich_mi        = regs->phich_mi,
                             .cfi             = cfi,
                             .sf_idx          = tti % 10,
                             .nof_rx          = nof_rx};
  /* srsran_regs_t does not store the mbsfn_or_sf1_6_tdd it was initialised with.  It is derived from the map: the flag only matters with the extended PHICH
   * length, where without it the third REG of every mapping unit lies on symbol 2 (regs.c:334, li = i) and with it every REG lies on symbol 0 or 1
   * (regs.c:332) -- so the flag was set when the extended length has no PHICH REG on symbol 2. */
  if (d.phich_length == 1 && regs->phich_mi > 0 && regs->phich) {
    const uint32_t units = SRSRAN_CP_ISEXT(regs->cell.cp) ? regs->ngroups_phich / 2 : regs->ngroups_phich;
    bool           on_2  = false;
    for (uint32_t u = 0; u < units; u++) {
      for (uint32_t i = 0; i < regs->phich[u].nof_regs; i++) {
        on_2 = on_2 || regs->phich[u].regs[i]->l == 2;
      }
    }
    d.mbsfn_or_sf1_6_tdd = units > 0 && !on_2;
  }
  return d;
}

static uint32_t reg_re(const srsran_regs_reg_t* r, uint32_t i, uint32_t nof_prb)
{
  return r->k[i] + r->l * nof_prb * SRSRAN_NRE;
}

/* once per distinct map: the library's tables against the indices of the object's srsran_regs_t, in the order srsran_regs_*_get reads them.  Host only. */
static void check_tables(const srsran_hip_pdcch_sf_t* desc, const srsran_regs_t* regs)
{
  static srsran_hip_pdcch_sf_t* seen;
  static size_t                 n_seen, cap;
  srsran_hip_pdcch_sf_t         key = *desc;
  key.cfi = key.sf_idx = key.nof_rx = 0;
  if (n_seen && !memcmp(&seen[n_seen - 1], &key, sizeof(key))) {
    return;
  }
  for (size_t i = 0; i < n_seen; i++) {
    if (!memcmp(&seen[i], &key, sizeof(key))) {
      return;
    }
  }
  if (n_seen == cap) {
    cap  = cap ? 2 * cap : 64;
    seen = realloc(seen, cap * sizeof(*seen));
    if (!seen) {
      abort();
    }
  }
  seen[n_seen++] = key;
  n_tables++;

  const uint32_t        prb = regs->cell.nof_prb;
  unsigned              wrong = 0;
  srsran_hip_pdcch_sf_t d     = *desc;
  d.cfi                       = 1;
  uint32_t t16[16], t12[12];
  if (srsran_hip_regs_pcfich_table(&d, t16) != 16) {
    wrong++;
  } else {
    for (uint32_t i = 0; i < REGS_PCFICH_NREGS; i++) {
      for (uint32_t j = 0; j < REGS_RE_X_REG; j++) {
        wrong += t16[4 * i + j] != reg_re(regs->pcfich.regs[i], j, prb);
      }
    }
  }
  const uint32_t ngroups = regs->phich_mi > 0 ? regs->ngroups_phich : 0;
  if (srsran_hip_regs_phich_ngroups(&d) != (int)ngroups) {
    wrong++;
  } else {
    for (uint32_t g = 0; g < ngroups; g++) {
      const srsran_regs_ch_t* ch = &regs->phich[SRSRAN_CP_ISEXT(regs->cell.cp) ? g / 2 : g];
      if (srsran_hip_regs_phich_table(&d, g, t12) != 12) {
        wrong++;
        continue;
      }
      for (uint32_t i = 0; i < REGS_PHICH_REGS_X_GROUP; i++) {
        for (uint32_t j = 0; j < REGS_RE_X_REG; j++) {
          wrong += t12[4 * i + j] != reg_re(ch->regs[i], j, prb);
        }
      }
    }
  }
  for (uint32_t cfi = 1; cfi <= 3; cfi++) {
    d.cfi                      = cfi;
    const srsran_regs_ch_t* ch = &regs->pdcch[cfi - 1];
    uint32_t*               t  = malloc((size_t)4 * (ch->nof_regs + 9) * sizeof(uint32_t)); /* nof_regs: whole CCEs (regs.c:128) */
    if (!t) {
      abort();
    }
    if (srsran_hip_regs_pdcch_nregs(&d) != (int)ch->nof_regs || srsran_hip_regs_pdcch_table(&d, t) != (int)ch->nof_regs) {
      wrong++;
    } else {
      for (uint32_t i = 0; i < ch->nof_regs; i++) {
        for (uint32_t j = 0; j < REGS_RE_X_REG; j++) {
          wrong += t[4 * i + j] != reg_re(ch->regs[i], j, prb);
        }
      }
    }
    free(t);
  }
  if (wrong) {
    if (n_tables_bad++ < 8) {
      fprintf(stderr, "[ctrl_bind] MISMATCH tables: %u entries differ (prb %u ports %u id %u cp %u len %u ng %u mi %u mbsfn %u)\n", wrong, d.cell_nof_prb,
              d.cell_nof_ports, d.cell_id, d.cp_nsymb, d.phich_length, d.phich_resources, d.phich_mi, d.mbsfn_or_sf1_6_tdd);
    }
  }
}

/* the inputs of one call, for the float64 model: the description, the noise estimate, then per receive antenna the grid's first `rows` symbols followed
 * by each port's estimate rows */
static void dump_call(const char* what, const srsran_hip_pdcch_sf_t* d, const srsran_chest_dl_res_t* ch, cf_t* const sf_symbols[], uint32_t rows, const uint32_t extra[2])
{
  static bool done;
  if (done || !dump_path) {
    return;
  }
  done    = true;
  FILE* f = fopen(dump_path, "wb");
  if (!f) {
    return;
  }
  char           tag[16] = {0};
  const uint32_t n       = rows * 12 * d->cell_nof_prb;
  strncpy(tag, what, sizeof(tag) - 1);
  fwrite(tag, 1, sizeof(tag), f);
  fwrite(d, sizeof(*d), 1, f);
  fwrite(&ch->noise_estimate, sizeof(float), 1, f);
  fwrite(&rows, sizeof(rows), 1, f);
  fwrite(extra, sizeof(uint32_t), 2, f);
  for (uint32_t a = 0; a < d->nof_rx; a++) {
    fwrite(sf_symbols[a], sizeof(cf_t), n, f);
    for (uint32_t p = 0; p < d->cell_nof_ports; p++) {
      fwrite(ch->ce[p][a], sizeof(cf_t), n, f);
    }
  }
  fclose(f);
  fprintf(stderr, "[ctrl_bind] the inputs of this %s call are in %s\n", what, dump_path);
}

static double rel1(double a, double ref) /* the records' measure on a set of one: |a - ref| / rms(ref) */
{
  return ref != 0 ? fabs(a - ref) / fabs(ref) : (a != 0 ? 1.0 : 0.0);
}

/* ---- pcfich.c:156 */
int srsran_pcfich_decode(srsran_pcfich_t* q, srsran_dl_sf_cfg_t* sf, srsran_chest_dl_res_t* channel, cf_t* sf_symbols[SRSRAN_MAX_PORTS], float* corr_result)
{
  if (!q || !sf_symbols || !sf || !channel) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  arm();
  const srsran_hip_pdcch_sf_t d = describe(&q->cell, q->regs, 1, sf->tti, q->nof_rx_antennas); /* the call does not read cfi: it is what comes out */
  uint32_t                    cfi  = 0;
  float                       corr = 0;
  const int                   r    = srsran_hip_pcfich_decode(&d, sf_symbols, channel->ce, channel->noise_estimate, &cfi, &corr);
  if (r == SRSRAN_ERROR_INVALID_INPUTS) {
    n_ref[PCFICH]++;
    return srsran_pcfich_decode_ref(q, sf, channel, sf_symbols, corr_result);
  }
  n_dev[PCFICH]++;
  if (r < 0) {
    return SRSRAN_ERROR;
  }
  if (check) {
    check_tables(&d, q->regs);
    srsran_dl_sf_cfg_t sf2   = *sf;
    float              corr2 = 0;
    const int          r2    = srsran_pcfich_decode_ref(q, &sf2, channel, sf_symbols, &corr2);
    if (r2 != r || sf2.cfi != cfi) {
      bad(PCFICH, &d, "cfi", cfi, sf2.cfi);
    }
    const double dev = rel1(corr, corr2);
    worst_corr       = dev > worst_corr ? dev : worst_corr;
    if (!(dev <= tol_corr)) {
      bad(PCFICH, &d, "corr", corr, corr2);
      dump_call("pcfich", &d, channel, sf_symbols, 1, (uint32_t[2]){0, 0});
    }
  }
  sf->cfi = cfi;
  if (corr_result) {
    *corr_result = corr;
  }
  return r;
}

/* The PHICH's distance is measured as the record measures it (float_devs of tests/test_ctrl_golden.py): the largest |device - reference| over the resources of
 * ONE subframe, over the rms of the reference's distances of that subframe -- a capture's distance can be the small remainder of three soft bits of mixed sign,
 * and its own magnitude is no scale for a rounding difference.  The calls of one subframe are those in a row with the same description, tti and grid; the set
 * is judged when the next one begins and at exit. */
static struct {
  bool                  open;
  srsran_hip_pdcch_sf_t d;
  uint32_t              tti;
  const void*           grid;
  double                worst, sq;
  unsigned              n;
} dist_set;

static void distance_close(void)
{
  if (!dist_set.open) {
    return;
  }
  dist_set.open    = false;
  const double rms = sqrt(dist_set.sq / dist_set.n), dev = rms > 0 ? dist_set.worst / rms : (dist_set.worst != 0 ? 1.0 : 0.0);
  worst_distance   = dev > worst_distance || isnan(dev) ? dev : worst_distance;
  if (!(dev <= tol_distance)) {
    bad(PHICH, &dist_set.d, "distance over the subframe's rms", dev, tol_distance);
  }
}

static void distance_add(const srsran_hip_pdcch_sf_t* d, uint32_t tti, const void* grid, double mine, double theirs)
{
  if (dist_set.open && (memcmp(&dist_set.d, d, sizeof(*d)) || dist_set.tti != tti || dist_set.grid != grid)) {
    distance_close();
  }
  if (!dist_set.open) {
    dist_set.open  = true;
    dist_set.d     = *d;
    dist_set.tti   = tti;
    dist_set.grid  = grid;
    dist_set.worst = dist_set.sq = 0;
    dist_set.n                   = 0;
  }
  const double dd = fabs(mine - theirs);
  dist_set.worst  = dd > dist_set.worst || isnan(dd) ? dd : dist_set.worst;
  dist_set.sq += theirs * theirs;
  dist_set.n++;
}

/* ---- phich.c:181 */
int srsran_phich_decode(srsran_phich_t* q, srsran_dl_sf_cfg_t* sf, srsran_chest_dl_res_t* channel, srsran_phich_resource_t n_phich, cf_t* sf_symbols[SRSRAN_MAX_PORTS],
                        srsran_phich_res_t* result)
{
  if (!q || !sf_symbols || !sf || !channel) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  arm();
  const srsran_hip_pdcch_sf_t       d   = describe(&q->cell, q->regs, 1, sf->tti, q->nof_rx_antennas);
  const srsran_hip_phich_resource_t res = {.ngroup = n_phich.ngroup, .nseq = n_phich.nseq};
  srsran_hip_phich_res_t            out;
  const int                         r = srsran_hip_phich_decode_multi(&d, sf_symbols, channel->ce, channel->noise_estimate, 1, &res, &out);
  if (r == SRSRAN_ERROR_INVALID_INPUTS) {
    n_ref[PHICH]++;
    return srsran_phich_decode_ref(q, sf, channel, n_phich, sf_symbols, result);
  }
  n_dev[PHICH]++;
  if (r != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  if (check) {
    check_tables(&d, q->regs);
    srsran_phich_res_t r2 = {0};
    const int          e2 = srsran_phich_decode_ref(q, sf, channel, n_phich, sf_symbols, &r2);
    if (e2 != SRSRAN_SUCCESS || (uint32_t)r2.ack_value != out.ack_value) {
      bad(PHICH, &d, "ack_value", out.ack_value, e2 != SRSRAN_SUCCESS ? -1.0 : (double)r2.ack_value);
    }
    distance_add(&d, sf->tti, sf_symbols[0], out.distance, r2.distance);
  }
  if (result) {
    result->ack_value = out.ack_value != 0;
    result->distance  = out.distance;
  }
  return SRSRAN_SUCCESS;
}

/* ---- pdcch.c:424.  CTRL_BIND_SEARCH keeps the region's rows of every plane of the last subframe */
static struct {
  const srsran_pdcch_t* q;
  srsran_hip_pdcch_sf_t d;
  float                 noise;
  cf_t*                 rows; /* the planes one behind the other: [rx][1 + port] */
  size_t                cap;
  cf_t*                 sym[SRSRAN_MAX_PORTS];
  cf_t*                 ce[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS];
} kept;

static void keep(const srsran_pdcch_t* q, const srsran_hip_pdcch_sf_t* d, const srsran_chest_dl_res_t* ch, cf_t* const sf_symbols[])
{
  const size_t n = (size_t)(d->cfi + (d->cell_nof_prb <= 10 ? 1 : 0)) * 12 * d->cell_nof_prb, planes = (size_t)d->nof_rx * (1 + d->cell_nof_ports);
  if (kept.cap < n * planes) {
    free(kept.rows);
    kept.rows = malloc(n * planes * sizeof(cf_t));
    kept.cap  = kept.rows ? n * planes : 0;
  }
  kept.q = NULL;
  if (!kept.rows) {
    return;
  }
  cf_t* w = kept.rows;
  memset(kept.sym, 0, sizeof(kept.sym));
  memset(kept.ce, 0, sizeof(kept.ce));
  for (uint32_t a = 0; a < d->nof_rx; a++) {
    memcpy(w, sf_symbols[a], n * sizeof(cf_t));
    kept.sym[a] = w;
    w += n;
    for (uint32_t p = 0; p < d->cell_nof_ports; p++) {
      memcpy(w, ch->ce[p][a], n * sizeof(cf_t));
      kept.ce[p][a] = w;
      w += n;
    }
  }
  kept.q     = q;
  kept.d     = *d;
  kept.noise = ch->noise_estimate;
}

int srsran_pdcch_extract_llr(srsran_pdcch_t* q, srsran_dl_sf_cfg_t* sf, srsran_chest_dl_res_t* channel, cf_t* sf_symbols[SRSRAN_MAX_PORTS])
{
  if (!q || !sf || !channel || !sf_symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  arm();
  kept.q = NULL;
  if (sf->cfi < 1 || sf->cfi > 3) {
    return SRSRAN_ERROR_INVALID_INPUTS; /* :435 */
  }
  const srsran_hip_pdcch_sf_t d      = describe(&q->cell, q->regs, sf->cfi, sf->tti, q->nof_rx_antennas);
  const uint32_t              e_bits = 72 * q->nof_cce[sf->cfi - 1];
  memset(q->llr, 0, q->max_bits * sizeof(float)); /* :439 */
  const int r = e_bits <= q->max_bits ? srsran_hip_pdcch_extract_llr(&d, sf_symbols, channel->ce, channel->noise_estimate, q->llr) : SRSRAN_ERROR_INVALID_INPUTS;
  if (r == SRSRAN_ERROR_INVALID_INPUTS) {
    n_ref[LLR]++;
    return srsran_pdcch_extract_llr_ref(q, sf, channel, sf_symbols);
  }
  n_dev[LLR]++;
  if (r != (int)e_bits) {
    if (r >= 0) {
      bad(LLR, &d, "soft-bit count", r, e_bits);
    }
    return SRSRAN_ERROR;
  }
  if (check) {
    check_tables(&d, q->regs);
    float* mine = malloc(2 * (size_t)q->max_bits * sizeof(float));
    if (!mine) {
      abort();
    }
    float* theirs = mine + q->max_bits;
    memcpy(mine, q->llr, q->max_bits * sizeof(float));
    const int e2 = srsran_pdcch_extract_llr_ref(q, sf, channel, sf_symbols);
    memcpy(theirs, q->llr, q->max_bits * sizeof(float));
    memcpy(q->llr, mine, q->max_bits * sizeof(float));
    if (e2 != SRSRAN_SUCCESS) {
      bad(LLR, &d, "return value", SRSRAN_SUCCESS, e2);
    }
    double worst = 0, sq = 0; /* rel_dev of tests/test_pdcch_sf_golden.py: max |a - b| / rms(b), over the region's soft bits */
    for (uint32_t i = 0; i < e_bits; i++) {
      const double dd = fabs((double)mine[i] - (double)theirs[i]);
      worst           = dd > worst || isnan(dd) ? dd : worst;
      sq += (double)theirs[i] * (double)theirs[i];
    }
    const double rms = sqrt(sq / e_bits), dev = rms > 0 ? worst / rms : (worst != 0 ? 1.0 : 0.0);
    worst_llr = dev > worst_llr || isnan(dev) ? dev : worst_llr;
    if (!(dev <= tol_llr)) {
      bad(LLR, &d, "soft bits over rms", dev, tol_llr);
      dump_call("extract_llr", &d, channel, sf_symbols, d.cfi + (d.cell_nof_prb <= 10 ? 1 : 0), (uint32_t[2]){0, 0});
    }
    free(mine);
  }
  if (search_on) {
    keep(q, &d, channel, sf_symbols);
  }
  return SRSRAN_SUCCESS;
}

/* ---- pdcch.c:376: the location check, the size of the format and the 0 / 1A differentiation stay the reference's; the candidate's mean rule, rate de-matching,
 * decoder and CRC are one device call on q->llr */
int srsran_pdcch_decode_msg(srsran_pdcch_t* q, srsran_dl_sf_cfg_t* sf, srsran_dci_cfg_t* dci_cfg, srsran_dci_msg_t* msg)
{
  arm();
  if (!q || !msg || !sf || !dci_cfg || !srsran_dci_location_isvalid(&msg->location)) {
    if (msg) {
      ERROR("Invalid parameters, location=%d,%d", msg->location.ncce, msg->location.L);
    }
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t nof_cce = (sf->cfi > 0 && sf->cfi < 4) ? q->nof_cce[sf->cfi - 1] : 0;
  if (msg->location.ncce * 72 + (72u << msg->location.L) > nof_cce * 72) {
    ERROR("Invalid location: nCCE: %d, L: %d, NofCCE: %d", msg->location.ncce, msg->location.L, nof_cce);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const srsran_hip_pdcch_sf_t   d    = describe(&q->cell, q->regs, sf->cfi, sf->tti, q->nof_rx_antennas);
  const srsran_hip_pdcch_cand_t cand = {.ncce = msg->location.ncce, .L = msg->location.L, .nof_bits = srsran_dci_format_sizeof(&q->cell, sf, dci_cfg, msg->format)};
  srsran_hip_pdcch_res_t        res;
  const srsran_dci_msg_t        before = *msg;
  const int                     r      = srsran_hip_pdcch_dci_decode_multi(q->llr, 72 * nof_cce, 1, &cand, &res);
  if (r == SRSRAN_ERROR_INVALID_INPUTS) {
    n_ref[MSG]++;
    return srsran_pdcch_decode_msg_ref(q, sf, dci_cfg, msg);
  }
  n_dev[MSG]++;
  if (r < 0) {
    ERROR("Error calling pdcch_dci_decode");
    return SRSRAN_ERROR;
  }
  if (res.decoded) { /* mean > 0.3 (:393) */
    const uint32_t n = cand.nof_bits + 16 < sizeof(msg->payload) ? cand.nof_bits + 16 : sizeof(msg->payload);
    memcpy(msg->payload, res.payload, n); /* the reference's decoder leaves the 16 CRC bits behind the payload too */
    msg->rnti     = res.crc_rem;
    msg->nof_bits = cand.nof_bits;
    if (msg->format == SRSRAN_DCI_FORMAT0 || msg->format == SRSRAN_DCI_FORMAT1A) { /* :398 */
      msg->format = (msg->payload[dci_cfg->cif_enabled ? 3 : 0] == 0) ? SRSRAN_DCI_FORMAT0 : SRSRAN_DCI_FORMAT1A;
    }
  }
  if (check) {
    srsran_dci_msg_t m2 = before;
    const int        e2 = srsran_pdcch_decode_msg_ref(q, sf, dci_cfg, &m2); /* on the same q->llr */
    if (e2 != SRSRAN_SUCCESS) {
      bad(MSG, &d, "return value", SRSRAN_SUCCESS, e2);
    } else if (m2.nof_bits != msg->nof_bits) {
      bad(MSG, &d, "nof_bits", msg->nof_bits, m2.nof_bits);
    } else if (m2.rnti != msg->rnti) {
      bad(MSG, &d, "rnti", msg->rnti, m2.rnti);
    } else if (m2.format != msg->format) {
      bad(MSG, &d, "format", msg->format, m2.format);
    } else if (memcmp(m2.payload, msg->payload, sizeof(msg->payload))) {
      uint32_t i = 0;
      while (m2.payload[i] == msg->payload[i]) {
        i++;
      }
      bad(MSG, &d, "payload, first differing bit", i, i);
    }
  }
  if (search_on) {
    if (kept.q != q || kept.d.cfi != d.cfi || kept.d.sf_idx != d.sf_idx) {
      n_ref[SEARCH]++; /* no subframe kept for this object: nothing to search from */
    } else {
      srsran_hip_pdcch_res_t res2;
      const int              s = srsran_hip_pdcch_search_sf(&kept.d, kept.sym, kept.ce, kept.noise, 1, &cand, &res2);
      if (s == SRSRAN_ERROR_INVALID_INPUTS) {
        n_ref[SEARCH]++;
      } else {
        n_dev[SEARCH]++;
        if (s < 0 || memcmp(&res, &res2, sizeof(res))) {
          bad(SEARCH, &d, s < 0 ? "return value" : "result bytes (mean shown)", s < 0 ? s : res2.mean, s < 0 ? 0 : res.mean);
        }
      }
    }
  }
  return SRSRAN_SUCCESS;
}
