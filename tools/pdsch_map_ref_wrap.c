/* pdsch_map_ref_wrap.c -- the one exported wrapper tools/gen_golden_pdsch_map.py and tools/measure/pdsch_sf_time.py call: the reference's srsran_pdsch_get on the
 * planes of one subframe description.  The reference's source files are included where they lie (REF_PDSCH_C, REF_PRB_DL_C: their paths, given on the compiler's
 * command line; nothing of them is copied or committed) and the wrapper fills the fields srsran_pdsch_cp reads.  Built into a temporary directory with the
 * reference flags of oracle/Makefile and loaded lazily behind oracle/_ref/libsrsran_ref.so: the call binds nothing outside this object. */
#include REF_PDSCH_C
#include REF_PRB_DL_C

/* prb: [2][nof_prb] bytes.  Returns what srsran_pdsch_get returned for the last plane. */
int pdsch_map_ref_get(unsigned nof_prb, unsigned nof_ports, unsigned cell_id, unsigned cp_nsymb, unsigned frame_type, unsigned sf_idx, unsigned lstart,
                      unsigned nsymb0, unsigned nsymb1, const unsigned char* prb, unsigned n_planes, cf_t* const* grids, cf_t* const* planes)
{
  static srsran_pdsch_t q; /* (zero but for the cell: a large object, not cleared per call) */
  srsran_pdsch_grant_t  grant;
  int                   n = 0;
  memset(&grant, 0, sizeof(grant));
  q.cell.nof_prb         = nof_prb;
  q.cell.nof_ports       = nof_ports;
  q.cell.id              = cell_id;
  q.cell.cp              = cp_nsymb == 7 ? SRSRAN_CP_NORM : SRSRAN_CP_EXT;
  q.cell.frame_type      = frame_type ? SRSRAN_TDD : SRSRAN_FDD;
  grant.nof_symb_slot[0] = nsymb0;
  grant.nof_symb_slot[1] = nsymb1;
  for (unsigned s = 0; s < 2; s++) {
    for (unsigned k = 0; k < nof_prb; k++) {
      grant.prb_idx[s][k] = prb[s * nof_prb + k] != 0;
    }
  }
  for (unsigned p = 0; p < n_planes; p++) {
    n = srsran_pdsch_get(&q, grids[p], planes[p], &grant, lstart, sf_idx);
  }
  return n;
}
