/* csi_ref_wrap.c -- the one exported wrapper tools/gen_golden_csi.py calls: the reference's csi_correction is `static`, so its source file is included
 * where it lies (REF_PDSCH_C: its path, given on the compiler's command line; nothing of it is copied or committed) and the wrapper fills the four fields
 * the function reads.  Built into a temporary directory with the reference flags of oracle/Makefile and loaded lazily behind oracle/_ref/libsrsran_ref.so:
 * the call binds srsran_mod_bits_x_symbol and srsran_vec_max_fi only. */
#include REF_PDSCH_C

void csi_ref_correction(float* csi, void* e, int mod, unsigned nof_bits, int llr_is_8bit)
{
  srsran_pdsch_t     q;
  srsran_pdsch_cfg_t cfg;
  memset(&q, 0, sizeof(q));
  memset(&cfg, 0, sizeof(cfg));
  q.csi[0]              = csi;
  q.llr_is_8bit         = llr_is_8bit != 0;
  cfg.grant.tb[0].mod   = (srsran_mod_t)mod;
  cfg.grant.tb[0].nof_bits = (int)nof_bits;
  csi_correction(&q, &cfg, 0, 0, e);
}
