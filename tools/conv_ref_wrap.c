/* conv_ref_wrap.c -- the two exported wrappers tools/gen_golden_conv.py calls.  The reference's viterbi37_avx2_16bit.c is included where it lies
 * (REF_V37_C: its path, given on the compiler's command line; nothing of it is copied or committed), so that struct v37 can be read; viterbi.c, rm_conv.c
 * and pdcch.c (srsran_pdcch_dci_decode) are compiled from where they lie next to it, with the reference flags of oracle/Makefile, into a temporary
 * directory, and loaded lazily. */
/* the reference flags include debug.h in front of every file, whose DEBUG() macro would switch the decoder's own #ifdef DEBUG printing on */
#undef DEBUG
#include REF_V37_C

#include "srsran/phy/fec/convolutional/viterbi.h"
#include "srsran/phy/fec/crc.h"
#include "srsran/phy/phch/pdcch.h"

static void leave(srsran_viterbi_t* dec, uint32_t nsym, uint16_t* sym_out, uint32_t* best_state, uint16_t* metrics)
{
  struct v37* vp = (struct v37*)dec->ptr;
  /* zero further steps: the reference's own best-state rule on the metrics it left */
  update_viterbi37_blk_avx2_16bit(vp, dec->symbols_us, 0, best_state);
  memcpy(metrics, vp->old_metrics->c, 64 * sizeof(uint16_t));
  if (sym_out) {
    memcpy(sym_out, dec->symbols_us, nsym * sizeof(uint16_t));
  }
}

/* kind 0: srsran_viterbi_decode_f on float, 1: _decode_s on int16, 2: _decode_us on uint16.  gain_quant <= 0: the default is kept.
 * sym_out: the quantised symbols (kinds 0 and 1).  Returns what the decode call returned. */
int conv_ref_viterbi(int kind, int tail_biting, uint32_t framebits, uint32_t frame_length, float gain_quant, void* in, uint8_t* bits, uint16_t* sym_out,
                     uint32_t* best_state, uint16_t* metrics)
{
  int              poly[3] = {0x6D, 0x4F, 0x57};
  srsran_viterbi_t dec;
  if (srsran_viterbi_init(&dec, SRSRAN_VITERBI_37, poly, framebits, tail_biting != 0)) {
    return -100;
  }
  if (gain_quant > 0) {
    srsran_viterbi_set_gain_quant(&dec, gain_quant);
  }
  const uint32_t nsym = 3 * (frame_length + (tail_biting ? 0 : 6));
  int            rc;
  if (kind == 0) {
    rc = srsran_viterbi_decode_f(&dec, (float*)in, bits, frame_length);
  } else if (kind == 1) {
    rc = srsran_viterbi_decode_s(&dec, (int16_t*)in, bits, frame_length);
  } else {
    rc = srsran_viterbi_decode_us(&dec, (uint16_t*)in, bits, frame_length);
  }
  leave(&dec, nsym, kind == 2 ? NULL : sym_out, best_state, metrics);
  srsran_viterbi_free(&dec);
  return rc;
}

/* srsran_pdcch_dci_decode on the E soft bits of one candidate, on a srsran_pdcch_t that holds what srsran_pdcch_init_ gives the fields the call reads
 * (pdcch.c:73-139: the decoder over SRSRAN_DCI_MAX_BITS + 16 bits with tail biting, the 16-bit CRC; rm_f is a member).  rm_out: 3 (nof_bits + 16) de-matched floats;
 * sym_out: as many quantised symbols; bits: nof_bits + 16. */
int conv_ref_dci(float* e, uint32_t E, uint32_t nof_bits, float* rm_out, uint16_t* sym_out, uint8_t* bits, uint16_t* crc_rem, uint32_t* best_state,
                 uint16_t* metrics)
{
  int            poly[3] = {0x6D, 0x4F, 0x57};
  static srsran_pdcch_t q;
  memset(&q, 0, sizeof(q));
  q.max_bits = 6 * 72 * 100;
  if (srsran_crc_init(&q.crc, SRSRAN_LTE_CRC16, 16) || srsran_viterbi_init(&q.decoder, SRSRAN_VITERBI_37, poly, SRSRAN_DCI_MAX_BITS + 16, true)) {
    return -100;
  }
  int rc = srsran_pdcch_dci_decode(&q, e, bits, E, nof_bits, crc_rem);
  memcpy(rm_out, q.rm_f, 3 * (nof_bits + 16) * sizeof(float));
  leave(&q.decoder, 3 * (nof_bits + 16), sym_out, best_state, metrics);
  srsran_viterbi_free(&q.decoder);
  return rc;
}
