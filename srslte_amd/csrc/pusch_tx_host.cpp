// pusch_tx_host.cpp -- PUSCH transmit in one device call, with or without control information (include/srsran_amd/phy_chan_abi.h: srsran_hip_pusch_encode,
// _dbg, srsran_hip_ulsch_encode_uci): srsran_pusch_encode (pusch.c:259-354) chained on the calling thread's transport-block stream.  Behind the coding pass
// (G Qm bits, the coder's own layout) two launches: the multiplexer + scrambler + fix-up + modulator (pusch_tx_kernels.hip) and the forward transform of
// 12 L_prb points per SC-FDMA symbol, whose rows land in the pinned image; after the one host wait they are copied to the caller's grid in pusch_put's order.
#include "chan_internal.h"
#include "modem_device.h"
#include "pusch_tx_device.h"

using namespace phyhip;
using namespace phyhip::chan;

namespace {

struct TxCall {
  const char*                      who;
  srsran_hip_grant_tb_t            tb;
  uint32_t                         rows, cols;
  uint32_t                         L_prb; // 0: srsran_ulsch_encode's level -- unscrambled bits, no points, no transform
  srsran_hip_pusch_uci_t           u;
  const srsran_hip_pusch_uci_in_t* in;
  srsran_softbuffer_tx_t*          sb;
  uint8_t*                         data;
  bool                             want_q, want_d;
  // out: where the results are in the thread's pinned image after the call
  const uint8_t *z = nullptr, *q = nullptr, *d = nullptr;
};

// the control-information part of the checks; nullptr when the grant can be taken
const char* uci_refusal(const TxCall& c)
{
  const uint32_t                   Qm = qm_of(c.tb.mod);
  const srsran_hip_pusch_uci_t&    u  = c.u;
  const srsran_hip_pusch_uci_in_t* in = c.in;
  if (u.Q_prime_ack > 4 * c.rows || u.Q_prime_ri > 4 * c.rows) {
    return "more ACK / RI symbols than four columns hold";
  }
  if ((u.Q_prime_ack || u.Q_prime_ri) && c.cols < 9) {
    return "ACK / RI columns need at least 9 SC-FDMA symbols";
  }
  if ((uint64_t)u.Q_prime_ri + u.Q_prime_cqi >= c.tb.nof_re) {
    return "RI and CQI leave no symbol for the transport block";
  }
  if ((u.Q_prime_ack | u.Q_prime_ri | u.Q_prime_cqi) &&
      (!in || (u.Q_prime_ack && !in->ack_type) || (u.Q_prime_ri && !in->ri_type) || (u.Q_prime_cqi && !in->cqi_bits))) {
    return "no input array for a non-zero count";
  }
  for (size_t i = 0; i < (size_t)u.Q_prime_ack * Qm; i++) {
    if (in->ack_type[i] > 3) {
      return "an ACK type byte above 3";
    }
  }
  for (size_t i = 0; i < (size_t)u.Q_prime_ri * Qm; i++) {
    if (in->ri_type[i] > 3) {
      return "an RI type byte above 3";
    }
  }
  for (size_t i = 0; i < (size_t)u.Q_prime_cqi * Qm; i++) {
    if (in->cqi_bits[i] > 1) {
      return "a CQI bit above 1";
    }
  }
  return nullptr;
}

// behind the checks: staging, the coding pass, the two launches, the downloads _dbg asked for, one host wait
int run(TxCall& c)
{
  ChanStage* sp = stage_for(c.who);
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage&      s = *sp;
  srsran_cbsegm_t seg;
  if (!segment(&seg, c.tb.tbs)) {
    return SRSRAN_ERROR;
  }
  const uint32_t Qm = qm_of(c.tb.mod), n = c.tb.nof_re, Qa = c.u.Q_prime_ack, Qr = c.u.Q_prime_ri, Qc = c.u.Q_prime_cqi;
  const uint32_t G  = n - Qr - Qc;
  const bool     points = c.L_prb != 0;
  const size_t   nd = points ? al256((size_t)n * sizeof(cf_t)) : 0, nq = c.want_q ? al256((((size_t)n * Qm + 31) / 32) * 4) : 0;
  const size_t   nc = al256(pusch_tx::ctl_bytes(Qa, Qr, Qc, Qm));
  // pinned: [z | control image | q | d]; device: [d | q]
  const size_t o_z = 0, o_ctl = nd, o_q = o_ctl + nc, o_d = o_q + nq;
  if (!s.grow(o_d + (c.want_d ? nd : 0), nd + nq)) {
    fprintf(stderr, "[srsran_phy_hip] %s: staging allocation failed\n", c.who);
    return SRSRAN_ERROR;
  }
  srsran_hip_dft_batch_t* plan = points ? s.plan(c.L_prb, true) : nullptr;
  if (points && !plan) {
    return SRSRAN_ERROR;
  }
  uint8_t* ctl = s.pin + o_ctl;
  if (Qa) {
    memcpy(ctl, c.in->ack_type, (size_t)Qa * Qm);
  }
  if (Qr) {
    memcpy(ctl + (size_t)Qa * Qm, c.in->ri_type, (size_t)Qr * Qm);
  }
  if (Qc) {
    memcpy(ctl + (size_t)(Qa + Qr) * Qm, c.in->cqi_bits, (size_t)Qc * Qm);
  }
  uint8_t *          pin = s.pin, *dev = s.dev;
  const TxCall&      k    = c;
  const sch::BackEnd back = [=, &k](hipStream_t st, const uint8_t* d_e) {
    modem::Params sq;
    const float2* tab = modem::mod_tables();
    if (!modem::params_for(sq, modem::LLR_I16) || !tab) {
      return false;
    }
    pusch_tx::Params p = {};
    p.e_bits   = d_e;
    p.e_bytes  = (G * Qm + 7) / 8;
    p.ctl      = pin + o_ctl;
    p.d        = points ? reinterpret_cast<float2*>(dev) : nullptr;
    p.q_words  = k.want_q ? reinterpret_cast<uint32_t*>(dev + nd) : nullptr;
    p.table    = tab;
    p.mod      = k.tb.mod;
    p.n        = n;
    p.rows     = k.rows;
    p.cols     = k.cols;
    p.q_ack    = Qa;
    p.q_ri     = Qr;
    p.q_cqi    = Qc;
    p.seed     = k.tb.seed;
    p.scramble = points ? 1u : 0u;
    p.x1_bits  = sq.x1_bits;
    p.x2_cols  = sq.x2_cols;
    if ((k.want_q && hipMemsetAsync(dev + nd, 0, nq, st) != hipSuccess) || pusch_tx::launch_mux_mod(p, st) != hipSuccess) {
      set_error("%s: multiplexer launch failed", k.who);
      return false;
    }
    if ((k.want_q && hipMemcpyAsync(pin + o_q, dev + nd, ((size_t)n * Qm + 7) / 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (k.want_d && hipMemcpyAsync(pin + o_d, dev, (size_t)n * sizeof(cf_t), hipMemcpyDeviceToHost, st) != hipSuccess)) {
      set_error("%s: copy of the intermediate results failed", k.who);
      return false;
    }
    // srsran_dft_precoding, transmit: forward, normalised, one transform per SC-FDMA symbol; the rows land in the pinned image
    return !points || srsran_hip_dft_batch_run(plan, reinterpret_cast<const cf_t*>(dev), reinterpret_cast<cf_t*>(pin + o_z), k.cols, st) == SRSRAN_SUCCESS;
  };
  const int rc = sch::encode_tb_staged(c.sb, &seg, Qm, c.tb.rv, G * Qm, c.data, nullptr, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  c.z = s.pin + o_z;
  c.q = s.pin + o_q;
  c.d = s.pin + o_d;
  return SRSRAN_SUCCESS;
}

inline srsran_hip_pusch_uci_t counts_of(const srsran_hip_pusch_uci_t* uci)
{
  return uci ? *uci : srsran_hip_pusch_uci_t{0, 0, 0};
}

} // namespace

extern "C" int srsran_hip_pusch_encode_dbg(const srsran_hip_pusch_tx_t* g, const srsran_hip_pusch_uci_t* uci, const srsran_hip_pusch_uci_in_t* in,
                                           srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* sf_symbols, uint8_t* q_out, cf_t* d_out, cf_t* z_out)
{
  TraceRange        trace_("srsran_hip_pusch_encode");
  static const char who[] = "srsran_hip_pusch_encode";
  if (!g || !softbuffer || !sf_symbols) {
    return refuse("%s: NULL argument", who);
  }
  const srsran_hip_pusch_tx_t& x = *g;
  if (!tb_valid(x.tb, who)) { // (tbs == 0 -- a CQI-only grant -- among them)
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t nsymb = 2 * (x.cp_nsymb - 1) - (x.shortened ? 1u : 0u);
  if ((x.cp_nsymb != 7 && x.cp_nsymb != 6) || x.L_prb == 0 || !srsran_dft_precoding_valid_prb(x.L_prb) || x.n_prb_tilde[0] + x.L_prb > x.cell_nof_prb ||
      x.n_prb_tilde[1] + x.L_prb > x.cell_nof_prb || x.tb.nof_re != nsymb * 12 * x.L_prb || x.tb.mod < SRSRAN_MOD_QPSK || x.tb.mod > SRSRAN_MOD_64QAM) {
    return refuse("%s: allocation (%u PRB at %u / %u of %u, %u REs, mod %u) is not a PUSCH allocation", who, x.L_prb, x.n_prb_tilde[0], x.n_prb_tilde[1], x.cell_nof_prb,
                  x.tb.nof_re, x.tb.mod);
  }
  TxCall c = {who, x.tb, 12 * x.L_prb, nsymb, x.L_prb, counts_of(uci), in, softbuffer, data, q_out != nullptr, d_out != nullptr};
  if (const char* why = uci_refusal(c)) {
    return refuse("%s: (Q'ack %u, Q'ri %u, Q'cqi %u, %u PRB): %s", who, c.u.Q_prime_ack, c.u.Q_prime_ri, c.u.Q_prime_cqi, x.L_prb, why);
  }
  const int rc = run(c);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  // pusch.c:48-100 (pusch_put): row by row to the allocation's 12 L_prb sub-carriers of every symbol but the slot's reference symbol (and the SRS symbol)
  const uint32_t L_ref = x.cp_nsymb == 7 ? 3 : 2;
  const size_t   wid   = (size_t)x.L_prb * 12 * sizeof(cf_t);
  size_t         at    = 0;
  for (uint32_t slot = 0; slot < 2; slot++) {
    const uint32_t nl = x.cp_nsymb - ((x.shortened && slot == 1) ? 1u : 0u);
    for (uint32_t l = 0; l < nl; l++) {
      if (l == L_ref) {
        continue;
      }
      memcpy(sf_symbols + ((size_t)(l + slot * x.cp_nsymb) * x.cell_nof_prb + x.n_prb_tilde[slot]) * 12, c.z + at, wid);
      at += wid;
    }
  }
  if (z_out) {
    memcpy(z_out, c.z, (size_t)x.tb.nof_re * sizeof(cf_t));
  }
  if (d_out) {
    memcpy(d_out, c.d, (size_t)x.tb.nof_re * sizeof(cf_t));
  }
  if (q_out) {
    memcpy(q_out, c.q, ((size_t)x.tb.nof_re * qm_of(x.tb.mod) + 7) / 8);
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_pusch_encode(const srsran_hip_pusch_tx_t* g, const srsran_hip_pusch_uci_t* uci, const srsran_hip_pusch_uci_in_t* in,
                                       srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* sf_symbols)
{
  return srsran_hip_pusch_encode_dbg(g, uci, in, softbuffer, data, sf_symbols, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_ulsch_encode_uci(const srsran_hip_grant_tb_t* tbp, uint32_t nof_symb, const srsran_hip_pusch_uci_t* uci,
                                           const srsran_hip_pusch_uci_in_t* in, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, uint8_t* q_bits)
{
  TraceRange        trace_("srsran_hip_ulsch_encode");
  static const char who[] = "srsran_hip_ulsch_encode_uci";
  if (!tbp || !softbuffer || !q_bits) {
    return refuse("%s: NULL argument", who);
  }
  const srsran_hip_grant_tb_t tb = *tbp;
  if (!tb_valid(tb, who)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (nof_symb == 0 || tb.nof_re % nof_symb || tb.mod < SRSRAN_MOD_QPSK || tb.mod > SRSRAN_MOD_64QAM) {
    return refuse("%s: %u REs in %u columns, mod %u: not a PUSCH grant", who, tb.nof_re, nof_symb, tb.mod);
  }
  TxCall c = {who, tb, tb.nof_re / nof_symb, nof_symb, 0, counts_of(uci), in, softbuffer, data, true, false};
  if (const char* why = uci_refusal(c)) {
    return refuse("%s: (Q'ack %u, Q'ri %u, Q'cqi %u, %u rows): %s", who, c.u.Q_prime_ack, c.u.Q_prime_ri, c.u.Q_prime_cqi, c.rows, why);
  }
  const int rc = run(c);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  memcpy(q_bits, c.q, ((size_t)tb.nof_re * qm_of(tb.mod) + 7) / 8);
  return SRSRAN_SUCCESS;
}
