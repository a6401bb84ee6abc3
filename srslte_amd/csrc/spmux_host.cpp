// spmux_host.cpp -- spatial multiplexing and large-delay CDD on 2 ports with 2 receive antennas (include/srsran_amd/phy_modem_abi.h, phy_chan_abi.h;
// spmux_kernels.hip): the two stages on HOST buffers (one kernel each on the calling thread's stage) and on device buffers, and the PDSCH grant of one or
// two codewords in one call each way.
#include "chan_internal.h"
#include "spmux_device.h"

#include <cmath>
#include <vector>

using namespace phyhip;
using namespace phyhip::chan;

namespace {

// one of the three transmissions that are taken, as the kernels want it
struct Taken {
  spmux::Scheme rx;         // (mmse, noise: set by the receive side)
  uint32_t      tx_kind[2]; // TXPRE_* of an even / odd RE
  float         tx_scale;   // the reference's float factor of the precoder (precoding.c:2046, :2098, :2126, :2131, :2164)
};

// nullptr when (tx_scheme, layers, codebook_idx, n, scaling) is taken, else why not
const char* mimo_case(int tx_scheme, int layers, int codebook_idx, int64_t n, float scaling, Taken& t)
{
  if (!(scaling != 0.f) || !std::isfinite(scaling)) {
    return "scaling is 0 or not finite";
  }
  t = {};
  if (tx_scheme == SRSRAN_HIP_TXSCHEME_CDD) {
    if (layers != 2) {
      return "CDD is taken with 2 layers";
    }
    if (n & 1) {
      return "CDD needs an even number of REs";
    }
    t.rx       = {2, {modem::HEFF_PM, modem::HEFF_MP}, 0, 2.0f / scaling, 0.f};
    t.tx_kind[0] = modem::TXPRE_CDD;
    t.tx_kind[1] = modem::TXPRE_CDD + 1;
    t.tx_scale = scaling / 2.0f;
    return nullptr;
  }
  if (tx_scheme != SRSRAN_HIP_TXSCHEME_SPATIALMUX) {
    return "the scheme is neither spatial multiplexing nor CDD";
  }
  if (layers == 2) {
    if (codebook_idx < 0 || codebook_idx > 2) {
      return "codebook_idx is 0 .. 2 with 2 layers";
    }
    const uint32_t pre = codebook_idx == 0 ? modem::HEFF_IDENT : codebook_idx == 1 ? modem::HEFF_PM : modem::HEFF_J;
    t.rx = {2, {pre, pre}, 0, codebook_idx == 0 ? (float)M_SQRT2 / scaling : 2.0f / scaling, 0.f};
    t.tx_kind[0] = t.tx_kind[1] = modem::TXPRE_MUX2 + (uint32_t)codebook_idx;
    t.tx_scale = codebook_idx == 0 ? (float)(scaling * M_SQRT1_2) : scaling / 2.0f;
    return nullptr;
  }
  if (layers == 1) {
    if (codebook_idx < 0 || codebook_idx > 3) {
      return "codebook_idx is 0 .. 3 with 1 layer";
    }
    t.rx = {1, {(uint32_t)codebook_idx, (uint32_t)codebook_idx}, 0, (float)M_SQRT2 / scaling, 0.f};
    t.tx_kind[0] = t.tx_kind[1] = modem::TXPRE_MUX1 + (uint32_t)codebook_idx;
    t.tx_scale = (float)(scaling * M_SQRT1_2);
    return nullptr;
  }
  return "spatial multiplexing is taken with 1 or 2 layers";
}

// the receive side's own conditions on top
const char* mimo_rx_case(int tx_scheme, int layers, int codebook_idx, int64_t n, float scaling, int nof_rx, int decoder, float noise, Taken& t)
{
  if (nof_rx != 2) {
    return "2 receive antennas are taken";
  }
  if (decoder != SRSRAN_HIP_MIMO_DECODER_ZF && decoder != SRSRAN_HIP_MIMO_DECODER_MMSE) {
    return "the decoder is neither ZF nor MMSE";
  }
  if (!(noise >= 0.f) || !std::isfinite(noise)) {
    return "noise_estimate is negative or not finite";
  }
  const char* why = mimo_case(tx_scheme, layers, codebook_idx, n, scaling, t);
  t.rx.mmse       = decoder == SRSRAN_HIP_MIMO_DECODER_MMSE ? 1u : 0u;
  t.rx.noise      = noise;
  return why;
}

int refuse_stage(const char* who, const char* why, int tx_scheme, int ports, int layers, int codebook_idx, int n)
{
  return refuse("%s: %s (scheme %d, %d ports, %d layers, codebook_idx %d, %d REs)", who, why, tx_scheme, ports, layers, codebook_idx, n);
}

inline const float* fl(const cf_t* p)
{
  return reinterpret_cast<const float*>(p);
}
inline float* fl(cf_t* p)
{
  return reinterpret_cast<float*>(p);
}
inline bool al4(const void* p)
{
  return (reinterpret_cast<uintptr_t>(p) & 3u) == 0;
}

spmux::EqParams eq_params(const cf_t* const* y, const cf_t* const (*h)[SRSRAN_MAX_PORTS], cf_t* const* x, float* const* csi, uint32_t n, const spmux::Scheme& s)
{
  spmux::EqParams p = {};
  for (uint32_t r = 0; r < 2; r++) {
    p.y[r] = fl(y[r]);
    for (uint32_t k = 0; k < 2; k++) {
      p.h[k][r] = fl(h[k][r]);
    }
  }
  for (uint32_t k = 0; k < s.layers; k++) {
    p.x[k] = fl(x[k]);
  }
  // what the reference's scalar bodies write: two-layer ZF spatial multiplexing gets csi[0] only (precoding.c:1330-1331)
  const bool second = s.layers == 2 && (s.mmse || s.pre[0] != s.pre[1]);
  p.csi[0]          = csi ? csi[0] : nullptr;
  p.csi[1]          = (csi && csi[0] && second) ? csi[1] : nullptr;
  p.n               = n;
  p.s               = s;
  return p;
}

} // namespace

// ------------------------------------------------------------------------------------------------ the stages on device buffers

extern "C" int srsran_hip_predecoding_mimo_dev(const cf_t* const d_y[SRSRAN_MAX_PORTS], const cf_t* const d_h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS],
                                               cf_t* const d_x[SRSRAN_MAX_LAYERS], float* const d_csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_layers,
                                               int codebook_idx, int nof_symbols, int tx_scheme, float scaling, float noise_estimate, int decoder, void* stream)
{
  Taken       t;
  const char* why = nof_ports != 2 ? "2 ports are taken" : nof_symbols < 0 ? "a negative number of REs" : (!d_y || !d_h || !d_x) ? "NULL argument" : nullptr;
  why             = why ? why : mimo_rx_case(tx_scheme, nof_layers, codebook_idx, nof_symbols, scaling, nof_rxant, decoder, noise_estimate, t);
  for (uint32_t r = 0; !why && nof_symbols && r < 2; r++) {
    const bool ok = d_y[r] && al4(d_y[r]) && d_h[0][r] && al4(d_h[0][r]) && d_h[1][r] && al4(d_h[1][r]) && (r >= t.rx.layers || (d_x[r] && al4(d_x[r]))) &&
                    (!d_csi || al4(d_csi[r]));
    why           = ok ? nullptr : "a NULL or misaligned plane";
  }
  if (why) {
    return refuse_stage("srsran_hip_predecoding_mimo", why, tx_scheme, nof_ports, nof_layers, codebook_idx, nof_symbols);
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  PHY_HIP_CHECK(spmux::launch_eq(eq_params(d_y, d_h, d_x, d_csi, (uint32_t)nof_symbols, t.rx), (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_precoding_mimo_dev(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* const d_y[SRSRAN_MAX_PORTS], int nof_layers, int nof_ports,
                                             int codebook_idx, int nof_symbols, float scaling, int tx_scheme, void* stream)
{
  Taken       t;
  const char* why = nof_ports != 2 ? "2 ports are taken" : nof_symbols < 0 ? "a negative number of REs" : (!d_x || !d_y) ? "NULL argument" : nullptr;
  why             = why ? why : mimo_case(tx_scheme, nof_layers, codebook_idx, nof_symbols, scaling, t);
  for (uint32_t k = 0; !why && nof_symbols && k < 2; k++) {
    why = (d_y[k] && al4(d_y[k]) && (k >= t.rx.layers || (d_x[k] && al4(d_x[k])))) ? nullptr : "a NULL or misaligned plane";
  }
  if (why) {
    return refuse_stage("srsran_hip_precoding_mimo", why, tx_scheme, nof_ports, nof_layers, codebook_idx, nof_symbols);
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  spmux::PrecodeParams p = {{fl(d_x[0]), t.rx.layers == 2 ? fl(d_x[1]) : nullptr}, {fl(d_y[0]), fl(d_y[1])}, (uint32_t)nof_symbols, {t.tx_kind[0], t.tx_kind[1]}, t.tx_scale};
  PHY_HIP_CHECK(spmux::launch_precode(p, (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ the stages on HOST buffers

extern "C" int srsran_hip_predecoding_mimo(cf_t* y[SRSRAN_MAX_PORTS], cf_t* h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS], cf_t* x[SRSRAN_MAX_LAYERS],
                                           float* csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_layers, int codebook_idx, int nof_symbols,
                                           int tx_scheme, float scaling, float noise_estimate, int decoder)
{
  Taken       t;
  const char* why = nof_ports != 2 ? "2 ports are taken" : nof_symbols < 0 ? "a negative number of REs" : (!y || !h || !x) ? "NULL argument" : nullptr;
  why             = why ? why : mimo_rx_case(tx_scheme, nof_layers, codebook_idx, nof_symbols, scaling, nof_rxant, decoder, noise_estimate, t);
  for (uint32_t r = 0; !why && r < 2; r++) {
    why = (y[r] && h[0][r] && h[1][r] && (r >= t.rx.layers || x[r])) ? nullptr : "a NULL plane";
  }
  if (why) {
    return refuse_stage("srsran_hip_predecoding_mimo", why, tx_scheme, nof_ports, nof_layers, codebook_idx, nof_symbols);
  }
  if (nof_symbols == 0) {
    return SRSRAN_SUCCESS;
  }
  // y[rx], then h[port][rx], then the layers and the channel-state rows
  const size_t nb = (size_t)nof_symbols * sizeof(cf_t), nc = (size_t)nof_symbols * sizeof(float);
  PlaneGroup   grp[5] = {{y, 2, nb, true, false}, {h[0], 2, nb, true, false}, {h[1], 2, nb, true, false}, {x, t.rx.layers, nb, false, true}, {nullptr, 2, nc, false, false}};
  float*       cp[2]  = {nullptr, nullptr};
  const bool   ok = run_on_planes("srsran_hip_predecoding_mimo", grp, 5, [&](hipStream_t st) {
    const cf_t* hp[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{grp[1].pin[0], grp[1].pin[1]}, {grp[2].pin[0], grp[2].pin[1]}};
    float*      cpin[2] = {reinterpret_cast<float*>(grp[4].pin[0]), reinterpret_cast<float*>(grp[4].pin[1])};
    const spmux::EqParams ep = eq_params(grp[0].pin, hp, grp[3].pin, (csi && csi[0]) ? cpin : nullptr, (uint32_t)nof_symbols, t.rx);
    cp[0] = ep.csi[0]; // the rows the kernel writes: only those go back to the caller (the reference leaves the others untouched)
    cp[1] = ep.csi[1];
    return spmux::launch_eq(ep, st);
  });
  for (uint32_t k = 0; ok && csi && k < 2; k++) {
    if (cp[k] && csi[k]) {
      memcpy(csi[k], cp[k], nc);
    }
  }
  return ok ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

extern "C" int srsran_hip_precoding_mimo(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* y[SRSRAN_MAX_PORTS], int nof_layers, int nof_ports, int codebook_idx, int nof_symbols,
                                         float scaling, int tx_scheme)
{
  Taken       t;
  const char* why = nof_ports != 2 ? "2 ports are taken" : nof_symbols < 0 ? "a negative number of REs" : (!x || !y) ? "NULL argument" : nullptr;
  why             = why ? why : mimo_case(tx_scheme, nof_layers, codebook_idx, nof_symbols, scaling, t);
  for (uint32_t k = 0; !why && k < 2; k++) {
    why = (y[k] && (k >= t.rx.layers || x[k])) ? nullptr : "a NULL plane";
  }
  if (why) {
    return refuse_stage("srsran_hip_precoding_mimo", why, tx_scheme, nof_ports, nof_layers, codebook_idx, nof_symbols);
  }
  if (nof_symbols == 0) {
    return SRSRAN_SUCCESS;
  }
  const size_t nb = (size_t)nof_symbols * sizeof(cf_t);
  PlaneGroup   grp[2] = {{x, t.rx.layers, nb, true, false}, {y, 2, nb, false, true}};
  const bool   ok = run_on_planes("srsran_hip_precoding_mimo", grp, 2, [&](hipStream_t st) {
    spmux::PrecodeParams p = {{fl(grp[0].pin[0]), t.rx.layers == 2 ? fl(grp[0].pin[1]) : nullptr}, {fl(grp[1].pin[0]), fl(grp[1].pin[1])}, (uint32_t)nof_symbols,
                              {t.tx_kind[0], t.tx_kind[1]}, t.tx_scale};
    return spmux::launch_precode(p, st);
  });
  return ok ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

// ------------------------------------------------------------------------------------------------ PDSCH grant, receive

// weight: the _csi forms (cfg->csi_enable): the front end files each layer's channel-state values in the rows the frame (chan_internal.h) weights both
// codewords with in one launch.  Two-layer zero-forcing spatial multiplexing: the reference's equaliser
// writes q->csi[0] only (precoding.c:1330-1331) and weights codeword 1 with whatever an earlier call left in q->csi[1]; here that row is 1.0, as row 0 is.
static int pdsch_decode_mimo(bool weight, const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                             srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                             srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS],
                             float* const csi_out[SRSRAN_MAX_CODEWORDS], bool sf_form = false, const srsran_hip_pdsch_sf_t* sf = nullptr,
                             cf_t* const sym_out[] = nullptr, cf_t* const (*ce_out)[SRSRAN_MAX_PORTS] = nullptr, EstMap* est = nullptr)
{
  // est: the _est calls -- there is no ce and g->noise_estimate is not read: the estimator's kernel makes the grids on the device in front of the de-mapping,
  // and the MMSE equaliser averages get_noise() from the pairs' estimates there
  // sf_form: the _sf calls -- symbols and ce are grids, sf describes them (weight is its csi_enable), sym_out / ce_out take the extracted planes
  static const char* who = "srsran_hip_pdsch_decode_mimo";
  TraceRange         trace_(who);
  if (res) {
    res[0] = res[1] = {0, 0.f, NAN};
  }
  if (est && est->out) {
    *est->out = {};
  }
  if (!g || !symbols || (!ce && !est) || !softbuffers || !data || !res) {
    fprintf(stderr, "[srsran_phy_hip] %s: NULL argument\n", who);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t ntb = g->nof_tb;
  if ((ntb != 1 && ntb != 2) || g->nof_layers != ntb) {
    return refuse("%s: %u codewords on %u layers is not taken (1 on 1, or 2 on 2)", who, ntb, g->nof_layers);
  }
  const uint32_t nof_re = g->tb[0].nof_re;
  Taken          t;
  const char*    why = mimo_rx_case((int)g->tx_scheme, (int)g->nof_layers, (int)g->codebook_idx, nof_re, g->scaling, (int)g->nof_rx, (int)g->decoder, est ? 0.f : g->noise_estimate, t);
  if (!why && (!symbols[0] || !symbols[1] || (!est && (!ce[0][0] || !ce[0][1] || !ce[1][0] || !ce[1][1])))) {
    why = "a NULL plane";
  }
  if (!why && ntb == 2 && (g->tb[1].nof_re != nof_re || g->tb[1].llr_is_8bit != g->tb[0].llr_is_8bit || g->tb[1].max_nof_iterations != g->tb[0].max_nof_iterations)) {
    why = "the two codewords differ in nof_re, llr_is_8bit or max_nof_iterations";
  }
  bool any = false;
  for (uint32_t k = 0; !why && k < ntb; k++) {
    any = any || softbuffers[k];
    why = (softbuffers[k] && !data[k]) ? "a codeword without room for its payload" : nullptr;
  }
  if (!why && !any) {
    why = "every codeword is skipped";
  }
  if (why) {
    return refuse("%s: %s (scheme %u, %u layers, codebook_idx %u, decoder %u, %u receive antennas, %u REs, scaling %g, noise %g)", who, why, g->tx_scheme, g->nof_layers,
                  g->codebook_idx, g->decoder, g->nof_rx, nof_re, (double)g->scaling, (double)g->noise_estimate);
  }
  for (uint32_t k = 0; k < ntb; k++) {
    if (!tb_valid(g->tb[k], who)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (sf_form && !sf_valid(est ? "srsran_hip_pdsch_decode_mimo_est" : "srsran_hip_pdsch_decode_mimo_sf", sf, 2, nof_re)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (est && !est_valid("srsran_hip_pdsch_decode_mimo_est", est, sf, 2)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  // staged: 2 symbol planes, then 2 x 2 estimate planes; codeword k is layer k
  const bool   llr8 = g->tb[0].llr_is_8bit != 0;
  const size_t nd   = (size_t)nof_re * sizeof(cf_t);
  PlaneGroup   in[3] = {{symbols, 2, nd, true, false}, {est ? nullptr : ce[0], 2, nd, true, false}, {est ? nullptr : ce[1], 2, nd, true, false}};
  SfMap        map = {sf, {}};
  for (uint32_t r = 0; r < 2; r++) {
    map.out[r] = sym_out ? sym_out[r] : nullptr;
    for (uint32_t k = 0; k < 2; k++) {
      map.out[2 + 2 * k + r] = ce_out ? ce_out[k][r] : nullptr;
    }
  }
  RxGrant      gr = {who, in, 3, sf_form ? &map : nullptr, nullptr, {}, ntb, ntb, false, weight, est};
  for (uint32_t k = 0; k < ntb; k++) {
    gr.cw[k] = {&g->tb[k], qm_of(g->tb[k].mod), softbuffers[k], data[k], &res[k], d_out ? d_out[k] : nullptr, e_out ? e_out[k] : nullptr, csi_out ? csi_out[k] : nullptr};
  }
  return pdsch_decode_grant(gr, [&](hipStream_t st, void* const* d_e, float* const* row, uint8_t* d_d) {
    modem::Params mp;
    if (!modem::params_for(mp, llr8 ? modem::LLR_I8 : modem::LLR_I16)) {
      return false;
    }
    const cf_t*        hp[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {{in[1].pin[0], in[1].pin[1]}, {in[2].pin[0], in[2].pin[1]}};
    spmux::FrontParams fp = {};
    for (uint32_t r = 0; r < 2; r++) {
      fp.y[r] = reinterpret_cast<const float4*>(in[0].pin[r]);
      for (uint32_t k = 0; k < 2; k++) {
        fp.h[k][r] = reinterpret_cast<const float4*>(hp[k][r]);
      }
    }
    for (uint32_t k = 0; k < ntb; k++) {
      fp.mod[k]  = g->tb[k].mod;
      fp.seed[k] = g->tb[k].seed;
      fp.out[k]  = d_e[k];
      fp.csi[k]  = row[k];
    }
    if (est && t.rx.mmse) { // (zero forcing: 0, as pdsch.c:819 passes)
      t.rx.dev_noise = est->noise;
    }
    fp.n       = nof_re;
    fp.s       = t.rx;
    fp.x1_bits = mp.x1_bits;
    fp.x2_cols = mp.x2_cols;
    fp.k       = mp.k;
    if (spmux::launch_front(fp, llr8, st) != hipSuccess) {
      set_error("grant front end: spatial-multiplexing front-end launch failed");
      return false;
    }
    // what the reference leaves in q->d: the symbols exist in the front end's registers only, so the per-stage kernel makes them (same arithmetic)
    if (d_d) {
      cf_t* xd[SRSRAN_MAX_LAYERS] = {reinterpret_cast<cf_t*>(d_d), reinterpret_cast<cf_t*>(d_d + al256(nd))};
      if (spmux::launch_eq(eq_params(in[0].pin, hp, xd, nullptr, nof_re, t.rx), st) != hipSuccess) {
        set_error("grant front end: the equalised symbols could not be produced");
        return false;
      }
    }
    return true;
  });
}

extern "C" int srsran_hip_pdsch_decode_mimo(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                            srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                            srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS])
{
  return pdsch_decode_mimo(false, g, symbols, ce, softbuffers, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_mimo_dbg(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], cf_t* const d_out[SRSRAN_MAX_CODEWORDS],
                                                void* const e_out[SRSRAN_MAX_CODEWORDS])
{
  return pdsch_decode_mimo(false, g, symbols, ce, softbuffers, data, res, d_out, e_out, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_mimo_csi(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS])
{
  return pdsch_decode_mimo(true, g, symbols, ce, softbuffers, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_mimo_csi_dbg(const srsran_hip_pdsch_mimo_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                    srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                    srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], cf_t* const d_out[SRSRAN_MAX_CODEWORDS],
                                                    void* const e_out[SRSRAN_MAX_CODEWORDS], float* const csi_out[SRSRAN_MAX_CODEWORDS])
{
  return pdsch_decode_mimo(true, g, symbols, ce, softbuffers, data, res, d_out, e_out, csi_out);
}

extern "C" int srsran_hip_pdsch_decode_mimo_sf(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                               cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                               uint8_t* const data[SRSRAN_MAX_CODEWORDS], srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS])
{
  return pdsch_decode_mimo(sf && sf->csi_enable, g, sf_symbols, ce, softbuffers, data, res, nullptr, nullptr, nullptr, true, sf);
}

extern "C" int srsran_hip_pdsch_decode_mimo_sf_dbg(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                   cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                                   uint8_t* const data[SRSRAN_MAX_CODEWORDS], srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS],
                                                   cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS],
                                                   float* const csi_out[SRSRAN_MAX_CODEWORDS], cf_t* const sym_out[],
                                                   cf_t* const (*ce_out)[SRSRAN_MAX_PORTS])
{
  const bool weight = sf && sf->csi_enable;
  return pdsch_decode_mimo(weight, g, sf_symbols, ce, softbuffers, data, res, d_out, e_out, weight ? csi_out : nullptr, true, sf, sym_out, ce_out);
}

// ------------------------------------------------------------------------------------------------ PDSCH grant, transmit

extern "C" int srsran_hip_pdsch_encode_mimo(const srsran_hip_pdsch_mimo_tx_t* g, srsran_softbuffer_tx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                            uint8_t* const data[SRSRAN_MAX_CODEWORDS], cf_t* const symbols[])
{
  if (!softbuffers || !data) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_encode_mimo: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return srsran_hip_pdsch_encode_mimo_multi(1, g, reinterpret_cast<srsran_softbuffer_tx_t* const(*)[SRSRAN_MAX_CODEWORDS]>(softbuffers),
                                            reinterpret_cast<uint8_t* const(*)[SRSRAN_MAX_CODEWORDS]>(data), &symbols);
}

extern "C" int srsran_hip_pdsch_encode_mimo_multi(uint32_t n, const srsran_hip_pdsch_mimo_tx_t* g, srsran_softbuffer_tx_t* const (*softbuffers)[SRSRAN_MAX_CODEWORDS],
                                                  uint8_t* const (*data)[SRSRAN_MAX_CODEWORDS], cf_t* const* const* symbols)
{
  static const char* who = "srsran_hip_pdsch_encode_mimo";
  TraceRange         trace_(who);
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !softbuffers || !data || !symbols) {
    fprintf(stderr, "[srsran_phy_hip] %s: NULL argument\n", who);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  // the codewords of all grants in one list: a grant's first codeword owns its two port planes
  std::vector<TxCodeword> cw;
  std::vector<Taken>      taken(n);
  std::vector<uint32_t>   first(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t ntb = g[i].nof_tb;
    if ((ntb != 1 && ntb != 2) || g[i].nof_layers != ntb) {
      return refuse("%s: grant %u: %u codewords on %u layers is not taken (1 on 1, or 2 on 2)", who, i, ntb, g[i].nof_layers);
    }
    const uint32_t nof_re = g[i].tb[0].nof_re;
    const char*    why    = mimo_case((int)g[i].tx_scheme, (int)g[i].nof_layers, (int)g[i].codebook_idx, nof_re, g[i].scaling, taken[i]);
    if (!why && (!symbols[i] || !symbols[i][0] || !symbols[i][1])) {
      why = "a NULL plane";
    }
    if (!why && ntb == 2 && g[i].tb[1].nof_re != nof_re) {
      why = "the two codewords differ in nof_re";
    }
    for (uint32_t k = 0; !why && k < ntb; k++) {
      why = softbuffers[i][k] ? nullptr : "a codeword without a soft buffer";
    }
    if (why) {
      return refuse("%s: grant %u: %s (scheme %u, %u layers, codebook_idx %u, %u REs, scaling %g)", who, i, why, g[i].tx_scheme, g[i].nof_layers, g[i].codebook_idx, nof_re,
                    (double)g[i].scaling);
    }
    first[i] = (uint32_t)cw.size();
    for (uint32_t k = 0; k < ntb; k++) {
      if (!tb_valid(g[i].tb[k], who)) {
        return SRSRAN_ERROR_INVALID_INPUTS;
      }
      cw.push_back({&g[i].tb[k], qm_of(g[i].tb[k].mod), k == 0 ? 2u : 0u, softbuffers[i][k], data[i][k], k == 0 ? symbols[i] : nullptr, 0});
    }
  }
  ChanStage* sp = stage_for(who);
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage& s = *sp;
  return pdsch_encode_codewords<spmux::ModJob>(s, cw.data(), (uint32_t)cw.size(), [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, JobList<spmux::ModJob>& jobs) {
    modem::Params mp;
    const float2* tab = modem::mod_tables();
    if (!modem::params_for(mp, modem::LLR_I16) || !tab) {
      return false;
    }
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t f = first[i], nof_re = g[i].tb[0].nof_re;
      const bool     two   = g[i].nof_tb == 2;
      const size_t   plane = al256((size_t)nof_re * sizeof(cf_t));
      jobs.jobs[i] = {{g[i].tb[0].mod, two ? g[i].tb[1].mod : 0u},
                      {g[i].tb[0].seed, two ? g[i].tb[1].seed : 0u},
                      {e_byte_off[f], two ? e_byte_off[f + 1] : 0u},
                      nof_re,
                      g[i].nof_layers,
                      {taken[i].tx_kind[0], taken[i].tx_kind[1]},
                      taken[i].tx_scale,
                      {(uint32_t)(cw[f].o_out / sizeof(cf_t)), (uint32_t)((cw[f].o_out + plane) / sizeof(cf_t))},
                      jobs.append(i, (nof_re + MODEM_TILE_SYMS - 1) / MODEM_TILE_SYMS)};
    }
    spmux::ModParams p = {d_e, reinterpret_cast<float2*>(s.pin.get()), tab, jobs.jobs, jobs.tile_job, jobs.n_tiles, mp.x1_bits, mp.x2_cols};
    if (spmux::launch_mod(p, st) != hipSuccess) {
      set_error("spatial-multiplexing modulator launch failed");
      return false;
    }
    return true;
  });
}

// the same from the grids alone (chest_dl_kernels.hip in front of the de-mapping)
static int pdsch_decode_mimo_est(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                 const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS],
                                 uint8_t* const data[SRSRAN_MAX_CODEWORDS], srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], srsran_hip_chest_dl_res_t* est_out,
                                 cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS], float* const csi_out[SRSRAN_MAX_CODEWORDS],
                                 cf_t* const sym_out[], cf_t* const (*ce_out)[SRSRAN_MAX_PORTS], cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS])
{
  if (res) {
    res[0] = res[1] = {0, 0.f, NAN};
  }
  if (est_out) {
    *est_out = {};
  }
  if (!sf || !est || !state_in || !est_out) {
    return refuse("srsran_hip_pdsch_decode_mimo_est: NULL argument");
  }
  EstMap em = {est, state_in, est_out, {}, {}};
  for (uint32_t k = 0; ce_grid_out && k < SRSRAN_MAX_PORTS; k++) {
    for (uint32_t r = 0; r < SRSRAN_MAX_PORTS; r++) {
      em.grid_out[k][r] = ce_grid_out[k][r];
    }
  }
  return pdsch_decode_mimo(sf->csi_enable != 0, g, sf_symbols, nullptr, softbuffers, data, res, d_out, e_out, csi_out, true, sf, sym_out, ce_out, &em);
}

extern "C" int srsran_hip_pdsch_decode_mimo_est(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                                srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], srsran_hip_chest_dl_res_t* est_out)
{
  return pdsch_decode_mimo_est(g, sf, est, state_in, sf_symbols, softbuffers, data, res, est_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_mimo_est_dbg(const srsran_hip_pdsch_mimo_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                    const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[],
                                                    srsran_softbuffer_rx_t* const softbuffers[SRSRAN_MAX_CODEWORDS], uint8_t* const data[SRSRAN_MAX_CODEWORDS],
                                                    srsran_hip_grant_res_t res[SRSRAN_MAX_CODEWORDS], srsran_hip_chest_dl_res_t* est_out,
                                                    cf_t* const d_out[SRSRAN_MAX_CODEWORDS], void* const e_out[SRSRAN_MAX_CODEWORDS],
                                                    float* const csi_out[SRSRAN_MAX_CODEWORDS], cf_t* const sym_out[], cf_t* const (*ce_out)[SRSRAN_MAX_PORTS],
                                                    cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS])
{
  return pdsch_decode_mimo_est(g, sf, est, state_in, sf_symbols, softbuffers, data, res, est_out, d_out, e_out, csi_out, sym_out, ce_out, ce_grid_out);
}
