// txdiv_host.cpp -- transmit diversity on 2 and 4 ports (include/srsran_amd/phy_chan_abi.h, txdiv_kernels.hip): the reference-named stages on HOST buffers
// (one kernel each on the calling thread's stage, like srsran_hip_modulate_bytes), their device-pointer twins, and the PDSCH codeword of a multi-port
// cell in one call each way.
#include "chan_internal.h"
#include "txdiv_device.h"

#include <cmath>
#include <vector>

using namespace phyhip;
using namespace phyhip::chan;

namespace {

bool txdiv_shape(const char* who, int nof_ports, int nof_rx, int nof_symbols)
{
  if (nof_ports != 2 && nof_ports != 4) {
    fprintf(stderr, "Number of ports must be 2 or 4 for transmit diversity (nof_ports=%d)\n", nof_ports); // precoding.c:775
    return false;
  }
  if (nof_rx != 1 && nof_rx != 2) {
    fprintf(stderr, "[srsran_phy_hip] %s: 1 or 2 receive antennas are taken (nof_rxant=%d)\n", who, nof_rx);
    return false;
  }
  if (nof_symbols % nof_ports) {
    fprintf(stderr, "[srsran_phy_hip] %s: %d symbols are not whole groups of %d\n", who, nof_symbols, nof_ports);
    return false;
  }
  return true;
}

// the transmit factor as the reference computes it (precoding.c:1958, :1962): double arithmetic on the float argument, converted to float once
inline float txdiv_tx_scale(uint32_t nof_ports, float scaling)
{
  return nof_ports == 2 ? (float)(scaling * M_SQRT1_2) : (float)(scaling / M_SQRT2);
}

inline bool aligned(const void* p, uintptr_t bytes)
{
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// ---- the kernels' parameter blocks from plane pointers (device memory, or planes of the pinned image)

txdiv::EqParams eq_params(const cf_t* const* y, const cf_t* const (*h)[SRSRAN_MAX_PORTS], cf_t* const* x, float* csi, uint32_t x_stride, uint32_t nof_rx, uint32_t ports, uint32_t n, float scaling)
{
  txdiv::EqParams p = {};
  for (uint32_t r = 0; r < nof_rx; r++) {
    p.y[r] = reinterpret_cast<const float4*>(y[r]);
    for (uint32_t k = 0; k < ports; k++) {
      p.h[k][r] = reinterpret_cast<const float4*>(h[k][r]);
    }
  }
  for (uint32_t k = 0; k < ports; k++) {
    p.x[k] = reinterpret_cast<float2*>(x[k]);
  }
  p.csi      = csi;
  p.x_stride = x_stride;
  p.ports    = ports;
  p.nof_rx   = nof_rx;
  p.n        = n;
  p.scaling  = scaling;
  return p;
}

txdiv::PrecodeParams precode_params(const cf_t* const* x, cf_t* const* y, uint32_t ports, uint32_t n, float scaling)
{
  txdiv::PrecodeParams p = {};
  for (uint32_t k = 0; k < ports; k++) {
    p.x[k] = reinterpret_cast<const float2*>(x[k]);
    p.y[k] = reinterpret_cast<float2*>(y[k]);
  }
  p.ports = ports;
  p.n     = n;
  p.scale = txdiv_tx_scale(ports, scaling);
  return p;
}

txdiv::LayerParams layer_params(const cf_t* d, const cf_t* const* x, uint32_t layers, uint32_t n, bool to_layers)
{
  txdiv::LayerParams p = {};
  for (uint32_t k = 0; k < layers; k++) {
    p.x[k] = reinterpret_cast<float2*>(const_cast<cf_t*>(x[k]));
  }
  p.d         = reinterpret_cast<float2*>(const_cast<cf_t*>(d));
  p.layers    = layers;
  p.n         = n;
  p.to_layers = to_layers ? 1u : 0u;
  return p;
}

} // namespace

extern "C" int srsran_hip_predecoding_diversity_multi(const cf_t* const d_y[SRSRAN_MAX_PORTS], const cf_t* const d_h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS],
                                                      cf_t* const d_x[SRSRAN_MAX_LAYERS], float* d_csi, uint32_t nof_rxant, uint32_t nof_ports,
                                                      uint32_t nof_symbols, float scaling, void* stream)
{
  if (!d_y || !d_h || !d_x || nof_symbols > 0x7fffffffu || !txdiv_shape("srsran_hip_predecoding_diversity_multi", (int)nof_ports, (int)nof_rxant, (int)nof_symbols) ||
      !aligned(d_csi, 8)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (uint32_t k = 0; nof_symbols && k < nof_ports; k++) {
    bool ok = d_x[k] && aligned(d_x[k], 16);
    for (uint32_t r = 0; ok && r < nof_rxant; r++) {
      ok = d_y[r] && aligned(d_y[r], 16) && d_h[k][r] && aligned(d_h[k][r], 16);
    }
    if (!ok) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  PHY_HIP_CHECK(txdiv::launch_eq(eq_params(d_y, d_h, d_x, d_csi, 1, nof_rxant, nof_ports, nof_symbols, scaling), (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_precoding_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* const d_y[SRSRAN_MAX_PORTS], uint32_t nof_ports,
                                              uint32_t nof_symbols, float scaling, void* stream)
{
  if (!d_x || !d_y || nof_symbols > 0x7fffffffu / 4 || !txdiv_shape("srsran_hip_precoding_diversity", (int)nof_ports, 1, 0)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (uint32_t k = 0; nof_symbols && k < nof_ports; k++) {
    if (!d_x[k] || !d_y[k] || !aligned(d_y[k], 16) || !aligned(d_x[k], 8)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  PHY_HIP_CHECK(txdiv::launch_precode(precode_params(d_x, d_y, nof_ports, nof_symbols, scaling), (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

static int hip_layers(const cf_t* const* d_x, const cf_t* d_d, uint32_t nof_layers, uint32_t n, bool to_layers, void* stream)
{
  if (!d_x || nof_layers == 0 || nof_layers > SRSRAN_MAX_LAYERS || (uint64_t)n * nof_layers > 0x7fffffffu) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (uint32_t k = 0; n && k < nof_layers; k++) {
    if (!d_x[k] || !aligned(d_x[k], 8)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (n && (!d_d || !aligned(d_d, 8))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!device_available()) {
    return SRSRAN_ERROR;
  }
  PHY_HIP_CHECK(txdiv::launch_layers(layer_params(d_d, d_x, nof_layers, n, to_layers), (hipStream_t)stream), SRSRAN_ERROR);
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_layermap_diversity(const cf_t* d_d, cf_t* const d_x[SRSRAN_MAX_LAYERS], uint32_t nof_layers, uint32_t nof_symbols, void* stream)
{
  return hip_layers(d_x, d_d, nof_layers, nof_layers ? nof_symbols / nof_layers : 0u, true, stream);
}

extern "C" int srsran_hip_layerdemap_diversity(const cf_t* const d_x[SRSRAN_MAX_LAYERS], cf_t* d_d, uint32_t nof_layers, uint32_t nof_layer_symbols,
                                               void* stream)
{
  return hip_layers(d_x, d_d, nof_layers, nof_layer_symbols, false, stream);
}

// the HOST-buffer forms: planes into the thread's pinned image (the kernels work on it directly), one kernel, one wait, planes out
extern "C" int srsran_predecoding_diversity_multi(cf_t* y[SRSRAN_MAX_PORTS], cf_t* h[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS], cf_t* x[SRSRAN_MAX_LAYERS],
                                                  float* csi[SRSRAN_MAX_CODEWORDS], int nof_rxant, int nof_ports, int nof_symbols, float scaling)
{
  if (!y || !h || !x || nof_symbols < 0 || !txdiv_shape("srsran_predecoding_diversity_multi", nof_ports, nof_rxant, nof_symbols)) {
    return -1;
  }
  if (nof_symbols == 0) {
    return 0;
  }
  // y[rx], then h[port][rx], then the layers and the channel-state values
  float*       c  = (csi && csi[0]) ? csi[0] : nullptr;
  const size_t nb = (size_t)nof_symbols * sizeof(cf_t);
  PlaneGroup   grp[SRSRAN_MAX_PORTS + 3] = {{y, (uint32_t)nof_rxant, nb, true, false}};
  for (int k = 0; k < nof_ports; k++) {
    grp[1 + k] = {h[k], (uint32_t)nof_rxant, nb, true, false};
  }
  PlaneGroup &gx = grp[1 + nof_ports], &gc = grp[2 + nof_ports];
  gx = {x, (uint32_t)nof_ports, nb / nof_ports, false, true};
  gc = {nullptr, 1, (size_t)nof_symbols * sizeof(float), false, false};
  const bool ok = run_on_planes("srsran_predecoding_diversity_multi", grp, nof_ports + 3, [&](hipStream_t st) {
    const cf_t* hp[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {};
    for (int k = 0; k < nof_ports; k++) {
      for (int r = 0; r < nof_rxant; r++) {
        hp[k][r] = grp[1 + k].pin[r];
      }
    }
    return txdiv::launch_eq(eq_params(grp[0].pin, hp, gx.pin, c ? reinterpret_cast<float*>(gc.pin[0]) : nullptr, 1, nof_rxant, nof_ports, nof_symbols, scaling), st);
  });
  if (ok && c) {
    memcpy(c, gc.pin[0], gc.bytes);
  }
  return ok ? nof_symbols / nof_ports : -1;
}

extern "C" int srsran_precoding_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* y[SRSRAN_MAX_PORTS], int nof_ports, int nof_symbols, float scaling)
{
  if (!x || !y || nof_symbols < 0 || nof_symbols > 0x7fffffff / 4 || !txdiv_shape("srsran_precoding_diversity", nof_ports, 1, 0)) {
    return -1;
  }
  if (nof_symbols == 0) {
    return 0;
  }
  const size_t nb = (size_t)nof_symbols * sizeof(cf_t);
  PlaneGroup   grp[2] = {{x, (uint32_t)nof_ports, nb, true, false}, {y, (uint32_t)nof_ports, nb * nof_ports, false, true}};
  const bool   ok = run_on_planes("srsran_precoding_diversity", grp, 2, [&](hipStream_t st) {
    return txdiv::launch_precode(precode_params(grp[0].pin, grp[1].pin, nof_ports, nof_symbols, scaling), st);
  });
  return ok ? nof_ports * nof_symbols : -1;
}

static int host_layers(cf_t* d, cf_t* x[SRSRAN_MAX_LAYERS], int nof_layers, int n, bool to_layers, const char* who)
{
  if (!d || !x || nof_layers < 1 || nof_layers > SRSRAN_MAX_LAYERS || n < 0 || (int64_t)n * nof_layers > 0x7fffffff) {
    return -1;
  }
  if (n == 0) {
    return 0;
  }
  const size_t nb = (size_t)n * sizeof(cf_t);
  PlaneGroup   grp[2] = {{&d, 1, nb * nof_layers, to_layers, !to_layers}, {x, (uint32_t)nof_layers, nb, !to_layers, to_layers}};
  const bool   ok = run_on_planes(who, grp, 2, [&](hipStream_t st) {
    return txdiv::launch_layers(layer_params(grp[0].pin[0], grp[1].pin, nof_layers, n, to_layers), st);
  });
  return !ok ? -1 : to_layers ? n : n * nof_layers;
}

extern "C" int srsran_layermap_diversity(cf_t* d, cf_t* x[SRSRAN_MAX_LAYERS], int nof_layers, int nof_symbols)
{
  return host_layers(d, x, nof_layers, (nof_layers > 0 && nof_symbols >= 0) ? nof_symbols / nof_layers : -1, true, "srsran_layermap_diversity");
}

extern "C" int srsran_layerdemap_diversity(cf_t* x[SRSRAN_MAX_LAYERS], cf_t* d, int nof_layers, int nof_layer_symbols)
{
  return host_layers(d, x, nof_layers, nof_layer_symbols, false, "srsran_layerdemap_diversity");
}

// ---- PDSCH codeword with transmit diversity, receive

// weight: the _csi forms (cfg->csi_enable): the front end files the combiner's channel-state values in the row the frame (chan_internal.h) weights with
// sf_form: the _sf calls -- symbols and ce are grids, sf describes them (weight is its csi_enable), sym_out / ce_out take the extracted planes
static int pdsch_decode_txdiv(bool weight, const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                              srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out, float* csi_out,
                              bool sf_form = false, const srsran_hip_pdsch_sf_t* sf = nullptr, cf_t* const sym_out[] = nullptr,
                              cf_t* const (*ce_out)[SRSRAN_MAX_PORTS] = nullptr, EstMap* est = nullptr)
{
  // est: the _est calls -- there is no ce: the estimator's kernel makes the grids on the device in front of the de-mapping
  TraceRange trace_("srsran_hip_pdsch_decode_txdiv");
  if (res) {
    *res = {0, 0.f, NAN};
  }
  if (est && est->out) {
    *est->out = {};
  }
  if (!g || !symbols || (!ce && !est) || !softbuffer || !data || !res) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_decode_txdiv: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!tb_valid(g->tb, "srsran_hip_pdsch_decode_txdiv")) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t ports = g->nof_ports, nrx = g->nof_rx, nof_re = g->tb.nof_re;
  bool           planes = (ports == 2 || ports == 4) && (nrx == 1 || nrx == 2);
  for (uint32_t r = 0; planes && r < nrx; r++) {
    planes = symbols[r] != nullptr;
    for (uint32_t k = 0; planes && !est && k < ports; k++) {
      planes = ce[k][r] != nullptr;
    }
  }
  if (!planes || nof_re % ports || !(g->scaling != 0.f) || !std::isfinite(g->scaling)) {
    return refuse("srsran_hip_pdsch_decode_txdiv: %u ports, %u receive antennas, %u REs, scaling %g%s is not a transmit-diversity grant", ports, nrx, nof_re, (double)g->scaling,
                  (ports == 2 || ports == 4) && (nrx == 1 || nrx == 2) && !planes ? ", a NULL plane" : "");
  }
  if (sf_form && !sf_valid(est ? "srsran_hip_pdsch_decode_txdiv_est" : "srsran_hip_pdsch_decode_txdiv_sf", sf, ports, nof_re)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (est && !est_valid("srsran_hip_pdsch_decode_txdiv_est", est, sf, nrx)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  // staged: nof_rx symbol planes, then nof_ports x nof_rx estimate planes
  const srsran_hip_grant_tb_t& tb = g->tb;
  const size_t                 nd = (size_t)nof_re * sizeof(cf_t);
  PlaneGroup                   in[1 + SRSRAN_MAX_PORTS] = {{symbols, nrx, nd, true, false}};
  SfMap                        map = {sf, {}};
  for (uint32_t r = 0; r < nrx; r++) {
    map.out[r] = sym_out ? sym_out[r] : nullptr;
  }
  for (uint32_t k = 0; k < ports; k++) {
    in[1 + k] = {est ? nullptr : ce[k], nrx, nd, true, false};
    for (uint32_t r = 0; r < nrx; r++) {
      map.out[nrx + k * nrx + r] = ce_out ? ce_out[k][r] : nullptr;
    }
  }
  RxGrant gr = {"srsran_hip_pdsch_decode_txdiv", in, 1 + ports, sf_form ? &map : nullptr, nullptr, {{&tb, 2 * qm_of(tb.mod), softbuffer, data, res, d_out, e_out, csi_out}}, 1, 1, false, weight, est};
  return pdsch_decode_grant(gr, [&](hipStream_t st, void* const* d_e, float* const* row, uint8_t* d_d) {
    const cf_t* hp[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS] = {};
    cf_t*       xd[SRSRAN_MAX_LAYERS]                  = {};
    for (uint32_t k = 0; k < ports; k++) {
      for (uint32_t r = 0; r < nrx; r++) {
        hp[k][r] = in[1 + k].pin[r];
      }
      xd[k] = d_d ? reinterpret_cast<cf_t*>(d_d) + k : nullptr; // the combined symbols layer-demapped: layer k's symbol i is d[ports i + k]
    }
    const txdiv::EqParams ep = eq_params(in[0].pin, hp, xd, nullptr, ports, nrx, ports, nof_re, g->scaling);
    modem::Params         mp;
    if (!modem::params_for(mp, tb.llr_is_8bit ? modem::LLR_I8 : modem::LLR_I16)) {
      return false;
    }
    txdiv::FrontParams fp = {};
    memcpy(fp.y, ep.y, sizeof(fp.y));
    memcpy(fp.h, ep.h, sizeof(fp.h));
    fp.out     = d_e[0];
    fp.csi     = row[0];
    fp.mod     = tb.mod;
    fp.n       = nof_re;
    fp.seed    = tb.seed;
    fp.ports   = ports;
    fp.nof_rx  = nrx;
    fp.scaling = g->scaling;
    fp.x1_bits = mp.x1_bits;
    fp.x2_cols = mp.x2_cols;
    fp.k       = mp.k;
    if (txdiv::launch_front(fp, tb.llr_is_8bit != 0, st) != hipSuccess) {
      set_error("grant front end: transmit-diversity front-end launch failed");
      return false;
    }
    // what the reference leaves in q->d: the symbols exist in the front end's registers only, so the per-stage kernel makes them (same arithmetic)
    if (d_d && txdiv::launch_eq(ep, st) != hipSuccess) {
      set_error("grant front end: the combined symbols could not be produced");
      return false;
    }
    return true;
  });
}

extern "C" int srsran_hip_pdsch_decode_txdiv(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                             srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res)
{
  return pdsch_decode_txdiv(false, g, symbols, ce, softbuffer, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                 srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out)
{
  return pdsch_decode_txdiv(false, g, symbols, ce, softbuffer, data, res, d_out, e_out, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_csi(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                 srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res)
{
  return pdsch_decode_txdiv(true, g, symbols, ce, softbuffer, data, res, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_csi_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, cf_t* const symbols[], cf_t* const (*ce)[SRSRAN_MAX_PORTS],
                                                     srsran_softbuffer_rx_t* softbuffer, uint8_t* data, srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out,
                                                     float* csi_out)
{
  return pdsch_decode_txdiv(true, g, symbols, ce, softbuffer, data, res, d_out, e_out, csi_out);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_sf(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                                srsran_hip_grant_res_t* res)
{
  return pdsch_decode_txdiv(sf && sf->csi_enable, g, sf_symbols, ce, softbuffer, data, res, nullptr, nullptr, nullptr, true, sf);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_sf_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, cf_t* const sf_symbols[],
                                                    cf_t* const (*ce)[SRSRAN_MAX_PORTS], srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                                    srsran_hip_grant_res_t* res, cf_t* d_out, void* e_out, float* csi_out, cf_t* const sym_out[],
                                                    cf_t* const (*ce_out)[SRSRAN_MAX_PORTS])
{
  const bool weight = sf && sf->csi_enable;
  return pdsch_decode_txdiv(weight, g, sf_symbols, ce, softbuffer, data, res, d_out, e_out, weight ? csi_out : nullptr, true, sf, sym_out, ce_out);
}

// ---- PDSCH codeword with transmit diversity, transmit

extern "C" int srsran_hip_pdsch_encode_txdiv(const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* softbuffer, uint8_t* data, cf_t* const symbols[])
{
  return srsran_hip_pdsch_encode_txdiv_multi(1, g, &softbuffer, &data, &symbols);
}

extern "C" int srsran_hip_pdsch_encode_txdiv_multi(uint32_t n, const srsran_hip_pdsch_txdiv_tx_t* g, srsran_softbuffer_tx_t* const* softbuffers,
                                                   uint8_t* const* data, cf_t* const* const* symbols)
{
  TraceRange trace_("srsran_hip_pdsch_encode_txdiv");
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!g || !softbuffers || !data || !symbols) {
    fprintf(stderr, "[srsran_phy_hip] srsran_hip_pdsch_encode_txdiv: NULL argument\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  std::vector<TxCodeword> cw(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t ports = g[i].nof_ports;
    bool           ok    = softbuffers[i] && symbols[i] && (ports == 2 || ports == 4);
    for (uint32_t k = 0; ok && k < ports; k++) {
      ok = symbols[i][k] != nullptr;
    }
    if (!ok || !(g[i].scaling != 0.f) || !std::isfinite(g[i].scaling)) {
      return refuse("srsran_hip_pdsch_encode_txdiv: codeword %u: %u ports, scaling %g or a NULL argument", i, ports, (double)g[i].scaling);
    }
    if (!tb_valid(g[i].tb, "srsran_hip_pdsch_encode_txdiv")) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (g[i].tb.nof_re % ports) {
      return refuse("srsran_hip_pdsch_encode_txdiv: codeword %u: %u REs are not whole groups of %u", i, g[i].tb.nof_re, ports);
    }
    cw[i] = {&g[i].tb, 2 * qm_of(g[i].tb.mod), ports, softbuffers[i], data[i], symbols[i], 0};
  }
  ChanStage* sp = stage_for("srsran_hip_pdsch_encode_txdiv");
  if (!sp) {
    return SRSRAN_ERROR;
  }
  ChanStage& s = *sp;
  return pdsch_encode_codewords<txdiv::ModJob>(s, cw.data(), n, [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, JobList<txdiv::ModJob>& jobs) {
    modem::Params mp;
    const float2* tab = modem::mod_tables();
    if (!modem::params_for(mp, modem::LLR_I16) || !tab) {
      return false;
    }
    for (uint32_t i = 0; i < n; i++) {
      const size_t plane = al256((size_t)g[i].tb.nof_re * sizeof(cf_t));
      jobs.jobs[i] = {g[i].tb.mod, g[i].tb.nof_re, g[i].tb.seed, g[i].nof_ports, txdiv_tx_scale(g[i].nof_ports, g[i].scaling), e_byte_off[i], {0, 0, 0, 0},
                      jobs.append(i, modem::tiles_of(g[i].tb.mod, g[i].tb.nof_re))};
      for (uint32_t k = 0; k < g[i].nof_ports; k++) {
        jobs.jobs[i].out_off[k] = (uint32_t)((cw[i].o_out + k * plane) / sizeof(cf_t));
      }
    }
    txdiv::ModParams p = {d_e, reinterpret_cast<float2*>(s.pin.get()), tab, jobs.jobs, jobs.tile_job, jobs.n_tiles, mp.x1_bits, mp.x2_cols};
    if (txdiv::launch_mod(p, st) != hipSuccess) {
      set_error("transmit-diversity modulator launch failed");
      return false;
    }
    return true;
  });
}

// the same from the grids alone: the estimator's kernel (chest_dl_kernels.hip) in front of the de-mapping; diversity combining takes no noise estimate
static int pdsch_decode_txdiv_est(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                  const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* softbuffer, uint8_t* data,
                                  srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out, cf_t* d_out, void* e_out, float* csi_out, cf_t* const sym_out[],
                                  cf_t* const (*ce_out)[SRSRAN_MAX_PORTS], cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS])
{
  if (res) {
    *res = {0, 0.f, NAN};
  }
  if (est_out) {
    *est_out = {};
  }
  if (!sf || !est || !state_in || !est_out) {
    return refuse("srsran_hip_pdsch_decode_txdiv_est: NULL argument");
  }
  EstMap em = {est, state_in, est_out, {}, {}};
  for (uint32_t k = 0; ce_grid_out && k < SRSRAN_MAX_PORTS; k++) {
    for (uint32_t r = 0; r < SRSRAN_MAX_PORTS; r++) {
      em.grid_out[k][r] = ce_grid_out[k][r];
    }
  }
  return pdsch_decode_txdiv(sf->csi_enable != 0, g, sf_symbols, nullptr, softbuffer, data, res, d_out, e_out, csi_out, true, sf, sym_out, ce_out, &em);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_est(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                 const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* softbuffer,
                                                 uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out)
{
  return pdsch_decode_txdiv_est(g, sf, est, state_in, sf_symbols, softbuffer, data, res, est_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int srsran_hip_pdsch_decode_txdiv_est_dbg(const srsran_hip_pdsch_txdiv_rx_t* g, const srsran_hip_pdsch_sf_t* sf, const srsran_hip_chest_dl_t* est,
                                                     const srsran_hip_chest_dl_state_t* state_in, cf_t* const sf_symbols[], srsran_softbuffer_rx_t* softbuffer,
                                                     uint8_t* data, srsran_hip_grant_res_t* res, srsran_hip_chest_dl_res_t* est_out, cf_t* d_out, void* e_out,
                                                     float* csi_out, cf_t* const sym_out[], cf_t* const (*ce_out)[SRSRAN_MAX_PORTS],
                                                     cf_t* const (*ce_grid_out)[SRSRAN_MAX_PORTS])
{
  return pdsch_decode_txdiv_est(g, sf, est, state_in, sf_symbols, softbuffer, data, res, est_out, d_out, e_out, csi_out, sym_out, ce_out, ce_grid_out);
}
