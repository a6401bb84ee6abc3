// chan_internal.h -- what the grant-level entry points share (chan_host.cpp: one port; txdiv_host.cpp: transmit diversity; spmux_host.cpp: spatial
// multiplexing and CDD): the calling thread's staging context, the grant checks, the two grant frames that exist once -- PDSCH receive of a grant's one or two
// codewords (pdsch_decode_grant: staging, transport-block stage, CSI weighting, the _dbg outputs and their bookkeeping; a scheme adds its kernels), PDSCH
// transmit of a TTI's codewords -- and the frame of a per-stage call on host planes.
#pragma once
#include "call_frame.h"
#include "hip_common.h"
#include "joblist.h"
#include "pdsch_map.h"
#include "sch_stage.h"
#include "srsran_amd/phy_chan_abi.h"

#include <map>
#include <vector>

namespace phyhip {
namespace chan {

inline uint32_t qm_of(uint32_t mod)
{
  return mod == 0 ? 1u : 2u * mod;
}
inline uint32_t qm_rm(const srsran_hip_grant_tb_t& tb) // what decode_tb / encode_tb get as Qm (sch.c:590,632)
{
  return qm_of(tb.mod) * (tb.nl ? tb.nl : 1u);
}

// per calling thread: pinned images the kernels read the grant's symbols / channel estimates from and write transmit symbols into, device
// scratch between the front-end kernels, the transform plans of the allocation sizes seen so far
struct ChanStage {
  HostImage pin;
  DeviceBuf dev;
  std::map<uint32_t, srsran_hip_dft_batch_t*> idft; // L_prb -> backward, normalised plan of 12 L_prb points (srsran_dft_precoding_init_rx)
  std::map<uint32_t, srsran_hip_dft_batch_t*> fdft; // L_prb -> forward, normalised plan (srsran_dft_precoding_init_tx): PUSCH transmit
  ~ChanStage()
  {
    for (auto& kv : idft) {
      srsran_hip_dft_batch_free(kv.second);
    }
    for (auto& kv : fdft) {
      srsran_hip_dft_batch_free(kv.second);
    }
  }
  bool grow(size_t need_pin, size_t need_dev) { return pin.grow(need_pin, need_pin / 2) && dev.grow(need_dev, need_dev / 2); }
  srsran_hip_dft_batch_t* plan(uint32_t L_prb, bool tx = false)
  {
    auto& plans = tx ? fdft : idft;
    auto  it    = plans.find(L_prb);
    if (it != plans.end()) {
      return it->second;
    }
    srsran_hip_dft_batch_t* h = nullptr;
    if (srsran_hip_dft_batch_create(&h, (int)(12 * L_prb), tx ? SRSRAN_DFT_FORWARD : SRSRAN_DFT_BACKWARD, false, false, true) != SRSRAN_SUCCESS) {
      return nullptr;
    }
    plans[L_prb] = h;
    return h;
  }
};

// the calling thread's stage; nullptr (one line on stderr) without a device
ChanStage* stage_for(const char* who);

bool segment(srsran_cbsegm_t* seg, uint32_t tbs);
bool tb_valid(const srsran_hip_grant_tb_t& tb, const char* who);

// a refused grant: the text is what srsran_hip_last_error() returns and one line on stderr
template <class... Args>
int refuse(const char* fmt, Args... args)
{
  set_error(fmt, args...);
  fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
  return SRSRAN_ERROR_INVALID_INPUTS;
}

// ---- CSI weighting of the soft bits (cfg->csi_enable: csi_correction, pdsch.c:523-618; csi_kernels.hip), what the three _csi grant calls share.
// The front end leaves the codeword's CSI row -- one float per RE -- in device scratch (or the caller's row went up in the pinned image); ONE launch
// behind it weights the soft bits of the call's codewords in place at d_e, in front of the transport-block stage and of the _dbg downloads.
struct CsiCodeword {
  void*        d_e;
  const float* csi; // device-readable
  uint32_t     mod;
};
bool enqueue_csi_weight(hipStream_t st, const CsiCodeword* cw, uint32_t n_cw, uint32_t nof_re, bool llr8);
inline size_t csi_plane(uint32_t nof_re) // a CSI row's room in a staging image
{
  return al256((size_t)nof_re * sizeof(float));
}
// a caller's row: every entry finite and >= 0 (checked before the device is looked for)
bool csi_row_valid(const float* csi, uint32_t nof_re);

// The codewords of a TTI, transmit, behind the caller's checks: one coding launch over the code blocks of all of them, one launch of the caller's
// modulator, one host wait.  The pinned image holds, per codeword, `planes` output planes of al256(nof_re points) from o_out, then the job list;
// `launch(stream, d_e, e_byte_off, JobList<J>&)` writes the jobs (e_byte_off[i]: codeword i's first byte in d_e) and enqueues the kernel.
struct TxCodeword {
  const srsran_hip_grant_tb_t* tb;
  uint32_t                     Qm; // the rate matcher's
  uint32_t                     planes;
  srsran_softbuffer_tx_t*      sb;
  uint8_t*                     data;
  cf_t* const*                 symbols; // [planes]: where the planes go
  size_t                       o_out;   // out: the first plane's byte offset in the pinned image
};
template <class J, class Launch>
int pdsch_encode_codewords(ChanStage& s, TxCodeword* cw, uint32_t n, Launch launch)
{
  std::vector<srsran_cbsegm_t> seg(n);
  std::vector<sch::TxItem>     items(n);
  size_t                       out_bytes = 0, tiles = 0;
  for (uint32_t i = 0; i < n; i++) {
    const srsran_hip_grant_tb_t& tb = *cw[i].tb;
    if (!segment(&seg[i], tb.tbs)) { // (behind every codeword's checks: it cannot fail for a grant tb_valid has passed)
      return SRSRAN_ERROR;
    }
    items[i]    = {cw[i].sb, &seg[i], cw[i].Qm, tb.rv, tb.nof_re * qm_of(tb.mod), cw[i].data, 0};
    cw[i].o_out = out_bytes;
    out_bytes += cw[i].planes * al256((size_t)tb.nof_re * sizeof(cf_t));
    tiles += modem::tiles_of(tb.mod, tb.nof_re);
  }
  const JobListLayout jl = job_list_layout(out_bytes, n * sizeof(J), tiles);
  if (out_bytes / sizeof(cf_t) > 0xffffffffull || !s.grow(jl.end, 0)) { // (the jobs count their planes' points from the image's start in 32 bits)
    return SRSRAN_ERROR;
  }
  const sch::GroupBackEnd back = [&](hipStream_t st, const uint8_t* d_e, const uint32_t* e_byte_off, uint32_t m) {
    JobList<J> jobs(s.pin, jl.o_jobs, jl.o_tj);
    return m == n && launch(st, d_e, e_byte_off, jobs);
  };
  const int rc = sch::encode_tbs_staged(items.data(), n, &back);
  if (rc != SRSRAN_SUCCESS) {
    return rc;
  }
  for (uint32_t i = 0; i < n; i++) {
    const size_t nb = (size_t)cw[i].tb->nof_re * sizeof(cf_t);
    for (uint32_t k = 0; k < cw[i].planes; k++) {
      memcpy(cw[i].symbols[k], s.pin + cw[i].o_out + k * al256(nb), nb);
    }
  }
  return SRSRAN_SUCCESS;
}

// ---- planes in the thread's pinned image (the kernels work on it directly)

struct PlaneGroup { // k planes of `bytes` each, 256-byte aligned, group behind group in the image
  cf_t* const* host;                  // the caller's planes (refused when one is NULL); nullptr: room in the image only
  uint32_t     k;
  size_t       bytes;
  bool         in, out;               // copied in before / out after the kernel
  cf_t*        pin[SRSRAN_MAX_PORTS]; // set by place_planes: the planes in the image
};
inline size_t plane_room(const PlaneGroup* grp, uint32_t n_grp)
{
  size_t need = 0;
  for (uint32_t g = 0; g < n_grp; g++) {
    need += grp[g].k * al256(grp[g].bytes);
  }
  return need;
}
// the groups' planes from the image's start (plane_room bytes), the `in` ones filled from the caller's
inline void place_planes(uint8_t* at, PlaneGroup* grp, uint32_t n_grp)
{
  for (uint32_t g = 0; g < n_grp; g++) {
    for (uint32_t i = 0; i < grp[g].k; i++, at += al256(grp[g].bytes)) {
      grp[g].pin[i] = reinterpret_cast<cf_t*>(at);
      if (grp[g].in) {
        memcpy(at, grp[g].host[i], grp[g].bytes);
      }
    }
  }
}

// a host-buffer stage: the caller's planes into the image, one kernel, one wait, planes out
template <class Launch>
bool run_on_planes(const char* who, PlaneGroup* grp, uint32_t n_grp, Launch launch)
{
  for (uint32_t g = 0; g < n_grp; g++) {
    for (uint32_t i = 0; grp[g].host && i < grp[g].k; i++) {
      if (!grp[g].host[i]) {
        return false;
      }
    }
  }
  ChanStage*  s  = stage_for(who);
  hipStream_t st = s ? sch::stage_stream() : nullptr;
  if (!st || !s->grow(plane_room(grp, n_grp), 0)) {
    return false;
  }
  place_planes(s->pin, grp, n_grp);
  if (call::settle(launch(st), st) != hipSuccess) {
    return false;
  }
  for (uint32_t g = 0; g < n_grp; g++) {
    for (uint32_t i = 0; grp[g].out && i < grp[g].k; i++) {
      memcpy(grp[g].host[i], grp[g].pin[i], grp[g].bytes);
    }
  }
  return true;
}

// ---- one PDSCH grant, receive, behind the caller's checks: the frame around a scheme's front-end kernels.  It stages the planes, runs the grant's one or two
// codewords as ONE pass of the transport-block stage (sch::decode_tbs_staged) whose front end is `front` and, with `weight`, one CSI weighting launch behind it
// (csi_kernels.hip), downloads what _dbg asked for, copies out and fills every codeword's res.  The codewords share nof_re, llr_is_8bit and max_nof_iterations.
// Pinned image: the planes, d_planes planes for the equalised symbols, every codeword's soft bits, every codeword's CSI row (the caller's, or what _dbg hands
// back); device scratch: the equalised symbols (when somebody wants them), the CSI rows the front end files.  Everything on a 256-byte boundary, a plane's
// padding behind it (the MIMO kernels read an odd grant's last pair whole).
// With g.est (the _est calls) the pinned image starts with the estimator's input -- the whole received grids, the pilot rows, the PSS -- and ONE more launch in
// front of the de-mapping makes the ce grids in device scratch; the pairs' records come down in the pinned image and are finished after the host wait.
// With g.map (the _sf calls) the planes' place in the pinned image holds the used rows of the grids and the segment table instead; ONE launch in front of the
// scheme's de-maps all planes into device scratch behind the CSI rows, and `front` reads them there (g.in[].pin); _sf_dbg's planes come down in one copy.
// SRSRAN_ERROR when a device-side step failed, and -- one line on stderr -- when a _dbg output that was asked for was not produced: the front end does not run for a
// codeword the transport-block stage drops (a soft buffer with fewer rows than code blocks) or whose blocks were all decoded in an earlier round.  Such an
// output is left untouched; res is filled in both cases.
struct RxCodeword {
  const srsran_hip_grant_tb_t* tb;
  uint32_t                     Qm; // the rate matcher's
  srsran_softbuffer_rx_t*      sb; // nullptr: skipped (its layer is still part of the front end)
  uint8_t*                     data;
  srsran_hip_grant_res_t*      res;
  cf_t*                        d_out; // _dbg, or nullptr: equalised symbols, soft bits, the CSI row that was used
  void*                        e_out;
  float*                       csi_out;
};

// ---- the _sf calls: the planes handed in are subframe grids, de-mapped on the device (pdsch_map.h, pdsch_map_kernels.hip)
#define PDSCH_MAX_RX_PLANES 10 // nof_rx * (1 + nof_ports) of the largest grant taken: 2 * (1 + 4)
struct SfMap {
  const srsran_hip_pdsch_sf_t* sf;
  cf_t*                        out[PDSCH_MAX_RX_PLANES]; // _sf_dbg, or nullptr: where the extracted plane goes, in the order the planes are staged
};
// one line on stderr and false for what the _sf calls refuse on top of their twins: a NULL or invalid description, a cell_nof_ports other than `ports`,
// another RE count than the grant's
bool sf_valid(const char* who, const srsran_hip_pdsch_sf_t* sf, uint32_t ports, uint32_t nof_re);
// the used rows of a grid into a plane's staged image of window w: whole rows in one copy, or the span of the allocation row by row
inline void stage_grid(uint8_t* at, const cf_t* grid, const srsran_hip_pdsch_sf_t& sf, const pdsch_map::Window& w)
{
  const size_t row = (size_t)12 * sf.cell_nof_prb, span = (size_t)12 * w.prbs;
  if (w.prbs == sf.cell_nof_prb) {
    memcpy(at, grid + w.row0 * row, w.rows * row * sizeof(cf_t));
    return;
  }
  for (uint32_t r = 0; r < w.rows; r++) {
    memcpy(at + r * span * sizeof(cf_t), grid + (w.row0 + r) * row + (size_t)12 * w.prb0, span * sizeof(cf_t));
  }
}

// ---- the _est calls: the channel estimates are made on the device from the received grids (chest_dl.h, chest_dl_kernels.hip), in the same frame
struct EstMap {
  const srsran_hip_chest_dl_t*       cfg;
  const srsran_hip_chest_dl_state_t* state;
  srsran_hip_chest_dl_res_t*         out;
  cf_t*                              grid_out[SRSRAN_MAX_PORTS][SRSRAN_MAX_PORTS]; // _est_dbg, or nullptr: where the pair's whole ce grid goes, [port][rx]
  modem::NoiseAvg                    noise; // set by the frame before `front` runs: the pairs' noise estimates in device memory (get_noise's order)
};
// one line on stderr and false for what the _est calls refuse on top of their _sf twins: a NULL description, state or est_out, what srsran_hip_chest_dl_estimate
// refuses, a cell or subframe that is not `sf`'s, another antenna count than the call's, a grant that does not span both whole slots (the estimator's grid).
// *est->out is zeroed first.
bool est_valid(const char* who, EstMap* est, const srsran_hip_pdsch_sf_t* sf, uint32_t nof_rx);

struct RxGrant {
  const char*  who;
  PlaneGroup*  in; // staged: symbols [nof_rx], then estimates [port][nof_rx]
  uint32_t     n_in;
  const SfMap* map; // nullptr: `in` are the grant's extracted REs; else they are grids (PlaneGroup::bytes is still a PLANE's) and pin[] will be device scratch
  const float* csi; // the caller's CSI row in place of the front end's (one port without estimates), or nullptr
  RxCodeword   cw[SRSRAN_MAX_CODEWORDS];
  uint32_t     n_cw;
  uint32_t     d_planes;  // planes of nof_re points the equalised symbols take: 1, one per layer with MIMO; 0: the front end makes none
  bool         d_scratch; // the front end needs that room whether or not d_out asks for it
  bool         weight;
  EstMap*      est; // nullptr, or (with map) the estimate planes have no host planes: the estimator's kernel runs ahead of the de-mapping on the whole received
                    // grids, its ce grids stay in device scratch and the de-mapping reads them there
};
// enqueues the scheme's kernels on the stage's stream, reading g.in[].pin: codeword k's soft bits to d_e[k] and, with weight, its CSI values to row[k]
// (d_e[k] == nullptr: not called for that codeword; row[k] is device-readable); the equalised symbols to d_d, plane behind plane of al256(nof_re points) --
// nullptr when nobody asked for them
using RxFront = std::function<bool(hipStream_t st, void* const* d_e, float* const* row, uint8_t* d_d)>;
int pdsch_decode_grant(RxGrant& g, const RxFront& front);

} // namespace chan
} // namespace phyhip
