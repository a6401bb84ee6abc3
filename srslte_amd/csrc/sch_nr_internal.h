// sch_nr_internal.h -- what sch_nr_host.cpp shares with the codeword-level entry points (nr_chan_host.cpp): the transport-block parameters of
// srsran_sch_nr_fill_tb_info, the per-thread transport-block staging context, and the decode loop on soft bits that are already on the device.
#pragma once
#include "call_frame.h"
#include "hip_common.h"
#include "srsran_amd/phy_nr_sch_abi.h"
#include "srsran_amd/phy_sch_abi.h"
#include <map>

namespace phyhip {
namespace nrtb {

struct TbCfg { // srsran_sch_nr_tb_info_t
  int      bg;
  uint32_t Qm, A, L_tb, L_cb, B, Bp, Kp, Kr, F, Z, G, Nl, Nref, C, N;
};
// srsran_sch_nr_fill_tb_info with cbsegm_ldpc; false where the reference fails
bool     tb_cfg(const srsran_hip_nr_tb_t& tb, TbCfg* c);
uint32_t get_E(const TbCfg& c, uint32_t j); // sch_nr_get_E, sch_nr.c:146-157 (all code blocks transmitted)

// (tail: device-to-host copies a caller wants queued behind the last kernel and in front of the call's one host wait)
struct TailCopy {
  void*       dst;
  const void* src;
  size_t      bytes;
};
// srsran_hip_sch_nr_decode with tail copies
int sch_nr_decode(srsran_hip_sch_nr_t* h, const int8_t* d_e_bits, const srsran_hip_nr_tb_t* tbs, uint32_t n_tb, int8_t* d_softbuffer, uint32_t sb_stride,
                  uint8_t* cb_crc, uint8_t* d_cb_data, uint32_t data_stride, uint8_t* d_payload, srsran_hip_nr_tb_result_t* res, void* stream,
                  const TailCopy* tail, int n_tail);

// the staging context of the host-pointer entry points: one per worker thread and device, kept in a pool (hip_common.h: StagePool) so that what
// srsran_hip_warmup() prepared on a short-lived thread is what a worker finds at its first slot
struct NrTbStage {
  StageStream                              st;
  std::map<uint64_t, srsran_hip_sch_nr_t*> sch; // (scaling factor, iterations) -> decoder object
  HostImage                                pin; // pinned image the kernels read and write themselves
  DeviceBuf                                dev;
  static const uint32_t                    MAX_CB = 160; // > SRSRAN_SCH_NR_MAX_NOF_CB_LDPC (sch_nr.h:41)
  ~NrTbStage();
  bool                 ready() { return st.open(); }
  srsran_hip_sch_nr_t* decoder(float scaling, uint32_t iters);
  bool                 grow(size_t need) { return dev.grow(need) && pin.grow(need); }
};
NrTbStage& tb_stage(); // of the calling thread, on the device it is bound to

// The reference's soft buffer of ONE codeword around a decode call on the stage's images (sch_nr.c:570-588 in, :633-652 out): rows at
// o_soft + (first_cb + r) * sb_stride, stored code blocks at o_data + (first_cb + r) * data_stride.  stage_in and fetch enqueue on the stage's stream, return
// the first error of that and wait for nothing.
struct SoftStager {
  srsran_softbuffer_rx_t* sb;
  const TbCfg*            c;
  uint32_t                first_cb, sb_stride, data_stride;
  size_t                  o_soft, o_data;
  uint8_t                 flags_in[NrTbStage::MAX_CB]; // the call's flags on entry
  bool                    fresh, any_flag;             // fresh: rows are written, not accumulated into, and not uploaded
  int                     first, last;                 // undecoded blocks: on entry (stage_in), still undecoded (fetch); -1: none
  // flags[first_cb + r] from cb_crc (none with new_data); stored blocks and, unless fresh, undecoded rows -> pinned image -> device (the rows in one copy)
  hipError_t stage_in(NrTbStage& s, srsran_softbuffer_rx_t* softbuffer, const TbCfg& cfg, uint32_t first_code_block, size_t soft_off, uint32_t soft_stride,
                      size_t data_off, uint32_t row_stride, bool new_data, uint8_t* flags);
  // behind the decode's host wait: cb_crc and data[r] of the blocks decoded now; one download of the rows still undecoded (first >= 0: wait again, then finish)
  hipError_t fetch(NrTbStage& s, const uint8_t* flags);
  void       finish(NrTbStage& s) const; // min(N, Nref) bytes of every row still undecoded, back into buffer_f[r]
};

} // namespace nrtb
} // namespace phyhip
