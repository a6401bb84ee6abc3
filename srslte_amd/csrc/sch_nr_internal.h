// sch_nr_internal.h -- what sch_nr_host.cpp shares with the codeword-level entry points (nr_chan_host.cpp): the transport-block parameters of
// srsran_sch_nr_fill_tb_info, the per-thread transport-block staging context, and the decode loop on soft bits that are already on the device.
#pragma once
#include "hip_common.h"
#include "stage.h"
#include "srsran_amd/phy_nr_sch_abi.h"
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

} // namespace nrtb
} // namespace phyhip
