// conv_host.cpp -- the LTE convolutional code's receive side (include/srsran_amd/phy_conv_abi.h): the reference's srsran_viterbi_* handle API on the
// device decoder, n frames in one launch (srsran_hip_viterbi_decode_us_multi) and the PDCCH blind search's decodes in one call
// (srsran_hip_pdcch_dci_decode_multi).  The kernels are in conv_kernels.hip.  Every call is one round trip (call_frame.h) with one launch on the calling
// thread's staging context, which srsran_hip_warmup() prepares (warmup_host.cpp).  One layout serves the pinned image and the device
// buffer: [jobs | inputs || outputs]; what is in front of || goes up, what is behind comes down.
#include "call_frame.h"
#include "conv_device.h"
#include "srsran_amd/phy_conv_abi.h"

#include <cmath>

using namespace phyhip;

static_assert(sizeof(srsran_viterbi_t) == 96, "srsran_viterbi_t has the reference's layout (viterbi.h:39-55)");
static_assert(sizeof(srsran_hip_pdcch_res_t) == 152 && sizeof(srsran_hip_pdcch_cand_t) == 12, "phy_conv_abi.h layout");
static_assert(conv::kMaxFrame == SRSRAN_HIP_VITERBI_MAX_FRAMEBITS && conv::kDciBits == SRSRAN_HIP_DCI_MAX_BITS + 16, "limits");

namespace {

struct ConvStage : call::Stage {};

ConvStage& conv_stage() // of the calling thread, on the device it is bound to
{
  static thread_local StageRef<ConvStage> r;
  return r.get();
}

char handle_tag; // what an initialised handle's ptr points at: the handle owns nothing on the host or the device

struct Frame { // one frame of a handle call: host symbols (uint16 or float by `kind`), host output, length
  const void* in;
  uint8_t*    out;
  uint32_t    L;
};

// n validated frames (1 <= L <= q->framebits <= kMaxFrame) in one launch.  Returns q->framebits, or SRSRAN_ERROR on a device-side failure.
int run_frames(const char* who, const srsran_viterbi_t* q, uint32_t kind, const Frame* f, uint32_t n)
{
  TraceRange     trace_(who);
  const bool     tail = q->tail_biting;
  const size_t   es   = kind == conv::IN_F32 ? sizeof(float) : sizeof(uint16_t);
  ConvStage&     s    = conv_stage();
  if (!s.ready()) {
    return call::no_device(who);
  }
  size_t   off  = al256((size_t)n * sizeof(conv::VitJob));
  uint32_t Lmax = 0;
  std::vector<conv::VitJob> jobs(n);
  for (uint32_t i = 0; i < n; i++) {
    jobs[i] = conv::VitJob{(uint32_t)off, f[i].L, 0, kind, q->gain_quant};
    off     = al256(off + (size_t)3 * (f[i].L + (tail ? 0 : 6)) * es);
    Lmax    = f[i].L > Lmax ? f[i].L : Lmax;
  }
  const size_t up = off;
  for (uint32_t i = 0; i < n; i++) {
    jobs[i].o_out = (uint32_t)off;
    off           = al256(off + f[i].L);
  }
  if (!s.grow(off)) {
    fprintf(stderr, "[srsran_phy_hip] %s: staging allocation of %zu bytes failed\n", who, off);
    return SRSRAN_ERROR;
  }
  memcpy(s.pin, jobs.data(), (size_t)n * sizeof(conv::VitJob));
  for (uint32_t i = 0; i < n; i++) {
    memcpy(s.pin + jobs[i].o_in, f[i].in, (size_t)3 * (f[i].L + (tail ? 0 : 6)) * es);
  }
  const auto enqueue = [&](hipStream_t st) { return conv::launch_viterbi(s.dev, reinterpret_cast<const conv::VitJob*>(s.dev.get()), s.dev, n, Lmax, tail, st); };
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, off - up, enqueue)) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < n; i++) {
    memcpy(f[i].out, s.pin + jobs[i].o_out, f[i].L);
  }
  return (int)q->framebits;
}

// the reference's checks in front of a decode (viterbi.c:551-554, :135-138): -1 with its line on stderr
bool handle_takes(const char* who, const srsran_viterbi_t* q, const void* symbols, const uint8_t* data, uint32_t frame_length, int* rc)
{
  if (!q || !q->ptr || !symbols || !data) {
    fprintf(stderr, "[srsran_phy_hip] %s: NULL argument or a handle that was not initialised\n", who);
    *rc = SRSRAN_ERROR;
    return false;
  }
  if (frame_length > q->framebits || frame_length == 0) {
    fprintf(stderr, "[srsran_phy_hip] %s: Initialized decoder for max frame length %u bits\n", who, q->framebits);
    *rc = -1;
    return false;
  }
  return true;
}

int decode_us(const char* who, srsran_viterbi_t* q, const uint16_t* symbols, uint8_t* data, uint32_t frame_length)
{
  const Frame f = {symbols, data, frame_length};
  return run_frames(who, q, conv::IN_US, &f, 1);
}

} // namespace

extern "C" int srsran_viterbi_init(srsran_viterbi_t* q, srsran_viterbi_type_t type, int poly[3], uint32_t max_frame_length, bool tail_bitting)
{
  if (!q) {
    return -1;
  }
  memset(q, 0, sizeof(*q));
  if (type != SRSRAN_VITERBI_37) {
    fprintf(stderr, "[srsran_phy_hip] srsran_viterbi_init: Decoder not implemented\n");
    return -1;
  }
  if (!poly || poly[0] != 0x6D || poly[1] != 0x4F || poly[2] != 0x57) {
    fprintf(stderr, "[srsran_phy_hip] srsran_viterbi_init: only the polynomials (0x6D, 0x4F, 0x57) of the LTE code are implemented\n");
    return -1;
  }
  if (max_frame_length == 0 || max_frame_length > conv::kMaxFrame) {
    fprintf(stderr, "[srsran_phy_hip] srsran_viterbi_init: max_frame_length %u is outside 1 .. %u (the decision words of a frame live in LDS)\n", max_frame_length,
            conv::kMaxFrame);
    return -1;
  }
  q->ptr          = &handle_tag;
  q->K            = 7;
  q->R            = 3;
  q->framebits    = max_frame_length;
  q->gain_quant_s = 4;
  q->gain_quant   = 1000.f; // DEFAULT_GAIN_16
  q->tail_biting  = tail_bitting;
  return 0;
}

extern "C" void srsran_viterbi_set_gain_quant(srsran_viterbi_t* q, float gain_quant)
{
  q->gain_quant = gain_quant;
}

extern "C" void srsran_viterbi_set_gain_quant_s(srsran_viterbi_t* q, int16_t gain_quant)
{
  q->gain_quant_s = gain_quant;
}

extern "C" void srsran_viterbi_free(srsran_viterbi_t* q)
{
  if (q) {
    memset(q, 0, sizeof(*q));
  }
}

extern "C" int srsran_viterbi_decode_f(srsran_viterbi_t* q, float* symbols, uint8_t* data, uint32_t frame_length)
{
  int rc;
  if (!handle_takes("srsran_viterbi_decode_f", q, symbols, data, frame_length, &rc)) {
    return rc;
  }
  const Frame f = {symbols, data, frame_length};
  return run_frames("srsran_viterbi_decode_f", q, conv::IN_F32, &f, 1); // max and quantiser on the device
}

extern "C" int srsran_viterbi_decode_s(srsran_viterbi_t* q, int16_t* symbols, uint8_t* data, uint32_t frame_length)
{
  int rc;
  if (!handle_takes("srsran_viterbi_decode_s", q, symbols, data, frame_length, &rc)) {
    return rc;
  }
  // srsran_vec_quant_sus(symbols, ., 1, 32767, 65535): (int32)(32767.f + (float)x) is exact, so integers do
  const uint32_t        len = 3 * (frame_length + (q->tail_biting ? 0 : 6));
  std::vector<uint16_t> us(len);
  for (uint32_t i = 0; i < len; i++) {
    const int32_t v = 32767 + (int32_t)symbols[i];
    us[i]           = (uint16_t)(v < 0 ? 0 : v);
  }
  return decode_us("srsran_viterbi_decode_s", q, us.data(), data, frame_length);
}

extern "C" int srsran_viterbi_decode_us(srsran_viterbi_t* q, uint16_t* symbols, uint8_t* data, uint32_t frame_length)
{
  int rc;
  if (!handle_takes("srsran_viterbi_decode_us", q, symbols, data, frame_length, &rc)) {
    return rc;
  }
  return decode_us("srsran_viterbi_decode_us", q, symbols, data, frame_length);
}

extern "C" int srsran_viterbi_decode_uc(srsran_viterbi_t*, uint8_t*, uint8_t*, uint32_t)
{
  return SRSRAN_ERROR; // the reference's 16-bit object leaves q->decode NULL (viterbi.c:619-628)
}

extern "C" int srsran_hip_viterbi_decode_us_multi(srsran_viterbi_t* q, uint32_t n, const uint16_t* const* symbols, uint8_t* const* data, const uint32_t* frame_length)
{
  const char* who = "srsran_hip_viterbi_decode_us_multi";
  if (n == 0) {
    return q ? (int)q->framebits : 0;
  }
  bool bad = !q || !q->ptr || !symbols || !data || !frame_length || n > SRSRAN_HIP_PDCCH_MAX_CANDIDATES;
  for (uint32_t i = 0; !bad && i < n; i++) {
    bad = !symbols[i] || !data[i] || frame_length[i] == 0 || frame_length[i] > q->framebits;
  }
  if (bad) {
    fprintf(stderr, "[srsran_phy_hip] %s: NULL argument, more than %d frames or a frame length outside 1 .. framebits\n", who, SRSRAN_HIP_PDCCH_MAX_CANDIDATES);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  std::vector<Frame> f(n);
  for (uint32_t i = 0; i < n; i++) {
    f[i] = Frame{symbols[i], data[i], frame_length[i]};
  }
  return run_frames(who, q, conv::IN_US, f.data(), n);
}

// ------------------------------------------------------------------------------------------------ PDCCH candidates
static int pdcch_multi(const char* who, const float* llr, uint32_t nof_llr, uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res, float* rm_f,
                       uint16_t* symbols)
{
  TraceRange trace_(who);
  if (n == 0) {
    return SRSRAN_SUCCESS;
  }
  const char* why = nullptr;
  if (!llr || !cand || !res) {
    why = "NULL argument";
  } else if (n > SRSRAN_HIP_PDCCH_MAX_CANDIDATES) {
    why = "more than 256 candidates";
  }
  if (!why) {
    memset(res, 0, (size_t)n * sizeof(*res));
    for (uint32_t i = 0; i < n && !why; i++) {
      why = conv::dci_cand_invalid(cand[i], nof_llr);
    }
  }
  if (why) {
    return call::refused(who, why);
  }
  if (rm_f) {
    memset(rm_f, 0, (size_t)n * conv::kDciSyms * sizeof(float));
  }
  if (symbols) {
    memset(symbols, 0, (size_t)n * conv::kDciSyms * sizeof(uint16_t));
  }
  // the rule of srsran_pdcch_decode_msg (pdcch.c:388-393) on the caller's array: a double sum in index order
  std::vector<conv::DciJob> jobs;
  std::vector<uint32_t>     slot;
  jobs.reserve(n);
  slot.reserve(n);
  for (uint32_t i = 0; i < n; i++) {
    const conv::DciJob job  = conv::dci_job(cand[i]);
    double             mean = 0;
    for (uint32_t k = 0; k < job.E; k++) {
      mean += fabsf(llr[job.first + k]);
    }
    mean /= job.E;
    res[i].mean = (float)mean;
    if (mean > 0.3) {
      jobs.push_back(job);
      slot.push_back(i);
    }
  }
  const uint32_t m = (uint32_t)jobs.size();
  if (m == 0) {
    return SRSRAN_SUCCESS;
  }
  ConvStage& s = conv_stage();
  if (!s.ready()) {
    memset(res, 0, (size_t)n * sizeof(*res));
    return call::no_device(who);
  }
  const bool   dbg   = rm_f || symbols;
  const size_t o_llr = al256((size_t)m * sizeof(conv::DciJob)), up = al256(o_llr + (size_t)nof_llr * sizeof(float));
  const size_t o_rm  = al256(up + (size_t)m * conv::kDciOutRow), o_sym = dbg ? al256(o_rm + (size_t)m * conv::kDciSyms * sizeof(float)) : o_rm;
  const size_t end   = dbg ? al256(o_sym + (size_t)m * conv::kDciSyms * sizeof(uint16_t)) : o_rm;
  if (!s.grow(end)) {
    fprintf(stderr, "[srsran_phy_hip] %s: staging allocation of %zu bytes failed\n", who, end);
    memset(res, 0, (size_t)n * sizeof(*res));
    return SRSRAN_ERROR;
  }
  memcpy(s.pin, jobs.data(), (size_t)m * sizeof(conv::DciJob));
  memcpy(s.pin + o_llr, llr, (size_t)nof_llr * sizeof(float));
  const auto enqueue = [&](hipStream_t st) {
    return conv::launch_pdcch_dci(reinterpret_cast<const float*>(s.dev + o_llr), reinterpret_cast<const conv::DciJob*>(s.dev.get()), s.dev + up,
                                  dbg ? reinterpret_cast<float*>(s.dev + o_rm) : nullptr, dbg ? reinterpret_cast<uint16_t*>(s.dev + o_sym) : nullptr, m, st);
  };
  if (!call::round_trip(who, s.st, s.pin, s.dev, up, up, end - up, enqueue)) {
    memset(res, 0, (size_t)n * sizeof(*res));
    return SRSRAN_ERROR;
  }
  for (uint32_t j = 0; j < m; j++) {
    const uint8_t*          row = s.pin + up + (size_t)j * conv::kDciOutRow;
    srsran_hip_pdcch_res_t& r   = res[slot[j]];
    memcpy(r.payload, row, conv::kDciBits);
    r.crc_rem = (uint16_t)(row[conv::kDciBits] | (row[conv::kDciBits + 1] << 8));
    r.decoded = 1;
    if (rm_f) {
      memcpy(rm_f + (size_t)slot[j] * conv::kDciSyms, s.pin + o_rm + (size_t)j * conv::kDciSyms * sizeof(float), conv::kDciSyms * sizeof(float));
    }
    if (symbols) {
      memcpy(symbols + (size_t)slot[j] * conv::kDciSyms, s.pin + o_sym + (size_t)j * conv::kDciSyms * sizeof(uint16_t), conv::kDciSyms * sizeof(uint16_t));
    }
  }
  return SRSRAN_SUCCESS;
}

extern "C" int srsran_hip_pdcch_dci_decode_multi(const float* llr, uint32_t nof_llr, uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res)
{
  return pdcch_multi("srsran_hip_pdcch_dci_decode_multi", llr, nof_llr, n, cand, res, nullptr, nullptr);
}

extern "C" int srsran_hip_pdcch_dci_decode_multi_dbg(const float* llr, uint32_t nof_llr, uint32_t n, const srsran_hip_pdcch_cand_t* cand, srsran_hip_pdcch_res_t* res,
                                                     float* rm_f, uint16_t* symbols)
{
  return pdcch_multi("srsran_hip_pdcch_dci_decode_multi_dbg", llr, nof_llr, n, cand, res, rm_f, symbols);
}
