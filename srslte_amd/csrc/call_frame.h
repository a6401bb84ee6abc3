// call_frame.h -- the frame of an entry point that is ONE device call: the plain staging context, the three messages, and the round trip -- upload, the
// call's launches, download, one host wait.  The wait is taken ALSO after a failed step: nothing of a failed call is in flight when the next one reuses the images.
#pragma once
#include "stage.h"

#include <string>

namespace phyhip {
namespace call {

// stream, pinned image, device buffer.  A family derives its own type (struct CtrlStage : call::Stage {}) and keeps its own StageRef pool.
struct Stage {
  StageStream st;
  HostImage   pin;
  DeviceBuf   dev;
  bool        ready() { return st.open(); }
  bool        grow(size_t need_pin, size_t need_dev) { return pin.grow(need_pin, need_pin / 2) && dev.grow(need_dev, need_dev / 2); }
  bool        grow(size_t need) { return grow(need, need); }
};

// one line on stderr each; none of them sets the last-error text
inline int refused(const char* who, const char* why)
{
  fprintf(stderr, "[srsran_phy_hip] %s: %s\n", who, why);
  return SRSRAN_ERROR_INVALID_INPUTS;
}
inline int failed(const char* who, const char* what)
{
  fprintf(stderr, "[srsran_phy_hip] %s: %s\n", who, what);
  return SRSRAN_ERROR;
}
inline int no_device(const char* who) // behind a context's ready() == false
{
  return failed(who, (std::string(get_error()) + " (there is no CPU fallback)").c_str());
}

inline int device_failed(const char* who, hipError_t e) // the last-error text is "who: the device's error" and stands on stderr, one line
{
  set_error("%s: %s", who, hipGetErrorString(e));
  fprintf(stderr, "[srsran_phy_hip] %s\n", get_error());
  return SRSRAN_ERROR;
}

// the call's one host wait; the first error of what was enqueued (e) and the wait
inline hipError_t settle(hipError_t e, hipStream_t st)
{
  const hipError_t w = hipStreamSynchronize(st);
  return e != hipSuccess ? e : w;
}

// [0, up_bytes) of pin to dev, enqueue(st) -- the call's launches chained, the first error returned --, [down_off, down_off + down_bytes) of dev to pin, settle.
// false: device_failed(who, the first error).
template <class Enqueue>
bool round_trip(const char* who, hipStream_t st, uint8_t* pin, uint8_t* dev, size_t up_bytes, size_t down_off, size_t down_bytes, Enqueue&& enqueue)
{
  hipError_t e = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    e = enqueue(st);
  }
  if (e == hipSuccess && down_bytes) {
    e = hipMemcpyAsync(pin + down_off, dev + down_off, down_bytes, hipMemcpyDeviceToHost, st);
  }
  e = settle(e, st);
  if (e != hipSuccess) {
    device_failed(who, e);
  }
  return e == hipSuccess;
}

} // namespace call
} // namespace phyhip
