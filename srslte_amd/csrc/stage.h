// stage.h -- what a per-thread staging context is made of: its stream and its growable images.  What else a context holds (decoder and encoder objects,
// transform plans) and who owns it -- a StagePool (hip_common.h) for the contexts srsran_hip_warmup() prepares, thread_device_local for the rest -- is
// the business of the file that defines it.
#pragma once
#include "hip_common.h"

namespace phyhip {

inline size_t al256(size_t v) // the next multiple of 256: the alignment of every region of a staging image
{
  return (v + 255) & ~(size_t)255;
}

// true when the n bytes at p (8-byte aligned, as the rows of a soft buffer are) are all zero: a row straight after srsran_softbuffer_rx_reset
// is not worth a copy, let alone a transfer.  Read-only, four independent accumulators (vectorises), early exit per 4 KB.
inline bool all_zero(const uint8_t* p, size_t n)
{
  size_t i = 0;
  if ((reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
    const size_t    w = n / 8;
    for (size_t j = 0; j < w;) {
      const size_t e = j + 512 < w ? j + 512 : w;
      uint64_t     a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      for (; j + 4 <= e; j += 4) {
        a0 |= q[j], a1 |= q[j + 1], a2 |= q[j + 2], a3 |= q[j + 3];
      }
      for (; j < e; j++) {
        a0 |= q[j];
      }
      if (a0 | a1 | a2 | a3) {
        return false;
      }
    }
    i = w * 8;
  }
  for (; i < n; i++) {
    if (p[i]) {
      return false;
    }
  }
  return true;
}

// The context's stream: hipStreamNonBlocking, created by the first open() on the device the calling thread is bound to and destroyed with its owner.
// Creation is tried ONCE (device_available() is sticky: a later call would find what the first one found).  Converts to the stream it holds: nullptr
// until open() has succeeded, and always without a device.
class StageStream {
public:
  StageStream()                              = default;
  StageStream(const StageStream&)            = delete;
  StageStream& operator=(const StageStream&) = delete;
  ~StageStream()
  {
    if (st_) {
      (void)hipStreamDestroy(st_);
    }
  }
  bool open()
  {
    if (!tried_) {
      tried_ = true;
      if (device_available()) {
        bind_thread();
        if (hipStreamCreateWithFlags(&st_, hipStreamNonBlocking) != hipSuccess) {
          st_ = nullptr;
        }
      }
    }
    return st_ != nullptr;
  }
  operator hipStream_t() const { return st_; }

private:
  hipStream_t st_    = nullptr;
  bool        tried_ = false;
};

// A buffer of T that only grows, in device memory or as a pinned host image the kernels work on themselves (host_image_alloc).  grow(need) leaves a
// buffer that holds `need` elements alone; a smaller one is FREED and need + headroom elements are allocated -- the contents are not kept, and a failed
// allocation leaves nullptr and capacity 0.  How much headroom a request gets is the site's policy (pinned memory is dear to re-allocate, and the
// first-call latencies on record were measured with these policies).  Converts to the pointer it holds.
enum class StageMem { Device, HostImage };
template <StageMem M, class T = uint8_t>
class StageBuf {
public:
  StageBuf()                           = default;
  StageBuf(const StageBuf&)            = delete;
  StageBuf& operator=(const StageBuf&) = delete;
  ~StageBuf() { release(); }
  bool grow(size_t need, size_t headroom = 0)
  {
    if (need <= cap_) {
      return true;
    }
    release();
    const size_t     n = need + headroom;
    const hipError_t e = M == StageMem::Device ? hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)) : host_image_alloc(&p_, n * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return false;
    }
    cap_ = n;
    return true;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

private:
  void release()
  {
    (void)(M == StageMem::Device ? hipFree(p_) : hipHostFree(p_));
    p_   = nullptr;
    cap_ = 0;
  }
  T*     p_   = nullptr;
  size_t cap_ = 0; // elements
};
using DeviceBuf = StageBuf<StageMem::Device>;
using HostImage = StageBuf<StageMem::HostImage>;

namespace rm {
bool build_all_tables(); // every rate-matching table in one allocation and one upload (rm_host.cpp): what srsran_hip_warmup (warmup_host.cpp) starts with
}

} // namespace phyhip
